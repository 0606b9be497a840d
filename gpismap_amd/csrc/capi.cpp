// C-ABI (include/gpismap_amd.h) over the C++ classes.  Nothing throws across it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/GPisMap.h"
#include "../../include/GPisMap3.h"
#include "../../include/gpismap_amd.h"
#include "map_query.h"
#include "mesh.h"
#include "dfield.h"
#include "render.h"
#include "track.h"
#include "locate.h"
#include "pf.h"
#include "plan.h"
#include "pplan.h"
#include "tplan.h"
#include "tpplan.h"
#include "traj.h"
#include "mppi.h"
#include "obst.h"
#include "body.h"
#include "cover.h"
#include "detect.h"
#include "view.h"
#include "obsgp.h"
#include "ongpis.h"

using namespace gpis;

// accessors implemented in gpismap3.cpp
void gpis3_impl_stats(GPisMap3* m, double* out, int n);
void gpis3_impl_profile(GPisMap3* m, int on);
void gpis2_impl_stats(GPisMap* m, double* out, int n);
void gpis3_impl_pass_jobs(GPisMap3* m, long long* out);
void gpis2_impl_pass_jobs(GPisMap* m, long long* out);
void gpis3_impl_pass_detail(GPisMap3* m, double* out);
void gpis2_impl_pass_detail(GPisMap* m, double* out);
int gpis3_impl_set_pass2_mode(GPisMap3* m, int mode);
int gpis3_impl_set_k4_schedule(GPisMap3* m, int mode);
int gpis2_impl_set_pass2_mode(GPisMap* m, int mode);
int gpis3_impl_fail(GPisMap3* m);
int gpis2_impl_fail(GPisMap* m);
int gpis3_impl_update_fail(GPisMap3* m);
int gpis3_impl_sync(GPisMap3* m);
void gpis3_impl_set_pipeline(GPisMap3* m, int on);
void gpis3_impl_set_host_gather(GPisMap3* m, int on);
void gpis3_impl_set_keep_factors(GPisMap3* m, int on);
void gpis3_impl_set_shard_factors(GPisMap3* m, int mode);
int gpis3_impl_prepare_test(GPisMap3* m);
void gpis3_impl_set_lazy_inverse(GPisMap3* m, int on);
int gpis2_impl_update_fail(GPisMap* m);
int gpis3_impl_device(GPisMap3* m);
int gpis3_impl_num_devices(GPisMap3* m);
GPisMap3* gpis3_impl_create_on(const GPisMap3Param& par, const camParam& c, const int* devices, int n);
int gpis3_impl_set_shard(GPisMap3* m, int rank, int world);
int gpis3_impl_shard_info(GPisMap3* m, int* out, int n);
long long gpis3_impl_shard_bytes(GPisMap3* m, int owner);
int gpis3_impl_shard_pack(GPisMap3* m, void* d_buf, void* stream);
int gpis3_impl_shard_unpack(GPisMap3* m, int owner, const void* d_buf, void* stream);
int gpis3_impl_shard_finish(GPisMap3* m);
int gpis3_impl_set_frame_export(GPisMap3* g, int on);
long long gpis3_impl_frame_record(GPisMap3* g, void* buf, long long cap);
int gpis3_impl_train_deferred(GPisMap3* g);
int gpis3_impl_apply_frame(GPisMap3* g, const void* buf, long long bytes);
int gpis2_impl_device(GPisMap* m);
int gpis2_impl_sync(GPisMap* m);
void gpis2_impl_set_pipeline(GPisMap* m, int on);
int gpis3_impl_extract(GPisMap3* g, MeshExtractor& me, const int* n3, const float* origin3, const float* step3, float level, void* stream);
int gpis2_impl_extract(GPisMap* g, MeshExtractor& me, const int* n2, const float* origin2, const float* step2, float level, void* stream);
int gpis3_impl_dfield(GPisMap3* g, DistanceField& df, const int* n3, const float* origin3, const float* step3, float level, float max_var,
                      void* stream);
int gpis2_impl_dfield(GPisMap* g, DistanceField& df, const int* n2, const float* origin2, const float* step2, float level, float max_var,
                      void* stream);
int gpis3_impl_render(GPisMap3* g, Renderer& r, const SensorFrame& f, const float* pose12, RenderOpts o, void* stream);
int gpis2_impl_render(GPisMap* g, Renderer& r, const SensorFrame& f, const float* pose6, RenderOpts o, void* stream);
int gpis3_impl_track(GPisMap3* g, Tracker& t, const SensorFrame& f, const float* depth, const float* pose12, TrackOpts o,
                     float* pose12_out, void* stream);
int gpis2_impl_track(GPisMap* g, Tracker& t, const SensorFrame& f, const float* ranges, const float* pose6, TrackOpts o,
                     float* pose6_out, void* stream);
void gpis3_impl_camera(GPisMap3* g, float* cam4, int* wh);
void gpis2_impl_sensor_offset(GPisMap* g, float* off2);

// The frame of an entry (frame.h): the caller's camera / sensor offset, else the map's.  Checked once, here, for every consumer.
static int depth_frame(void* m, const gpis_cam* cam, SensorFrame* f) {
    float c4[4];
    int wh[2];
    if (cam) { c4[0] = cam->fx; c4[1] = cam->fy; c4[2] = cam->cx; c4[3] = cam->cy; wh[0] = cam->width; wh[1] = cam->height; }
    else gpis3_impl_camera((GPisMap3*)m, c4, wh);
    return frame_from_camera(c4, wh, f);
}
static int scan_frame(void* m, const float* thetas, int n, const float* off2, SensorFrame* f) {
    float off[2];
    if (off2) { off[0] = off2[0]; off[1] = off2[1]; }
    else gpis2_impl_sensor_offset((GPisMap*)m, off);
    return frame_from_scan(thetas, n, off, f);
}

namespace gpis { int selftest_ranged_arith(unsigned long long seed, int blocks, int per_thread, int mode, unsigned long long* mismatches); }
extern "C" {

int gpis_selftest_ranged_arith(unsigned long long seed, int blocks, int per_thread, int mode, unsigned long long* mismatches2) {
    try { return gpis::selftest_ranged_arith(seed, blocks, per_thread, mode, mismatches2); } catch (...) { return GPIS_ERR_STATE; }
}
unsigned long long gpis_pool_cache_trim(void) { try { return (unsigned long long)gpis::pool_cache_trim(); } catch (...) { return 0; } }
int gpis_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char* gpis_version(void) { return "gpismap_amd 0.2 (gfx950)"; }
int gpis_set_device(int device) {
    int n = gpis_device_count();
    if (device < 0 || device >= n) return GPIS_ERR_ARG;
    return hipSetDevice(device) == hipSuccess ? GPIS_OK : GPIS_ERR_HIP;
}
int gpis_get_device(void) {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) return GPIS_ERR_HIP;
    return d;
}

// ---- 3-D map ----------------------------------------------------------------
void* gpis3_create(const gpis_cam* cam) {
    try {
        GPisMap3Param p;
        if (cam) { camParam c(cam->fx, cam->fy, cam->cx, cam->cy, (float)cam->width, (float)cam->height); return new GPisMap3(p, c); }
        return new GPisMap3(p);
    } catch (...) { return nullptr; }
}
void* gpis3_create_multi(const gpis_cam* cam, const int* devices, int n) {
    if (!devices || n < 1) return nullptr;
    try {
        GPisMap3Param p;
        camParam c;
        if (cam) c = camParam(cam->fx, cam->fy, cam->cx, cam->cy, (float)cam->width, (float)cam->height);
        return gpis3_impl_create_on(p, c, devices, n);
    } catch (...) { return nullptr; }
}
int gpis3_num_devices(void* m) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_num_devices((GPisMap3*)m); }
void gpis3_destroy(void* m) { delete (GPisMap3*)m; }
int gpis3_reset(void* m) { if (!m) return GPIS_ERR_ARG; ((GPisMap3*)m)->reset(); return GPIS_OK; }
int gpis3_set_camera(void* m, const gpis_cam* cam) {
    if (!m || !cam) return GPIS_ERR_ARG;
    camParam c(cam->fx, cam->fy, cam->cx, cam->cy, (float)cam->width, (float)cam->height);
    ((GPisMap3*)m)->resetCam(c);
    return GPIS_OK;
}
int gpis3_update(void* m, const float* depth, int n, const float* pose12) {
    if (!m || !depth || !pose12) return GPIS_ERR_ARG;
    if (gpis_device_count() < 1) return GPIS_ERR_HIP;
    try {
        std::vector<float> pose(pose12, pose12 + 12);
        ((GPisMap3*)m)->update(const_cast<float*>(depth), n, pose);
    } catch (...) { return GPIS_ERR_STATE; }
    return gpis3_impl_update_fail((GPisMap3*)m);   // 0 unless a device step inside failed (bad input is silent, as in the reference)
}
int gpis3_test(void* m, const float* x, int dim, int n, float* res) {
    if (!m) return GPIS_ERR_ARG;
    if (gpis_device_count() < 1) return GPIS_ERR_HIP;
    // false = the reference's own refusal (GPIS_ERR_ARG) unless the device path failed: that is reported as such
    try { if (((GPisMap3*)m)->test(const_cast<float*>(x), dim, n, res)) return GPIS_OK; int e = gpis3_impl_fail((GPisMap3*)m); return e ? e : GPIS_ERR_ARG; }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis3_test_device(void* m, const float* d_x, int n, float* d_res, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    try { if (((GPisMap3*)m)->testDevice(d_x, n, d_res, stream)) return GPIS_OK; int e = gpis3_impl_fail((GPisMap3*)m); return e ? e : GPIS_ERR_ARG; }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis3_device(void* m) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_device((GPisMap3*)m); }
int gpis3_set_shard(void* m, int rank, int world) {
    if (!m || world < 1 || rank < 0 || rank >= world) return GPIS_ERR_ARG;
    return gpis3_impl_set_shard((GPisMap3*)m, rank, world);
}
int gpis3_shard_info(void* m, int* out, int n) { if (!m || !out) return GPIS_ERR_ARG; return gpis3_impl_shard_info((GPisMap3*)m, out, n); }
long long gpis3_shard_bytes(void* m, int owner) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_shard_bytes((GPisMap3*)m, owner); }
int gpis3_shard_pack(void* m, void* d_buf, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    return gpis3_impl_shard_pack((GPisMap3*)m, d_buf, stream);
}
int gpis3_shard_unpack(void* m, int owner, const void* d_buf, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    return gpis3_impl_shard_unpack((GPisMap3*)m, owner, d_buf, stream);
}
int gpis3_shard_finish(void* m) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_shard_finish((GPisMap3*)m); }
int gpis3_set_frame_export(void* m, int on) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_set_frame_export((GPisMap3*)m, on); }
long long gpis3_frame_record(void* m, void* buf, long long cap) { if (!m || cap < 0) return GPIS_ERR_ARG; return gpis3_impl_frame_record((GPisMap3*)m, buf, cap); }
int gpis3_train_deferred(void* m) { if (!m) return GPIS_ERR_ARG; try { return gpis3_impl_train_deferred((GPisMap3*)m); } catch (...) { return GPIS_ERR_STATE; } }
int gpis3_apply_frame(void* m, const void* buf, long long bytes) { if (!m) return GPIS_ERR_ARG; return gpis3_impl_apply_frame((GPisMap3*)m, buf, bytes); }
int gpis3_num_points(void* m) {
    if (!m) return GPIS_ERR_ARG;
    std::vector<float> p; ((GPisMap3*)m)->getAllPoints(p); return (int)(p.size() / 3);
}
int gpis3_get_points(void* m, float* out, int cap) {
    if (!m) return GPIS_ERR_ARG;
    std::vector<float> p; ((GPisMap3*)m)->getAllPoints(p);
    int n = (int)(p.size() / 3);
    if (out && n <= cap && n > 0) std::memcpy(out, p.data(), p.size() * sizeof(float));
    return n;
}
int gpis3_get_nodes(void* m, float* out, int cap) {
    if (!m) return GPIS_ERR_ARG;
    std::vector<float> p; ((GPisMap3*)m)->getAllNodes(p);
    int n = (int)(p.size() / 9);
    if (out && n <= cap && n > 0) std::memcpy(out, p.data(), p.size() * sizeof(float));
    return n;
}
int gpis3_save(void* m, const char* path) { if (!m || !path) return GPIS_ERR_ARG; return ((GPisMap3*)m)->saveMap(path) ? GPIS_OK : GPIS_ERR_ARG; }
int gpis3_load(void* m, const char* path) {
    if (!m || !path) return GPIS_ERR_ARG;
    if (((GPisMap3*)m)->loadMap(path)) return GPIS_OK;
    const int rc = gpis3_impl_update_fail((GPisMap3*)m);
    return rc ? rc : GPIS_ERR_ARG;
}
int gpis3_stats(void* m, double* out, int n) { if (!m || !out) return GPIS_ERR_ARG; gpis3_impl_stats((GPisMap3*)m, out, n); return GPIS_OK; }
int gpis3_pass_jobs(void* m, long long* out4) { if (!m || !out4) return GPIS_ERR_ARG; gpis3_impl_pass_jobs((GPisMap3*)m, out4); return GPIS_OK; }
int gpis3_pass_detail(void* m, double* out8) { if (!m || !out8) return GPIS_ERR_ARG; gpis3_impl_pass_detail((GPisMap3*)m, out8); return GPIS_OK; }
int gpis3_set_k4_schedule(void* m, int mode) { if (!m || mode < 0 || mode > 1) return GPIS_ERR_ARG; return gpis3_impl_set_k4_schedule((GPisMap3*)m, mode); }
int gpis3_set_pass2_mode(void* m, int mode) { if (!m || mode < 0 || mode > 4) return GPIS_ERR_ARG; return gpis3_impl_set_pass2_mode((GPisMap3*)m, mode); }
int gpis3_sync(void* m) { if (!m) return GPIS_ERR_ARG; try { return gpis3_impl_sync((GPisMap3*)m); } catch (...) { return GPIS_ERR_STATE; } }
int gpis3_set_pipeline(void* m, int on) { if (!m) return GPIS_ERR_ARG; try { gpis3_impl_set_pipeline((GPisMap3*)m, on); return GPIS_OK; } catch (...) { return GPIS_ERR_STATE; } }
int gpis3_set_host_gather(void* m, int on) { if (!m) return GPIS_ERR_ARG; gpis3_impl_set_host_gather((GPisMap3*)m, on); return GPIS_OK; }
int gpis3_set_shard_factors(void* m, int mode) { if (!m) return GPIS_ERR_ARG; gpis3_impl_set_shard_factors((GPisMap3*)m, mode); return GPIS_OK; }
int gpis3_set_keep_factors(void* m, int on) { if (!m) return GPIS_ERR_ARG; try { gpis3_impl_set_keep_factors((GPisMap3*)m, on); return GPIS_OK; } catch (...) { return GPIS_ERR_STATE; } }
int gpis3_prepare_test(void* m) { if (!m) return GPIS_ERR_ARG; try { return gpis3_impl_prepare_test((GPisMap3*)m); } catch (...) { return GPIS_ERR_STATE; } }
int gpis3_set_lazy_inverse(void* m, int on) { if (!m) return GPIS_ERR_ARG; gpis3_impl_set_lazy_inverse((GPisMap3*)m, on); return GPIS_OK; }
int gpis3_set_profile(void* m, int on) { if (!m) return GPIS_ERR_ARG; gpis3_impl_profile((GPisMap3*)m, on); return GPIS_OK; }

// ---- 2-D map ----------------------------------------------------------------
void* gpis2_create(void) { try { return new GPisMap(); } catch (...) { return nullptr; } }
void gpis2_destroy(void* m) { delete (GPisMap*)m; }
int gpis2_reset(void* m) { if (!m) return GPIS_ERR_ARG; ((GPisMap*)m)->reset(); return GPIS_OK; }
int gpis2_update(void* m, const float* thetas, const float* ranges, int n, const float* pose6) {
    if (!m || !thetas || !ranges || !pose6) return GPIS_ERR_ARG;
    if (gpis_device_count() < 1) return GPIS_ERR_HIP;
    try {
        std::vector<float> pose(pose6, pose6 + 6);
        ((GPisMap*)m)->update(const_cast<float*>(thetas), const_cast<float*>(ranges), n, pose);
    } catch (...) { return GPIS_ERR_STATE; }
    return gpis2_impl_update_fail((GPisMap*)m);
}
int gpis2_test(void* m, const float* x, int dim, int n, float* res) {
    if (!m) return GPIS_ERR_ARG;
    if (gpis_device_count() < 1) return GPIS_ERR_HIP;
    try { if (((GPisMap*)m)->test(const_cast<float*>(x), dim, n, res)) return GPIS_OK; int e = gpis2_impl_fail((GPisMap*)m); return e ? e : GPIS_ERR_ARG; }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis2_test_device(void* m, const float* d_x, int n, float* d_res, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    try { if (((GPisMap*)m)->testDevice(d_x, n, d_res, stream)) return GPIS_OK; int e = gpis2_impl_fail((GPisMap*)m); return e ? e : GPIS_ERR_ARG; }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis2_device(void* m) { if (!m) return GPIS_ERR_ARG; return gpis2_impl_device((GPisMap*)m); }
int gpis2_sync(void* m) { if (!m) return GPIS_ERR_ARG; try { return gpis2_impl_sync((GPisMap*)m); } catch (...) { return GPIS_ERR_STATE; } }
int gpis2_set_pipeline(void* m, int on) { if (!m) return GPIS_ERR_ARG; try { gpis2_impl_set_pipeline((GPisMap*)m, on); } catch (...) { return GPIS_ERR_STATE; } return GPIS_OK; }
int gpis2_get_nodes(void* m, float* out, int cap) {
    if (!m) return GPIS_ERR_ARG;
    std::vector<float> p; ((GPisMap*)m)->getAllNodes(p);
    int n = (int)(p.size() / 7);
    if (out && n <= cap && n > 0) std::memcpy(out, p.data(), p.size() * sizeof(float));
    return n;
}
int gpis2_stats(void* m, double* out, int n) { if (!m || !out) return GPIS_ERR_ARG; gpis2_impl_stats((GPisMap*)m, out, n); return GPIS_OK; }
int gpis2_pass_jobs(void* m, long long* out4) { if (!m || !out4) return GPIS_ERR_ARG; gpis2_impl_pass_jobs((GPisMap*)m, out4); return GPIS_OK; }
int gpis2_pass_detail(void* m, double* out8) { if (!m || !out8) return GPIS_ERR_ARG; gpis2_impl_pass_detail((GPisMap*)m, out8); return GPIS_OK; }
int gpis2_set_pass2_mode(void* m, int mode) { if (!m || mode < 0 || mode > 4) return GPIS_ERR_ARG; return gpis2_impl_set_pass2_mode((GPisMap*)m, mode); }

// ---- ObsGP --------------------------------------------------------------------
struct ObsHandle { int device = -1; ObsGPDevice g; hipStream_t s = nullptr; hipStream_t sb = nullptr; int nb = -1; };   // sb: the second staging set's stream, nb: queries of its batch not collected yet, -1 none (gpis_obsgp_query_route)
void* gpis_obsgp_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    ObsHandle* h = new (std::nothrow) ObsHandle();
    if (h) (void)hipGetDevice(&h->device);
    if (h && hipStreamCreate(&h->s) != hipSuccess) { delete h; return nullptr; }
    return h;
}
void gpis_obsgp_destroy(void* g) { if (!g) return; ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device); (void)h->g.wait_b(); if (h->sb) (void)hipStreamDestroy(h->sb); if (h->s) (void)hipStreamDestroy(h->s); delete h; }
int gpis_obsgp_train2d(void* g, const float* vu, const float* f, int ni, int nj) {
    if (!g) return GPIS_ERR_ARG; ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device); return h->g.train2d(vu, f, ni, nj, h->s);
}
int gpis_obsgp_train1d(void* g, const float* th, const float* f, int n) {
    if (!g) return GPIS_ERR_ARG; ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device); return h->g.train1d(th, f, n, h->s);
}
int gpis_obsgp_query(void* g, const float* q, int nq, float* val, float* var) {
    if (!g || !q || !val || !var) return GPIS_ERR_ARG; ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device); return h->g.query(q, nq, val, var, h->s);
}
// One batch through one of the routes the maps' update() takes (kernel-level tests of the staging paths):
//   0  query()                                   val is read and written (untouched where no group answers)
//   1  stage_q() + query_staged()                val starts from 0; below 4096 queries the kernel works on the page-locked staging itself
//   2  stage_qb() + query_staged_b_async() + wait_b(), the batch on a stream of its own as in update(); val starts from 0
//   3  the first half of route 2: returns with the batch pending (val / var are not touched)
//   4  the second half: wait_b() and the answers of the batch route 3 left behind (q is not read); GPIS_ERR_STATE when there is
//      none, GPIS_ERR_ARG when nq is not that batch's size
int gpis_obsgp_query_route(void* g, int route, const float* q, int nq, float* val, float* var) {
    if (!g || route < 0 || route > 4 || nq < 0) return GPIS_ERR_ARG;
    if (nq > 0 && ((route != 4 && !q) || (route != 3 && (!val || !var)))) return GPIS_ERR_ARG;
    ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device);
    if (route == 0) return h->g.query(q, nq, val, var, h->s);
    if (!h->g.trained()) return GPIS_ERR_STATE;
    const size_t per = (h->g.mode() == 2) ? 2 : 1;
    if (route == 1) {
        if (nq == 0) return GPIS_OK;
        float* sq = h->g.stage_q(nq);
        if (!sq) return GPIS_ERR_HIP;
        std::memcpy(sq, q, sizeof(float) * per * (size_t)nq);
        const int rc = h->g.query_staged(nq, h->s);
        if (rc) return rc;
        std::memcpy(val, h->g.staged_val(), sizeof(float) * (size_t)nq);
        std::memcpy(var, h->g.staged_var(), sizeof(float) * (size_t)nq);
        return GPIS_OK;
    }
    if (route == 2 || route == 3) {
        if (nq > 0) {
            if (!h->sb && hipStreamCreateWithFlags(&h->sb, hipStreamNonBlocking) != hipSuccess) { h->sb = nullptr; return GPIS_ERR_HIP; }
            float* sq = h->g.stage_qb(nq);
            if (!sq) return GPIS_ERR_HIP;
            std::memcpy(sq, q, sizeof(float) * per * (size_t)nq);
            h->nb = -1;                       // (stage_qb collected whatever was pending: its answers are gone)
            const int rc = h->g.query_staged_b_async(nq, h->sb);
            if (rc) return rc;
        }
        if (route == 3) { if (nq > 0) h->nb = nq; return GPIS_OK; }
    } else {                                  // route 4: exactly the batch that route 3 left behind
        if (h->nb < 0) return GPIS_ERR_STATE;
        if (nq != h->nb) return GPIS_ERR_ARG;
        h->nb = -1;
    }
    const int rc = h->g.wait_b();
    if (rc) return rc;
    if (nq > 0) {
        if (!h->g.staged_val_b() || !h->g.staged_var_b()) return GPIS_ERR_STATE;
        std::memcpy(val, h->g.staged_val_b(), sizeof(float) * (size_t)nq);
        std::memcpy(var, h->g.staged_var_b(), sizeof(float) * (size_t)nq);
    }
    return GPIS_OK;
}
// 1 while a batch of the second staging set has been issued and not yet waited for (by route 4, by the next route 2 / 3, or by a
// training call, which waits before it rewrites the groups the batch reads), else 0
int gpis_obsgp_pending(void* g) { if (!g) return GPIS_ERR_ARG; return ((ObsHandle*)g)->g.pending_b() ? 1 : 0; }
int gpis_obsgp_num_groups(void* g) { if (!g) return GPIS_ERR_ARG; return ((ObsHandle*)g)->g.ngroups(); }
int gpis_obsgp_get_group(void* g, int group, int* n, float* x, float* alpha, float* L) {
    if (!g || !n) return GPIS_ERR_ARG; ObsHandle* h = (ObsHandle*)g; DeviceScope dev_scope_(h->device); return h->g.get_group(group, n, x, alpha, L, h->s);
}

// ---- OnGPIS -------------------------------------------------------------------
struct OnHandle {
    int device = -1;     // the device current at creation: every entry makes it current for its duration
    OnGPISStore st; hipStream_t s = nullptr;
    float* d_xq = nullptr; float* d_out = nullptr; size_t cap_xq = 0, cap_out = 0;
    OnHandle(int dim, float scale) : st(dim, scale) {}
};
void* gpis_ongpis_create(int dim, float scale) {
    if (dim != 2 && dim != 3) return nullptr;
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    OnHandle* h = new (std::nothrow) OnHandle(dim, scale);
    if (h) (void)hipGetDevice(&h->device);
    if (h && hipStreamCreate(&h->s) != hipSuccess) { delete h; return nullptr; }
    if (h) h->st.profile = true;
    return h;
}
void gpis_ongpis_destroy(void* s) {
    if (!s) return; OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    (void)hipFree(h->d_xq); (void)hipFree(h->d_out);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
}
int gpis_ongpis_train(void* s, const float* soa9, int npts, const int* off, const int* ids, int ncl, int* model_out) {
    if (!s || !soa9 || !off || !ids || ncl < 0) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    int dim = h->st.dim();
    int rc = h->st.upload_points(soa9, npts, h->s);
    if (rc) return rc;
    std::vector<TrainJob> jobs;
    std::vector<int> idv(ids, ids + off[ncl]);
    for (int c = 0; c < ncl; ++c) {
        TrainJob j; j.model = h->st.new_slot(); j.off = off[c]; j.n = off[c + 1] - off[c]; j.ng = 0;
        for (int k = j.off; k < j.off + j.n; ++k) {
            int id = ids[k];
            if (id < 0 || id >= npts) return GPIS_ERR_ARG;
            bool tiny = true;
            for (int d = 0; d < dim; ++d) tiny = tiny && ((double)fabsf(soa9[(size_t)(3 + d) * npts + id]) < 1e-6);
            if (!(((double)soa9[(size_t)8 * npts + id] > 0.1001) || tiny)) ++j.ng;
        }
        if (model_out) model_out[c] = j.model;
        jobs.push_back(j);
    }
    return h->st.train_batch(jobs, idv, h->s);
}
int gpis_ongpis_model_dims(void* s, int model, int* d4) {
    if (!s || !d4) return GPIS_ERR_ARG;
    const ClusterModel* m = ((OnHandle*)s)->st.model(model);
    if (!m || !m->base) return GPIS_ERR_ARG;
    d4[0] = m->N; d4[1] = m->ng; d4[2] = m->K; d4[3] = m->ld;
    return GPIS_OK;
}
int gpis_ongpis_get_model(void* s, int model, float* L, float* alpha, int* gidx) {
    if (!s) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    const ClusterModel* m = h->st.model(model);
    if (!m || !m->base) return GPIS_ERR_ARG;
    if (!m->L) return GPIS_ERR_STATE;   // imported (predict-only) model: no factor on this rank
    if (L) GPIS_HIP(hipMemcpyAsync(L, m->L, sizeof(float) * (size_t)m->ld * m->ld, hipMemcpyDeviceToHost, h->s));
    if (alpha) GPIS_HIP(hipMemcpyAsync(alpha, m->alpha, sizeof(float) * m->K, hipMemcpyDeviceToHost, h->s));
    if (gidx) GPIS_HIP(hipMemcpyAsync(gidx, m->gidx, sizeof(int) * m->N, hipMemcpyDeviceToHost, h->s));
    GPIS_HIP(hipStreamSynchronize(h->s));
    return GPIS_OK;
}
int gpis_ongpis_eval(void* s, const float* xq, int nq, const int* job_q, const int* job_model, int njobs, float* out8) {
    return gpis_ongpis_eval_layout(s, xq, nq, job_q, job_model, njobs, 0, out8);
}
int gpis_ongpis_eval_layout(void* s, const float* xq, int nq, const int* job_q, const int* job_model, int njobs, int layout, float* out8) {
    if (!s || !xq || !job_q || !job_model || !out8 || nq < 1 || njobs < 1 || layout < 0 || layout >= ONGPIS_NLAYOUT) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    int dim = h->st.dim();
    std::vector<float> x4((size_t)4 * nq, 0.f);
    for (int i = 0; i < nq; ++i) for (int d = 0; d < dim; ++d) x4[(size_t)4 * i + d] = xq[(size_t)dim * i + d];
    if (x4.size() > h->cap_xq) { (void)hipFree(h->d_xq); h->d_xq = nullptr; GPIS_HIP(hipMalloc(&h->d_xq, sizeof(float) * x4.size())); h->cap_xq = x4.size(); }
    size_t no = (size_t)8 * njobs;
    if (no > h->cap_out) { (void)hipFree(h->d_out); h->d_out = nullptr; GPIS_HIP(hipMalloc(&h->d_out, sizeof(float) * no)); h->cap_out = no; }
    GPIS_HIP(hipMemcpyAsync(h->d_xq, x4.data(), sizeof(float) * x4.size(), hipMemcpyHostToDevice, h->s));
    GPIS_HIP(hipMemsetAsync(h->d_out, 0, sizeof(float) * no, h->s));
    int rc = h->st.eval_jobs(h->d_xq, job_q, job_model, njobs, h->d_out, h->s, layout);
    if (rc && rc != GPIS_ERR_STATE) return rc;
    // (GPIS_ERR_STATE = the kernels' error word: the results still travel -- the affected ones are NaN -- and the call fails)
    GPIS_HIP(hipMemcpyAsync(out8, h->d_out, sizeof(float) * no, hipMemcpyDeviceToHost, h->s));
    GPIS_HIP(hipStreamSynchronize(h->s));
    return rc;
}
long long gpis_ongpis_packed_bytes(void* s, const int* models, int n) {
    if (!s || (!models && n > 0) || n < 0) return GPIS_ERR_ARG;
    return (long long)((OnHandle*)s)->st.packed_bytes(models, n);
}
int gpis_ongpis_pack(void* s, const int* models, int n, void* d_buf, long long stride, void* stream) {
    if (!s || !models || !d_buf || n < 0 || stride < 256 || stride % 256 != 0) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    return h->st.pack_models(models, n, d_buf, (size_t)stride, stream ? (hipStream_t)stream : h->s);
}
int gpis_ongpis_unpack(void* s, const void* d_buf, int n, long long stride, int* models_inout, void* stream) {
    if (!s || !d_buf || !models_inout || n < 0 || stride < 256 || stride % 256 != 0) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    return h->st.unpack_models(d_buf, n, (size_t)stride, models_inout, stream ? (hipStream_t)stream : h->s);
}
int gpis_ongpis_set_exp_table(void* s, int on) {
    if (!s) return GPIS_ERR_ARG;
    ((OnHandle*)s)->st.use_exp_table = on != 0;
    return GPIS_OK;
}
int gpis_ongpis_kernel_matrix(void* s, const float* x, const int* gidx, const float* sigx, const float* sigg, int n, float* K_out) {
    if (!s) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    return h->st.kernel_matrix(x, gidx, sigx, sigg, n, K_out, h->s);
}
int gpis_ongpis_set_keep_factor(void* s, int on) {
    if (!s) return GPIS_ERR_ARG;
    ((OnHandle*)s)->st.keep_factor = on != 0;
    return GPIS_OK;
}
int gpis_ongpis_set_fused(void* s, int on) {
    if (!s) return GPIS_ERR_ARG;
    ((OnHandle*)s)->st.use_fused = on != 0;
    return GPIS_OK;
}
int gpis_ongpis_set_lazy_inverse(void* s, int on) {
    if (!s) return GPIS_ERR_ARG;
    ((OnHandle*)s)->st.lazy_inverse = on != 0;
    return GPIS_OK;
}
int gpis_ongpis_set_debug(void* s, int inject, int wait_limit_ms) {
    if (!s || wait_limit_ms < 0 || wait_limit_ms > 20000) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    h->st.debug_inject = inject;
    h->st.wait_limit_ticks = wait_limit_ms * 100000;     // 100 MHz device clock
    return GPIS_OK;
}
int gpis_ongpis_set_cu_reserve(void* s, int n) {
    if (!s || n < 0) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    const int rc = h->st.set_cu_reserve(n);      // (joins a batch in flight, re-creates the side streams at the next training)
    if (rc != GPIS_OK) return rc;
    // the handle's own stream carries the largest clusters (the cooperative launch): masked like the others
    hipStream_t ns = nullptr;
    if (int src = ongpis_make_train_stream(&ns, n)) return src;
    if (h->s) { (void)hipStreamSynchronize(h->s); (void)hipStreamDestroy(h->s); }
    h->s = ns;
    return GPIS_OK;
}
int gpis_ongpis_last_ms(void* s, float* t, float* e) {
    if (!s) return GPIS_ERR_ARG;
    OnHandle* h = (OnHandle*)s;
    DeviceScope dev_scope_(h->device);
    if (t) *t = h->st.last_train_ms;
    if (e) *e = h->st.last_eval_ms;
    return GPIS_OK;
}

// ---- K5 probe: a MapQuery over an OnGPIS handle's store and a caller-given cluster table --------------------------
struct MqHandle {
    OnHandle* on;
    MapQuery mq;
    float* d_x = nullptr; float* d_res = nullptr; size_t cap_x = 0, cap_res = 0;
    int last_n = -1;     // queries of the last run when its candidates can be read back (one chunk, a table), else -1
    MqHandle(OnHandle* o, float half, float thre, float prior) : on(o), mq(o->st.dim(), half, thre, prior) {}
};
void* gpis_mapquery_create(void* ongpis, float search_half, float var_thre, float prior_var) {
    if (!ongpis || !(search_half > 0.f) || !std::isfinite(search_half) || std::isnan(var_thre) || std::isnan(prior_var)) return nullptr;
    OnHandle* o = (OnHandle*)ongpis;
    DeviceScope dev_scope_(o->device);
    return new (std::nothrow) MqHandle(o, search_half, var_thre, prior_var);
}
void gpis_mapquery_destroy(void* h) {
    if (!h) return; MqHandle* q = (MqHandle*)h;
    DeviceScope dev_scope_(q->on->device);
    (void)hipStreamSynchronize(q->on->s);
    (void)hipFree(q->d_x); (void)hipFree(q->d_res);
    delete q;
}
int gpis_mapquery_set_table(void* h, int ncl, const float* c, const float* lo, const float* hi, const int* model, const int* parent,
                            int nanc, const float* anc_lo, const float* anc_hi, const int* anc_parent, double pitch) {
    if (!h || ncl < 0 || nanc < 0 || !(pitch > 0.0) || !std::isfinite(pitch)) return GPIS_ERR_ARG;
    if (ncl > 0 && (!c || !lo || !hi || !model || !parent)) return GPIS_ERR_ARG;
    if (nanc > 0 && (!anc_lo || !anc_hi || !anc_parent)) return GPIS_ERR_ARG;
    MqHandle* q = (MqHandle*)h;
    // everything a kernel would index with is checked here: a model must be a trained slot of the store or -1, a parent an
    // ancestor or -1, an ancestor's parent an earlier ancestor or -1 (so that every chain ends)
    for (int a = 0; a < nanc; ++a) if (anc_parent[a] < -1 || anc_parent[a] >= a) return GPIS_ERR_ARG;
    for (int i = 0; i < ncl; ++i) {
        if (parent[i] < -1 || parent[i] >= nanc) return GPIS_ERR_ARG;
        if (model[i] < -1) return GPIS_ERR_ARG;
        if (model[i] >= 0) { const ClusterModel* m = q->on->st.model(model[i]); if (!m || !m->base) return GPIS_ERR_ARG; }
        for (int d = 0; d < 3; ++d) if (!std::isfinite(c[3 * i + d])) return GPIS_ERR_ARG;
    }
    DeviceScope dev_scope_(q->on->device);
    try {
        std::vector<ClusterEntry> ent((size_t)ncl);
        std::vector<AncestorEntry> anc((size_t)nanc);
        for (int i = 0; i < ncl; ++i) {
            for (int d = 0; d < 3; ++d) { ent[i].c[d] = c[3 * i + d]; ent[i].lo[d] = lo[3 * i + d]; ent[i].hi[d] = hi[3 * i + d]; }
            ent[i].model = model[i]; ent[i].parent = parent[i];
        }
        for (int a = 0; a < nanc; ++a) {
            for (int d = 0; d < 3; ++d) { anc[a].lo[d] = anc_lo[3 * a + d]; anc[a].hi[d] = anc_hi[3 * a + d]; }
            anc[a].parent = anc_parent[a];
        }
        q->last_n = -1;
        (void)hipStreamSynchronize(q->on->s);
        return q->mq.set_clusters(ent, anc, pitch, q->on->s);
    } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_mapquery_set_chunk(void* h, int n) {
    if (!h || n < 0) return GPIS_ERR_ARG;
    ((MqHandle*)h)->mq.chunk = n;   // (0: automatic)
    return GPIS_OK;
}
int gpis_mapquery_run(void* h, const float* x, int n, float* res_inout) {
    if (!h || n < 0 || (n > 0 && (!x || !res_inout))) return GPIS_ERR_ARG;
    MqHandle* q = (MqHandle*)h;
    DeviceScope dev_scope_(q->on->device);
    q->last_n = -1;
    const int dim = q->on->st.dim();
    const size_t nx = (size_t)dim * n, nr = (size_t)2 * (1 + dim) * n;
    if (nx > q->cap_x) { (void)hipFree(q->d_x); q->d_x = nullptr; q->cap_x = 0; GPIS_HIP(hipMalloc(&q->d_x, sizeof(float) * nx)); q->cap_x = nx; }
    if (nr > q->cap_res) { (void)hipFree(q->d_res); q->d_res = nullptr; q->cap_res = 0; GPIS_HIP(hipMalloc(&q->d_res, sizeof(float) * nr)); q->cap_res = nr; }
    hipStream_t s = q->on->s;
    if (n > 0) {
        GPIS_HIP(hipMemcpyAsync(q->d_x, x, sizeof(float) * nx, hipMemcpyHostToDevice, s));
        GPIS_HIP(hipMemcpyAsync(q->d_res, res_inout, sizeof(float) * nr, hipMemcpyHostToDevice, s));
    }
    int rc;
    try { rc = q->mq.run(q->on->st, q->d_x, n, q->d_res, s); } catch (...) { return GPIS_ERR_STATE; }
    // (GPIS_ERR_STATE is the kernels' error word -- the affected results are NaN -- or a tile list that outgrew its array: res is
    // delivered for inspection as gpis_ongpis_eval_layout does, and the call still fails; any other error returns at once)
    if (rc && rc != GPIS_ERR_STATE) return rc;
    if (n > 0) GPIS_HIP(hipMemcpyAsync(res_inout, q->d_res, sizeof(float) * nr, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    if (rc == GPIS_OK && n > 0 && n <= q->mq.last_chunk_len && q->mq.num_clusters() > 0) q->last_n = n;
    return rc;
}
int gpis_mapquery_run_device(void* h, const float* d_x, int n, float* d_res_inout, void* hip_stream) {
    if (!h || n < 0 || (n > 0 && (!d_x || !d_res_inout))) return GPIS_ERR_ARG;
    MqHandle* q = (MqHandle*)h;
    DeviceScope dev_scope_(q->on->device);
    q->last_n = -1;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : q->on->s;
    int rc;
    try { rc = q->mq.run(q->on->st, d_x, n, d_res_inout, s); } catch (...) { return GPIS_ERR_STATE; }
    if (rc && rc != GPIS_ERR_STATE) return rc;
    GPIS_HIP(hipStreamSynchronize(s));
    if (rc == GPIS_OK && n > 0 && n <= q->mq.last_chunk_len && q->mq.num_clusters() > 0) q->last_n = n;
    return rc;
}
int gpis_mapquery_candidates(void* h, int* ncand, int* cand3) {
    if (!h || !ncand || !cand3) return GPIS_ERR_ARG;
    MqHandle* q = (MqHandle*)h;
    if (q->last_n < 0) return GPIS_ERR_STATE;
    DeviceScope dev_scope_(q->on->device);
    const int* d_nc; const int* d_c; int cap;
    q->mq.last_candidates(&d_nc, &d_c, &cap);
    const int n = q->last_n;
    if (!d_nc || !d_c || cap < n) return GPIS_ERR_STATE;
    hipStream_t s = q->on->s;
    GPIS_HIP(hipMemcpyAsync(ncand, d_nc, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    for (int k = 0; k < 3; ++k)
        GPIS_HIP(hipMemcpyAsync(cand3 + (size_t)k * n, d_c + (size_t)k * cap, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}
int gpis_mapquery_pass_jobs(void* h, long long* out4) {
    if (!h || !out4) return GPIS_ERR_ARG;
    for (int k = 0; k < 4; ++k) out4[k] = ((MqHandle*)h)->mq.last_pass_jobs[k];
    return GPIS_OK;
}
int gpis_mapquery_pass_detail(void* h, double* out8) {
    if (!h || !out8) return GPIS_ERR_ARG;
    ((MqHandle*)h)->mq.pass_detail(out8);
    return GPIS_OK;
}
int gpis_mapquery_set_k4_schedule(void* h, int mode) {
    if (!h || mode < 0 || mode > 1) return GPIS_ERR_ARG;
    ((MqHandle*)h)->mq.k4_schedule = mode;
    return GPIS_OK;
}
int gpis_mapquery_last_counts(void* h, long long* out4) {
    if (!h || !out4) return GPIS_ERR_ARG;
    const MapQuery& mq = ((MqHandle*)h)->mq;
    out4[0] = mq.last_evals; out4[1] = mq.last_launches; out4[2] = mq.last_chunk_len; out4[3] = mq.k4_schedule;
    return GPIS_OK;
}
int gpis_mapquery_set_pass2_mode(void* h, int mode) {
    if (!h || mode < 0 || mode > 4) return GPIS_ERR_ARG;
    ((MqHandle*)h)->mq.pass2_mode = mode;
    return GPIS_OK;
}

// ---- surface extraction ---------------------------------------------------------------------------------------
void* gpis_mesh_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    MeshExtractor* me = new (std::nothrow) MeshExtractor();
    if (me && !me->own) { delete me; return nullptr; }
    return me;
}
void gpis_mesh_destroy(void* mesh) { delete (MeshExtractor*)mesh; }
int gpis_mesh_set_chunk(void* mesh, int points) {
    if (!mesh || points < 0) return GPIS_ERR_ARG;
    ((MeshExtractor*)mesh)->chunk = points ? points : (1 << 22);
    return GPIS_OK;
}
// (the result is dropped only once the arguments passed: an argument error leaves the previous one readable)
static int mesh_args(void* mesh, int dim, const int* n, const float* origin, const float* step) {
    if (!mesh) return GPIS_ERR_ARG;
    long long np = 0;
    return mesh_check_lattice(dim, n, origin, step, &np);
}
int gpis_mesh_from_grid(void* mesh, const float* d_val, int dim, const int* n, const float* origin, const float* step, float level,
                        void* stream) {
    if (int rc = mesh_args(mesh, dim, n, origin, step)) return rc;
    if (!d_val || !std::isfinite(level)) return GPIS_ERR_ARG;
    MeshExtractor& me = *(MeshExtractor*)mesh;
    DeviceScope ds(me.device);
    me.clear_result();
    try {
        const int rc = me.from_grid(d_val, dim, n, origin, step, level, stream ? (hipStream_t)stream : me.own);
        if (rc != GPIS_OK) me.clear_result();
        return rc;
    } catch (...) { me.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_extract_mesh(void* m, void* mesh, const int* n3, const float* origin3, const float* step3, float level, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    if (int rc = mesh_args(mesh, 3, n3, origin3, step3)) return rc;
    if (std::isinf(level)) return GPIS_ERR_ARG;
    MeshExtractor& me = *(MeshExtractor*)mesh;
    me.clear_result();
    const int rc = gpis3_impl_extract((GPisMap3*)m, me, n3, origin3, step3, level, stream);
    if (rc != GPIS_OK) me.clear_result();
    return rc;
}
int gpis2_extract_contour(void* m, void* mesh, const int* n2, const float* origin2, const float* step2, float level, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    if (int rc = mesh_args(mesh, 2, n2, origin2, step2)) return rc;
    if (std::isinf(level)) return GPIS_ERR_ARG;
    MeshExtractor& me = *(MeshExtractor*)mesh;
    me.clear_result();
    const int rc = gpis2_impl_extract((GPisMap*)m, me, n2, origin2, step2, level, stream);
    if (rc != GPIS_OK) me.clear_result();
    return rc;
}
int gpis_mesh_counts(void* mesh, long long* nvert, long long* nprim) {
    if (!mesh) return GPIS_ERR_ARG;
    const MeshExtractor& me = *(MeshExtractor*)mesh;
    if (nvert) *nvert = me.nvert;
    if (nprim) *nprim = me.nprim;
    return GPIS_OK;
}
int gpis_mesh_get(void* mesh, float* verts, int* prims, float* vrec) {
    if (!mesh) return GPIS_ERR_ARG;
    MeshExtractor& me = *(MeshExtractor*)mesh;
    if (vrec && me.nvert > 0 && !me.rec_valid) return GPIS_ERR_STATE;
    DeviceScope ds(me.device);
    const size_t d = (size_t)me.dim;
    if (verts && me.nvert > 0) GPIS_HIP(hipMemcpyAsync(verts, me.d_verts, sizeof(float) * d * me.nvert, hipMemcpyDeviceToHost, me.own));
    if (prims && me.nprim > 0) GPIS_HIP(hipMemcpyAsync(prims, me.d_prims, sizeof(int) * d * me.nprim, hipMemcpyDeviceToHost, me.own));
    if (vrec && me.nvert > 0) GPIS_HIP(hipMemcpyAsync(vrec, me.d_vrec, sizeof(float) * 2 * (1 + d) * me.nvert, hipMemcpyDeviceToHost, me.own));
    GPIS_HIP(hipStreamSynchronize(me.own));
    return GPIS_OK;
}
int gpis_mesh_get_grid(void* mesh, float* vals) {
    if (!mesh || !vals) return GPIS_ERR_ARG;
    MeshExtractor& me = *(MeshExtractor*)mesh;
    if (!me.grid_valid) return GPIS_ERR_STATE;
    DeviceScope ds(me.device);
    GPIS_HIP(hipMemcpyAsync(vals, me.d_val, sizeof(float) * me.ngrid, hipMemcpyDeviceToHost, me.own));
    GPIS_HIP(hipStreamSynchronize(me.own));
    return GPIS_OK;
}
int gpis_mesh_device(void* mesh, const float** d_verts, const int** d_prims, const float** d_vrec) {
    if (!mesh) return GPIS_ERR_ARG;
    const MeshExtractor& me = *(MeshExtractor*)mesh;
    if (d_verts) *d_verts = me.d_verts;
    if (d_prims) *d_prims = me.d_prims;
    if (d_vrec) *d_vrec = me.rec_valid ? me.d_vrec : nullptr;
    return GPIS_OK;
}

// ---- distance field ---------------------------------------------------------------------------------------------------
void* gpis_dfield_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    DistanceField* df = new (std::nothrow) DistanceField();
    if (df && !df->own) { delete df; return nullptr; }
    return df;
}
void gpis_dfield_destroy(void* df) { delete (DistanceField*)df; }
int gpis_dfield_set_chunk(void* df, int points) {
    if (!df || points < 0) return GPIS_ERR_ARG;
    ((DistanceField*)df)->chunk = points ? points : (1 << 22);
    return GPIS_OK;
}
// (the result is dropped only once the arguments passed: an argument error leaves the previous one readable)
static int dfield_args(void* df, int dim, const int* n, const float* origin, const float* step) {
    if (!df) return GPIS_ERR_ARG;
    long long np = 0;
    return dfield_check_lattice(dim, n, origin, step, &np);
}
int gpis_dfield_from_grid(void* d, const float* d_val, int dim, const int* n, const float* origin, const float* step, float level,
                          void* stream) {
    if (int rc = dfield_args(d, dim, n, origin, step)) return rc;
    if (!d_val || !std::isfinite(level)) return GPIS_ERR_ARG;
    DistanceField& df = *(DistanceField*)d;
    DeviceScope ds(df.device);
    df.clear_result();
    try {
        const int rc = df.from_grid(d_val, dim, n, origin, step, level, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) df.clear_result();
        return rc;
    } catch (...) { df.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_distance_field(void* m, void* d, const int* n3, const float* origin3, const float* step3, float level, float max_var,
                         void* stream) {
    if (!m) return GPIS_ERR_ARG;
    if (int rc = dfield_args(d, 3, n3, origin3, step3)) return rc;
    if (std::isinf(level) || std::isnan(max_var)) return GPIS_ERR_ARG;
    DistanceField& df = *(DistanceField*)d;
    df.clear_result();
    const int rc = gpis3_impl_dfield((GPisMap3*)m, df, n3, origin3, step3, level, max_var, stream);
    if (rc != GPIS_OK) df.clear_result();
    return rc;
}
int gpis2_distance_field(void* m, void* d, const int* n2, const float* origin2, const float* step2, float level, float max_var,
                         void* stream) {
    if (!m) return GPIS_ERR_ARG;
    if (int rc = dfield_args(d, 2, n2, origin2, step2)) return rc;
    if (std::isinf(level) || std::isnan(max_var)) return GPIS_ERR_ARG;
    DistanceField& df = *(DistanceField*)d;
    df.clear_result();
    const int rc = gpis2_impl_dfield((GPisMap*)m, df, n2, origin2, step2, level, max_var, stream);
    if (rc != GPIS_OK) df.clear_result();
    return rc;
}
int gpis_dfield_info(void* d, int* dim, int* n3, float* origin3, float* step) {
    if (!d) return GPIS_ERR_ARG;
    const DistanceField& df = *(DistanceField*)d;
    if (dim) *dim = df.valid ? df.dim : 0;
    for (int a = 0; a < 3; ++a) {
        if (n3) n3[a] = df.valid ? df.n[a] : 0;
        if (origin3) origin3[a] = df.valid ? df.origin[a] : 0.f;
    }
    if (step) *step = df.valid ? df.step : 0.f;
    return GPIS_OK;
}
int gpis_dfield_get(void* d, float* dist, int* site, float* f) {
    if (!d) return GPIS_ERR_ARG;
    DistanceField& df = *(DistanceField*)d;
    if ((dist || site || f) && !df.valid) return GPIS_ERR_STATE;
    if (f && !df.f_valid) return GPIS_ERR_STATE;
    DeviceScope ds(df.device);
    const size_t n = (size_t)df.ngrid;
    if (dist) GPIS_HIP(hipMemcpyAsync(dist, df.d_dist, sizeof(float) * n, hipMemcpyDeviceToHost, df.own));
    if (site) GPIS_HIP(hipMemcpyAsync(site, df.d_site(), sizeof(int) * n, hipMemcpyDeviceToHost, df.own));
    if (f) GPIS_HIP(hipMemcpyAsync(f, df.d_val, sizeof(float) * n, hipMemcpyDeviceToHost, df.own));
    GPIS_HIP(hipStreamSynchronize(df.own));
    return GPIS_OK;
}
int gpis_dfield_device(void* d, const float** d_dist, const int** d_site, const float** d_f) {
    if (!d) return GPIS_ERR_ARG;
    const DistanceField& df = *(DistanceField*)d;
    if (d_dist) *d_dist = df.valid ? df.d_dist : nullptr;
    if (d_site) *d_site = df.d_site();
    if (d_f) *d_f = df.f_valid ? df.d_val : nullptr;
    return GPIS_OK;
}
int gpis_dfield_sample(void* d, const float* d_x, long long m, float* d_out, void* stream) {
    if (!d || m < 0 || (m > 0 && (!d_x || !d_out))) return GPIS_ERR_ARG;
    DistanceField& df = *(DistanceField*)d;
    DeviceScope ds(df.device);
    try {
        return df.sample(d_x, m, d_out, stream ? (hipStream_t)stream : df.own);
    } catch (...) { return GPIS_ERR_STATE; }
}

// ---- planning through a distance field ---------------------------------------------------------------------------------------
int gpis_plan_default_opts(int dim, float step, gpis_plan_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->clearance = 0.f; o->margin = 4.f * step; o->gain = 4.f; o->connectivity = 1; o->max_rounds = 0;
    return GPIS_OK;
}
void* gpis_plan_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Planner* p = new (std::nothrow) Planner();
    if (p && !p->own) { delete p; return nullptr; }
    return p;
}
void gpis_plan_destroy(void* plan) { delete (Planner*)plan; }
int gpis_plan_set_schedule(void* plan, int check_every, int inner_cap) {
    if (!plan || check_every < 0 || inner_cap < 0) return GPIS_ERR_ARG;
    ((Planner*)plan)->sched.set(check_every, inner_cap);
    return GPIS_OK;
}
// the argument and state checks come before anything is dropped: such an error leaves the previous result readable
int gpis_plan_solve(void* plan, void* d, const float* goals, int ngoals, const gpis_plan_opts* opts, void* stream) {
    if (!plan || !d || !goals || ngoals < 1) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    gpis_plan_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_plan_default_opts(df.dim, df.step, &dflt);
        opts = &dflt;
    }
    PlanOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.gain = opts->gain; o.connectivity = opts->connectivity;
    o.max_rounds = opts->max_rounds;
    if (int rc = plan_check_opts(o)) return rc;
    if (!df.valid) return GPIS_ERR_STATE;
    Planner& p = *(Planner*)plan;
    DeviceScope ds(df.device);
    try {
        if (int rc = p.bind(df.device)) { p.clear_result(); return rc; }
        const int rc = p.solve(df, goals, ngoals, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) p.clear_result();
        return rc;
    } catch (...) { p.clear_result(); return GPIS_ERR_STATE; }
}
int gpis_plan_info(void* plan, double* out, int n) {
    if (!plan || !out || n < 0) return GPIS_ERR_ARG;
    const Planner& p = *(Planner*)plan;
    const bool v = p.valid;
    const PlanCounters& c = p.cnt;
    const double w[14] = {v ? 1.0 : 0.0, v ? (double)p.dim : 0.0, v ? (double)p.n[0] : 0.0, v ? (double)p.n[1] : 0.0,
                          v ? (double)p.n[2] : 0.0, v ? (double)p.step : 0.0, (double)c.goals_given, (double)c.goals_kept,
                          (double)c.nfree, (double)c.nreach, (double)c.rounds, (double)c.launches, c.solve_ms, (double)c.max_cost};
    for (int i = 0; i < n && i < 14; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_plan_get(void* plan, float* cost, unsigned char* policy) {
    if (!plan) return GPIS_ERR_ARG;
    Planner& p = *(Planner*)plan;
    if (!p.valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t n = (size_t)p.ngrid;
    if (cost) GPIS_HIP(hipMemcpyAsync(cost, p.d_cost, sizeof(float) * n, hipMemcpyDeviceToHost, p.own));
    if (policy) GPIS_HIP(hipMemcpyAsync(policy, p.d_policy, n, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    return GPIS_OK;
}
int gpis_plan_device(void* plan, const float** d_cost, const unsigned char** d_policy) {
    if (!plan) return GPIS_ERR_ARG;
    const Planner& p = *(Planner*)plan;
    if (d_cost) *d_cost = p.valid ? p.d_cost : nullptr;
    if (d_policy) *d_policy = p.valid ? p.d_policy : nullptr;
    return GPIS_OK;
}
int gpis_plan_paths(void* plan, const float* starts, int m, int max_points, void* stream) {
    if (!plan || !starts || m < 1 || max_points < 2) return GPIS_ERR_ARG;
    Planner& p = *(Planner*)plan;
    if (!p.valid) return GPIS_ERR_STATE;
    if (m > Planner::kMaxStarts) return GPIS_ERR_LIMIT;
    DeviceScope ds(p.device);
    try {
        const int rc = p.paths(starts, m, max_points, stream ? (hipStream_t)stream : p.own);
        if (rc != GPIS_OK) p.paths_valid = false;
        return rc;
    } catch (...) { p.paths_valid = false; return GPIS_ERR_STATE; }
}
int gpis_plan_path_counts(void* plan, long long* npaths, long long* npoints) {
    if (!plan) return GPIS_ERR_ARG;
    const Planner& p = *(Planner*)plan;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (npaths) *npaths = p.npaths;
    if (npoints) *npoints = p.npoints;
    return GPIS_OK;
}
int gpis_plan_get_paths(void* plan, long long* off, float* points, float* start_cost, unsigned char* status) {
    if (!plan) return GPIS_ERR_ARG;
    Planner& p = *(Planner*)plan;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t m = (size_t)p.npaths;
    if (off) GPIS_HIP(hipMemcpyAsync(off, p.d_off, sizeof(long long) * (m + 1), hipMemcpyDeviceToHost, p.own));
    if (points && p.npoints > 0)
        GPIS_HIP(hipMemcpyAsync(points, p.d_points, sizeof(float) * (size_t)p.npoints * p.dim, hipMemcpyDeviceToHost, p.own));
    if (start_cost) GPIS_HIP(hipMemcpyAsync(start_cost, p.d_scost, sizeof(float) * m, hipMemcpyDeviceToHost, p.own));
    if (status) GPIS_HIP(hipMemcpyAsync(status, p.d_status, m, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    return GPIS_OK;
}

// ---- trajectories through a distance field -----------------------------------------------------------------------------------
int gpis_traj_default_opts(int dim, float step, gpis_traj_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->clearance = 0.f; o->margin = 3.f * step; o->w_smooth = 1.f; o->w_obs = 0.25f * step; o->rate = 0.02f;
    o->max_move = 0.5f * step; o->tol = 0.01f * step; o->iters = 100; o->sub = 3;
    return GPIS_OK;
}
void* gpis_traj_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Trajectories* t = new (std::nothrow) Trajectories();
    if (t && !t->own) { delete t; return nullptr; }
    return t;
}
void gpis_traj_destroy(void* traj) { delete (Trajectories*)traj; }
// Trajectories::from_paths and ::set check their arguments and the planner's state before they drop anything, so such an error
// leaves the previous input and result readable; a failure after that leaves the handle without input.
int gpis_traj_from_paths(void* traj, void* plan, int N) {
    if (!traj || !plan) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const Planner& p = *(const Planner*)plan;
    DeviceScope ds(p.device);
    try { return t.from_paths(p, N); } catch (...) { t.has_input = t.valid = false; return GPIS_ERR_STATE; }
}
int gpis_traj_set(void* traj, const float* x, int m, int N, int dim) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.set(x, m, N, dim); } catch (...) { t.has_input = t.valid = false; return GPIS_ERR_STATE; }
}
int gpis_traj_optimize(void* traj, void* d, const gpis_traj_opts* opts, void* stream) {
    if (!traj || !d) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const DistanceField& df = *(const DistanceField*)d;
    gpis_traj_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_traj_default_opts(df.dim, df.step, &dflt);
        opts = &dflt;
    }
    TrajOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.w_smooth = opts->w_smooth; o.w_obs = opts->w_obs; o.rate = opts->rate;
    o.max_move = opts->max_move; o.tol = opts->tol; o.iters = opts->iters; o.sub = opts->sub;
    DeviceScope ds(df.device);
    try { return t.optimize(df, o, stream ? (hipStream_t)stream : df.own); } catch (...) { t.valid = false; return GPIS_ERR_STATE; }
}
int gpis_traj_info(void* traj, double* out, int n) {
    if (!traj || !out || n < 0) return GPIS_ERR_ARG;
    const Trajectories& t = *(const Trajectories*)traj;
    const bool h = t.has_input;
    const double w[6] = {h ? 1.0 : 0.0, t.valid ? 1.0 : 0.0, h ? (double)t.m : 0.0, h ? (double)t.N : 0.0, h ? (double)t.dim : 0.0,
                         t.valid ? t.opt_ms : 0.0};
    for (int i = 0; i < n && i < 6; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_traj_get(void* traj, float* x, unsigned char* status, int* iterations, float* length, float* smooth, float* obstacle,
                  float* min_dist, int* nonfinite, unsigned char* collides) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    if (!t.valid) return GPIS_ERR_STATE;
    DeviceScope ds(t.device);
    const size_t m = (size_t)t.m;
    std::vector<float> fr;
    std::vector<int> ir;
    if (x) GPIS_HIP(hipMemcpyAsync(x, t.d_x, sizeof(float) * m * t.N * t.dim, hipMemcpyDeviceToHost, t.own));
    if (length || smooth || obstacle || min_dist) {
        fr.resize(4 * m);
        GPIS_HIP(hipMemcpyAsync(fr.data(), t.d_fres, sizeof(float) * 4 * m, hipMemcpyDeviceToHost, t.own));
    }
    if (status || iterations || nonfinite || collides) {
        ir.resize(4 * m);
        GPIS_HIP(hipMemcpyAsync(ir.data(), t.d_ires, sizeof(int) * 4 * m, hipMemcpyDeviceToHost, t.own));
    }
    GPIS_HIP(hipStreamSynchronize(t.own));
    for (size_t k = 0; k < m; ++k) {
        if (length) length[k] = fr[4 * k];
        if (smooth) smooth[k] = fr[4 * k + 1];
        if (obstacle) obstacle[k] = fr[4 * k + 2];
        if (min_dist) min_dist[k] = fr[4 * k + 3];
        if (status) status[k] = (unsigned char)ir[4 * k];
        if (iterations) iterations[k] = ir[4 * k + 1];
        if (nonfinite) nonfinite[k] = ir[4 * k + 2];
        if (collides) collides[k] = (unsigned char)ir[4 * k + 3];
    }
    return GPIS_OK;
}
int gpis_traj_device(void* traj, const float** d_x, const float** d_fres, const int** d_ires) {
    if (!traj) return GPIS_ERR_ARG;
    const Trajectories& t = *(const Trajectories*)traj;
    if (d_x) *d_x = t.valid ? t.d_x : nullptr;
    if (d_fres) *d_fres = t.valid ? t.d_fres : nullptr;
    if (d_ires) *d_ires = t.valid ? t.d_ires : nullptr;
    return GPIS_OK;
}

// ---- time parametrisation of trajectories, control sequences, the controller's nominal sequence ------------------------------
int gpis_timing_default_opts(int dim, float step, gpis_traj_timing_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->v_max = 1.f; o->v_min = 0.05f; o->a_max = 0.5f; o->d_max = 0.5f; o->a_lat = 0.5f; o->w_max = 1.f; o->v_start = 0.f;
    o->v_end = 0.f; o->clearance = step; o->slow_dist = 4.f * step;
    return GPIS_OK;
}
// The options and the handles' states are checked before anything is dropped, so such an error leaves the previous timing
// readable; a failure after that leaves the result without a timing.
int gpis_timing_time(void* traj, void* d, const gpis_traj_timing_opts* opts, void* stream) {
    if (!traj || !opts) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    TimingOpts o;
    o.v_max = opts->v_max; o.v_min = opts->v_min; o.a_max = opts->a_max; o.d_max = opts->d_max; o.a_lat = opts->a_lat;
    o.w_max = opts->w_max; o.v_start = opts->v_start; o.v_end = opts->v_end; o.clearance = opts->clearance; o.slow_dist = opts->slow_dist;
    DeviceScope ds(t.device);
    try { return t.time((const DistanceField*)d, o, (hipStream_t)stream); } catch (...) { t.timed = false; return GPIS_ERR_STATE; }
}
int gpis_timing_info(void* traj, double* out, int n) {
    if (!traj || !out || n < 0) return GPIS_ERR_ARG;
    const Trajectories& t = *(const Trajectories*)traj;
    const bool h = t.has_timing();
    const double w[3] = {h ? 1.0 : 0.0, h ? t.time_ms : 0.0, h ? t.controls_ms : 0.0};
    for (int i = 0; i < n && i < 3; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_timing_get(void* traj, float* v, float* t_out, unsigned char* limiter, unsigned char* status, float* duration,
                    float* max_speed, float* max_curvature, int* limiter_counts) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    if (!t.has_timing()) return GPIS_ERR_STATE;
    DeviceScope ds(t.device);
    const size_t m = (size_t)t.m, mn = m * t.N;
    std::vector<float> fr;
    if (v) GPIS_HIP(hipMemcpyAsync(v, t.d_tv, sizeof(float) * mn, hipMemcpyDeviceToHost, t.own));
    if (t_out) GPIS_HIP(hipMemcpyAsync(t_out, t.d_tt, sizeof(float) * mn, hipMemcpyDeviceToHost, t.own));
    if (limiter) GPIS_HIP(hipMemcpyAsync(limiter, t.d_lim, mn, hipMemcpyDeviceToHost, t.own));
    if (duration || max_speed || max_curvature) {
        fr.resize(3 * m);
        GPIS_HIP(hipMemcpyAsync(fr.data(), t.d_tsum, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, t.own));
    }
    GPIS_HIP(hipStreamSynchronize(t.own));
    for (size_t k = 0; k < m; ++k) {
        if (duration) duration[k] = fr[3 * k];
        if (max_speed) max_speed[k] = fr[3 * k + 1];
        if (max_curvature) max_curvature[k] = fr[3 * k + 2];
        if (status) status[k] = (unsigned char)t.h_tint[9 * k];
        if (limiter_counts) for (int c = 0; c < 8; ++c) limiter_counts[8 * k + c] = t.h_tint[9 * k + 1 + c];
    }
    return GPIS_OK;
}
int gpis_timing_controls(void* traj, double dt, int T, double t0, double w_limit, double min_move, double* U, double* heading0,
                         double* p0, int* clamped) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.controls(dt, T, t0, w_limit, min_move, U, heading0, p0, clamped); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_timing_follow(void* mppi, void* traj, int index, double dt, double t0, double w_limit, double min_move, double* heading0,
                       double* p0) {
    if (!mppi || !traj) return GPIS_ERR_ARG;
    Controller& c = *(Controller*)mppi;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.follow(c, index, dt, t0, w_limit, min_move, heading0, p0); } catch (...) { return GPIS_ERR_STATE; }
}

// ---- rendering ---------------------------------------------------------------------------------------------------------
static RenderOpts render_opts(const gpis_render_opts* o) {
    RenderOpts r;
    r.tnear = o->tnear; r.tfar = o->tfar; r.min_step = o->min_step; r.max_step = o->max_step; r.far_step = o->far_step;
    r.level = o->level; r.max_var = o->max_var; r.refine = o->refine; r.max_steps = o->max_steps;
    return r;
}
int gpis_render_default_opts(int dim, gpis_render_opts* o) {
    if (!o || (dim != 2 && dim != 3)) return GPIS_ERR_ARG;
    const float nan = std::nanf("");
    if (dim == 3) { o->tnear = 0.4f; o->tfar = 4.0f; o->min_step = 1e-3f; o->max_step = 0.01f; o->max_steps = 512; }
    else { o->tnear = 0.2f; o->tfar = 30.0f; o->min_step = 0.01f; o->max_step = 0.1f; o->max_steps = 1024; }
    o->far_step = nan; o->level = nan; o->max_var = INFINITY; o->refine = 8;
    return GPIS_OK;
}
void* gpis_render_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Renderer* r = new (std::nothrow) Renderer();
    if (r && !r->own) { delete r; return nullptr; }
    return r;
}
void gpis_render_destroy(void* render) { delete (Renderer*)render; }
int gpis_render_set_chunk(void* render, int rays) {
    if (!render || rays < 0) return GPIS_ERR_ARG;
    ((Renderer*)render)->chunk = rays ? rays : (1 << 22);
    return GPIS_OK;
}
// the checks that need no map: an argument error leaves the previous result readable
static int render_args(void* render, int dim, const float* pose, const gpis_render_opts* opts, RenderOpts* o) {
    if (!render || !pose) return GPIS_ERR_ARG;
    gpis_render_opts d;
    if (!opts) { (void)gpis_render_default_opts(dim, &d); opts = &d; }
    *o = render_opts(opts);
    const int np = dim == 3 ? 12 : 6;
    for (int k = 0; k < np; ++k) if (!std::isfinite(pose[k])) return GPIS_ERR_ARG;
    if (std::isinf(o->level) || (!std::isnan(o->far_step) && !(std::isfinite(o->far_step) && o->far_step > 0.f))) return GPIS_ERR_ARG;
    RenderOpts c = *o;
    c.level = 0.f; c.far_step = 1.f;          // (resolved against the map by the entry)
    return render_check_opts(c);
}
int gpis3_render_depth(void* m, void* render, const gpis_cam* cam, const float* pose12, const gpis_render_opts* opts, void* stream) {
    if (!m) return GPIS_ERR_ARG;
    RenderOpts o;
    if (int rc = render_args(render, 3, pose12, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    Renderer& r = *(Renderer*)render;
    const int rc = gpis3_impl_render((GPisMap3*)m, r, f, pose12, o, stream);
    if (rc != GPIS_OK && rc != GPIS_ERR_ARG && rc != GPIS_ERR_LIMIT) r.clear_result();
    return rc;
}
int gpis2_render_scan(void* m, void* render, const float* thetas, int n, const float* pose6, const gpis_render_opts* opts, void* stream) {
    if (!m || !thetas || n < 1) return GPIS_ERR_ARG;
    RenderOpts o;
    if (int rc = render_args(render, 2, pose6, opts, &o)) return rc;
    Renderer& r = *(Renderer*)render;
    SensorFrame f;
    int rc = scan_frame(m, thetas, n, nullptr, &f);
    if (rc == GPIS_OK) rc = gpis2_impl_render((GPisMap*)m, r, f, pose6, o, stream);
    if (rc != GPIS_OK && rc != GPIS_ERR_ARG && rc != GPIS_ERR_LIMIT) r.clear_result();
    return rc;
}
int gpis_render_get(void* render, float* depth, float* rec, unsigned char* status) {
    if (!render) return GPIS_ERR_ARG;
    Renderer& r = *(Renderer*)render;
    if (!r.valid) return GPIS_ERR_STATE;
    DeviceScope ds(r.device);
    const size_t n = (size_t)r.nrays, nc = (size_t)r.rec_width();
    if (depth) GPIS_HIP(hipMemcpyAsync(depth, r.d_depth, sizeof(float) * n, hipMemcpyDeviceToHost, r.own));
    if (rec) GPIS_HIP(hipMemcpyAsync(rec, r.d_rec, sizeof(float) * nc * n, hipMemcpyDeviceToHost, r.own));
    if (status) GPIS_HIP(hipMemcpyAsync(status, r.d_status, n, hipMemcpyDeviceToHost, r.own));
    GPIS_HIP(hipStreamSynchronize(r.own));
    return GPIS_OK;
}
int gpis_render_device(void* render, const float** d_depth, const float** d_rec, const unsigned char** d_status) {
    if (!render) return GPIS_ERR_ARG;
    const Renderer& r = *(Renderer*)render;
    if (d_depth) *d_depth = r.valid ? r.d_depth : nullptr;
    if (d_rec) *d_rec = r.valid ? r.d_rec : nullptr;
    if (d_status) *d_status = r.valid ? r.d_status : nullptr;
    return GPIS_OK;
}
int gpis_render_info(void* render, double* out, int n) {
    if (!render || !out || n < 0) return GPIS_ERR_ARG;
    const Renderer& r = *(Renderer*)render;
    const double v[18] = {(double)r.nrays, (double)r.dim, (double)r.passes, (double)r.march_passes, (double)r.samples,
                          (double)r.evals, r.k4_ms, (double)r.hits, (double)r.box_lo[0], (double)r.box_lo[1], (double)r.box_lo[2],
                          (double)r.box_hi[0], (double)r.box_hi[1], (double)r.box_hi[2], r.valid ? 1.0 : 0.0, r.mq_ms,
                          r.field ? 1.0 : 0.0, (double)r.max_samples};
    for (int i = 0; i < n && i < 18; ++i) out[i] = v[i];
    return GPIS_OK;
}

// ---- rendering from a distance field ---------------------------------------------------------------------------------------
int gpis_render_field_default_opts(int dim, float step, gpis_render_field_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    gpis_render_opts d;
    (void)gpis_render_default_opts(dim, &d);
    o->tnear = d.tnear; o->tfar = d.tfar; o->max_steps = d.max_steps; o->refine = d.refine;
    o->min_step = step * 0.5f; o->max_step = INFINITY; o->slack = 3.0f;
    return GPIS_OK;
}
int gpis_render_set_field_tiles(void* render, int on) {
    if (!render) return GPIS_ERR_ARG;
    ((Renderer*)render)->field_tiles = on != 0;
    return GPIS_OK;
}
// the checks that need neither field nor map, then the field's state and dim (before anything is dropped) and the call on the
// field's device: an argument, state or limit error leaves the previous result readable
static int render_field_call(void* d, void* render, const SensorFrame& f, const float* pose, const gpis_render_field_opts* opts,
                             void* stream) {
    if (!d || !render || !pose) return GPIS_ERR_ARG;
    const int np = f.geo.dim == 3 ? 12 : 6;
    for (int k = 0; k < np; ++k) if (!std::isfinite(pose[k])) return GPIS_ERR_ARG;
    const RayGeom g = ray_geom(f, pose);
    const DistanceField& df = *(const DistanceField*)d;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != g.dim) return GPIS_ERR_ARG;
    gpis_render_field_opts dflt;
    if (!opts) { (void)gpis_render_field_default_opts(g.dim, df.step, &dflt); opts = &dflt; }
    RenderFieldOpts o;
    o.tnear = opts->tnear; o.tfar = opts->tfar; o.min_step = opts->min_step; o.max_step = opts->max_step; o.slack = opts->slack;
    o.refine = opts->refine; o.max_steps = opts->max_steps;
    if (int rc = render_field_check_opts(o)) return rc;
    Renderer& r = *(Renderer*)render;
    DeviceScope ds(df.device);
    try {
        if (int rc = r.bind(df.device)) { r.clear_result(); return rc; }
        const int rc = r.render_field(df, g, f.cs_or_null(), f.n, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) r.clear_result();
        return rc;
    } catch (...) { r.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_render_depth_field(void* m, void* df, void* render, const gpis_cam* cam, const float* pose12,
                             const gpis_render_field_opts* opts, void* stream) {
    if (!cam && !m) return GPIS_ERR_ARG;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return render_field_call(df, render, f, pose12, opts, stream);
}
int gpis2_render_scan_field(void* m, void* df, void* render, const float* thetas, int n, const float* off2, const float* pose6,
                            const gpis_render_field_opts* opts, void* stream) {
    if (!thetas || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) return rc;
    return render_field_call(df, render, f, pose6, opts, stream);
}

// ---- tracking ----------------------------------------------------------------------------------------------------------
static TrackOpts track_opts(const gpis_track_opts* o) {
    TrackOpts t;
    t.max_residual = o->max_residual; t.huber = o->huber; t.max_var = o->max_var; t.damping = o->damping;
    t.eps_t = o->eps_t; t.eps_r = o->eps_r; t.level = o->level; t.stride = o->stride; t.max_iters = o->max_iters;
    t.min_inliers = o->min_inliers;
    return t;
}
int gpis_track_default_opts(int dim, gpis_track_opts* o) {
    if (!o || (dim != 2 && dim != 3)) return GPIS_ERR_ARG;
    if (dim == 3) { o->max_residual = 0.05; o->huber = 0.01; o->min_inliers = 100; }
    else { o->max_residual = 0.5; o->huber = 0.1; o->min_inliers = 20; }
    o->max_var = INFINITY; o->damping = 1e-4; o->eps_t = 1e-5; o->eps_r = 1e-5; o->level = std::nanf("");
    o->stride = 2; o->max_iters = 20;
    return GPIS_OK;
}
void* gpis_track_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Tracker* t = new (std::nothrow) Tracker();
    if (t && !t->own) { delete t; return nullptr; }
    return t;
}
void gpis_track_destroy(void* tracker) { delete (Tracker*)tracker; }
int gpis_track_set_chunk(void* tracker, int points) {
    if (!tracker || points < 0) return GPIS_ERR_ARG;
    ((Tracker*)tracker)->chunk = points ? points : (1 << 22);
    return GPIS_OK;
}
// the checks that need no map: an argument error leaves the previous result readable.  field: level and max_var are not read.
static int track_args(void* tracker, int dim, const float* pose, const gpis_track_opts* opts, TrackOpts* o, bool field = false) {
    if (!tracker || !pose) return GPIS_ERR_ARG;
    gpis_track_opts d;
    if (!opts) { (void)gpis_track_default_opts(dim, &d); opts = &d; }
    *o = track_opts(opts);
    const int np = dim == 3 ? 12 : 6;
    for (int k = 0; k < np; ++k) if (!std::isfinite(pose[k])) return GPIS_ERR_ARG;
    if (field) { o->level = 0.f; o->max_var = INFINITY; }
    if (std::isinf(o->level)) return GPIS_ERR_ARG;
    TrackOpts c = *o;
    c.level = 0.f;                              // (resolved against the map by the entry)
    return track_check_opts(c);
}
int gpis3_track_depth(void* m, void* tracker, const gpis_cam* cam, const float* depth, const float* pose12_init,
                      const gpis_track_opts* opts, float* pose12_out, void* stream) {
    if (!m || !depth) return GPIS_ERR_ARG;
    TrackOpts o;
    if (int rc = track_args(tracker, 3, pose12_init, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    Tracker& t = *(Tracker*)tracker;
    const int rc = gpis3_impl_track((GPisMap3*)m, t, f, depth, pose12_init, o, pose12_out, stream);
    if (rc != GPIS_OK && rc != GPIS_ERR_ARG && rc != GPIS_ERR_LIMIT) t.clear_result();
    return rc;
}
int gpis2_track_scan(void* m, void* tracker, const float* thetas, const float* ranges, int n, const float* pose6_init,
                     const gpis_track_opts* opts, float* pose6_out, void* stream) {
    if (!m || !thetas || !ranges || n < 1) return GPIS_ERR_ARG;
    TrackOpts o;
    if (int rc = track_args(tracker, 2, pose6_init, opts, &o)) return rc;
    Tracker& t = *(Tracker*)tracker;
    SensorFrame f;
    int rc = scan_frame(m, thetas, n, nullptr, &f);
    if (rc == GPIS_OK) rc = gpis2_impl_track((GPisMap*)m, t, f, ranges, pose6_init, o, pose6_out, stream);
    if (rc != GPIS_OK && rc != GPIS_ERR_ARG && rc != GPIS_ERR_LIMIT) t.clear_result();
    return rc;
}
// the field's state and dim (before anything is dropped), then the call on the field's device
static int track_field_call(void* d, Tracker& t, const SensorFrame& f, const float* in, const float* pose_init, const TrackOpts& o,
                            float* pose_out, void* stream) {
    const DistanceField& df = *(const DistanceField*)d;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != f.geo.dim) return GPIS_ERR_ARG;
    const int np = f.geo.dim == 3 ? 12 : 6;
    DeviceScope ds(df.device);
    try {
        if (int rc = t.bind(df.device)) { t.clear_result(); return rc; }
        double p0[12];
        for (int k = 0; k < np; ++k) p0[k] = pose_init[k];
        const int rc = t.track_field(df, f.geo, in, f.cs_or_null(), f.n, p0, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) { t.clear_result(); return rc; }
        if (pose_out) for (int k = 0; k < np; ++k) pose_out[k] = (float)t.pose[k];
        return GPIS_OK;
    } catch (...) { t.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_track_depth_field(void* m, void* df, void* tracker, const gpis_cam* cam, const float* depth, const float* pose12_init,
                            const gpis_track_opts* opts, float* pose12_out, void* stream) {
    if (!df || !depth || (!cam && !m)) return GPIS_ERR_ARG;
    TrackOpts o;
    if (int rc = track_args(tracker, 3, pose12_init, opts, &o, true)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return track_field_call(df, *(Tracker*)tracker, f, depth, pose12_init, o, pose12_out, stream);
}
int gpis2_track_scan_field(void* m, void* df, void* tracker, const float* thetas, const float* ranges, int n, const float* off2,
                           const float* pose6_init, const gpis_track_opts* opts, float* pose6_out, void* stream) {
    if (!df || !thetas || !ranges || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    TrackOpts o;
    if (int rc = track_args(tracker, 2, pose6_init, opts, &o, true)) return rc;
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) { if (rc == GPIS_ERR_STATE) ((Tracker*)tracker)->clear_result(); return rc; }
    return track_field_call(df, *(Tracker*)tracker, f, ranges, pose6_init, o, pose6_out, stream);
}
int gpis_track_get(void* tracker, double* H, double* b, float* resid) {
    if (!tracker) return GPIS_ERR_ARG;
    Tracker& t = *(Tracker*)tracker;
    if (!t.valid) return GPIS_ERR_STATE;
    const int nj = t.dim == 3 ? 6 : 3;
    if (H) for (int k = 0; k < nj * nj; ++k) H[k] = t.H[k];
    if (b) for (int k = 0; k < nj; ++k) b[k] = t.b[k];
    if (resid) {
        DeviceScope ds(t.device);
        GPIS_HIP(hipMemcpyAsync(resid, t.d_resid, sizeof(float) * (size_t)t.pixels, hipMemcpyDeviceToHost, t.own));
        GPIS_HIP(hipStreamSynchronize(t.own));
    }
    return GPIS_OK;
}
int gpis_track_info(void* tracker, double* out, int n) {
    if (!tracker || !out || n < 0) return GPIS_ERR_ARG;
    const Tracker& t = *(Tracker*)tracker;
    const double v[13] = {(double)t.status, (double)t.iterations, (double)t.passes, (double)t.points, t.inliers, t.cost0, t.cost,
                          t.pass_ms, t.k4_ms, t.valid ? 1.0 : 0.0, (double)t.dim, (double)t.pixels, (double)t.evals};
    for (int i = 0; i < n && i < 13; ++i) out[i] = v[i];
    return GPIS_OK;
}

// ---- pose-hypothesis scoring against a distance field ---------------------------------------------------------------------
int gpis_locate_default_opts(int dim, gpis_locate_opts* o) {
    if (!o || (dim != 2 && dim != 3)) return GPIS_ERR_ARG;
    if (dim == 3) { o->max_residual = 0.05; o->stride = 8; }
    else { o->max_residual = 0.5; o->stride = 1; }
    o->top_k = 16;
    return GPIS_OK;
}
void* gpis_locate_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Locator* l = new (std::nothrow) Locator();
    if (l && !l->trk.own) { delete l; return nullptr; }
    return l;
}
void gpis_locate_destroy(void* locator) { delete (Locator*)locator; }
// the checks that need neither the field nor the frame: GPIS_ERR_ARG / GPIS_ERR_LIMIT leave the previous result readable
static int locate_args(void* locator, int dim, const float* poses, int m, const gpis_locate_opts* opts, LocateOpts* o) {
    if (!locator || !poses || m < 1) return GPIS_ERR_ARG;
    gpis_locate_opts d;
    if (!opts) { (void)gpis_locate_default_opts(dim, &d); opts = &d; }
    o->max_residual = opts->max_residual; o->stride = opts->stride; o->top_k = opts->top_k;
    return locate_check_opts(*o);
}
// the pose count's limit (before the poses are read), the poses, the field's state and dim, then the call on the field's device
static int locate_call(void* d, Locator& l, const SensorFrame& f, const float* in, const float* poses, int m, const LocateOpts& o,
                       void* stream) {
    const TrackGeom& g = f.geo;
    if ((long long)m > Locator::kMaxPoses) return GPIS_ERR_LIMIT;
    const size_t np = (size_t)(g.dim == 3 ? 12 : 6) * (size_t)m;
    for (size_t k = 0; k < np; ++k) if (!std::isfinite(poses[k])) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != g.dim) return GPIS_ERR_ARG;
    DeviceScope ds(df.device);
    try {
        if (int rc = l.bind(df.device)) { l.clear_result(); return rc; }
        const int rc = l.score(df, g, in, f.cs_or_null(), f.n, poses, m, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) l.clear_result();
        return rc;
    } catch (...) { l.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_locate_depth_field(void* m, void* df, void* locator, const gpis_cam* cam, const float* depth, const float* poses12, int np,
                             const gpis_locate_opts* opts, void* stream) {
    if (!df || !depth || (!cam && !m)) return GPIS_ERR_ARG;
    LocateOpts o;
    if (int rc = locate_args(locator, 3, poses12, np, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return locate_call(df, *(Locator*)locator, f, depth, poses12, np, o, stream);
}
int gpis2_locate_scan_field(void* m, void* df, void* locator, const float* thetas, const float* ranges, int n, const float* off2,
                            const float* poses6, int np, const gpis_locate_opts* opts, void* stream) {
    if (!df || !thetas || !ranges || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    LocateOpts o;
    if (int rc = locate_args(locator, 2, poses6, np, opts, &o)) return rc;
    if ((long long)np > Locator::kMaxPoses) return GPIS_ERR_LIMIT;   // (as ever in this entry: before the angles are read)
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) { if (rc == GPIS_ERR_STATE) ((Locator*)locator)->clear_result(); return rc; }
    return locate_call(df, *(Locator*)locator, f, ranges, poses6, np, o, stream);
}
int gpis_locate_get(void* locator, double* cost, int* inliers, int* order) {
    if (!locator) return GPIS_ERR_ARG;
    const Locator& l = *(const Locator*)locator;
    if (!l.valid) return GPIS_ERR_STATE;
    if (cost) std::memcpy(cost, l.cost.data(), sizeof(double) * l.cost.size());
    if (inliers) std::memcpy(inliers, l.inliers.data(), sizeof(int) * l.inliers.size());
    if (order) std::memcpy(order, l.order.data(), sizeof(int) * l.order.size());
    return GPIS_OK;
}
int gpis_locate_info(void* locator, double* out, int n) {
    if (!locator || !out || n < 0) return GPIS_ERR_ARG;
    const Locator& l = *(const Locator*)locator;
    const double v[7] = {l.valid ? 1.0 : 0.0, (double)l.dim, (double)l.poses, (double)l.npoints, (double)l.order.size(),
                         (double)l.pixels, l.ms};
    for (int i = 0; i < n && i < 7; ++i) out[i] = v[i];
    return GPIS_OK;
}
int gpis_locate_device(void* locator, void** d_cost, void** d_inliers) {
    if (!locator) return GPIS_ERR_ARG;
    const Locator& l = *(const Locator*)locator;
    if (!l.valid) return GPIS_ERR_STATE;
    if (d_cost) *d_cost = (void*)l.d_cost();
    if (d_inliers) *d_inliers = (void*)l.d_inliers();
    return GPIS_OK;
}

// ---- coverage, frontiers, the field restricted to seen space -----------------------------------------------------------------
int gpis_cover_default_opts(int dim, float step, gpis_cover_opts* o) {
    CoverOpts c;
    if (!o) return GPIS_ERR_ARG;
    if (int rc = cover_default_opts(dim, step, &c)) return rc;
    o->back_off = c.back_off; o->max_gap = c.max_gap; o->clearance = c.clearance; o->min_size = c.min_size; o->max_rounds = c.max_rounds;
    return GPIS_OK;
}
void* gpis_cover_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Coverage* c = new (std::nothrow) Coverage();
    if (c && !c->own) { delete c; return nullptr; }
    return c;
}
void gpis_cover_destroy(void* cover) { delete (Coverage*)cover; }
// the options of a call: the caller's, or the defaults for the holder's lattice; checked before anything is dropped
static int cover_args(void* cover, const gpis_cover_opts* opts, CoverOpts* o) {
    if (!cover) return GPIS_ERR_ARG;
    const Coverage& c = *(const Coverage*)cover;
    if (opts) { o->back_off = opts->back_off; o->max_gap = opts->max_gap; o->clearance = opts->clearance; o->min_size = opts->min_size;
                o->max_rounds = opts->max_rounds; }
    else if (!c.has_lattice) return GPIS_ERR_STATE;
    else (void)cover_default_opts(c.dim, c.step, o);
    return cover_check_opts(*o);
}
int gpis_cover_reset(void* cover, void* d) {
    if (!cover || !d) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    if (!df.valid) return GPIS_ERR_STATE;
    Coverage& c = *(Coverage*)cover;
    DeviceScope ds(df.device);
    try { return c.reset(df); } catch (...) { c.has_lattice = false; return GPIS_ERR_STATE; }
}
int gpis_cover_set(void* cover, const unsigned char* seen, long long n) {
    if (!cover || !seen) return GPIS_ERR_ARG;
    Coverage& c = *(Coverage*)cover;
    if (!c.has_lattice) return GPIS_ERR_STATE;
    if (n != c.ngrid) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    return c.set(seen);
}
int gpis_cover_get(void* cover, unsigned char* seen, long long n) {
    if (!cover || !seen) return GPIS_ERR_ARG;
    Coverage& c = *(Coverage*)cover;
    if (!c.has_lattice) return GPIS_ERR_STATE;
    if (n != c.ngrid) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    return c.get(seen);
}
int gpis_cover_device(void* cover, const unsigned char** d_seen) {
    if (!cover) return GPIS_ERR_ARG;
    const Coverage& c = *(const Coverage*)cover;
    if (d_seen) *d_seen = c.has_lattice ? c.d_seen : nullptr;
    return GPIS_OK;
}
// the pose, the holder's state and dim, then the gather on the holder's device
static int cover_call(Coverage& c, const SensorFrame& f, const float* in, const float* pose, const CoverOpts& o, void* stream) {
    for (int k = 0; k < (f.geo.dim == 3 ? 12 : 6); ++k) if (!std::isfinite(pose[k])) return GPIS_ERR_ARG;
    if (!c.has_lattice) return GPIS_ERR_STATE;
    if (c.dim != f.geo.dim) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    try {
        return c.integrate(f, in, pose, o, stream ? (hipStream_t)stream : c.own);
    } catch (...) { return GPIS_ERR_STATE; }
}
int gpis3_cover_depth(void* m, void* cover, const gpis_cam* cam, const float* depth, const float* pose12, const gpis_cover_opts* opts,
                      void* stream) {
    if (!cover || !depth || !pose12 || (!cam && !m)) return GPIS_ERR_ARG;
    CoverOpts o;
    if (int rc = cover_args(cover, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return cover_call(*(Coverage*)cover, f, depth, pose12, o, stream);
}
int gpis2_cover_scan(void* m, void* cover, const float* thetas, const float* ranges, int n, const float* pose6, const float* off2,
                     const gpis_cover_opts* opts, void* stream) {
    if (!cover || !thetas || !ranges || !pose6 || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    CoverOpts o;
    if (int rc = cover_args(cover, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) return rc;
    return cover_call(*(Coverage*)cover, f, ranges, pose6, o, stream);
}
int gpis_cover_frontiers(void* cover, void* d, const gpis_cover_opts* opts, void* stream) {
    if (!cover || !d) return GPIS_ERR_ARG;
    CoverOpts o;
    if (int rc = cover_args(cover, opts, &o)) return rc;
    Coverage& c = *(Coverage*)cover;
    const DistanceField& df = *(const DistanceField*)d;
    if (!c.has_lattice || !df.valid) return GPIS_ERR_STATE;
    if (!c.same_lattice(df)) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    try {
        const int rc = c.frontiers(df, o, stream ? (hipStream_t)stream : c.own);
        if (rc != GPIS_OK) c.clear_frontiers();
        return rc;
    } catch (...) { c.clear_frontiers(); return GPIS_ERR_STATE; }
}
int gpis_cover_counts(void* cover, long long* npoints, long long* ncomponents, long long* nclusters) {
    if (!cover) return GPIS_ERR_ARG;
    const Coverage& c = *(const Coverage*)cover;
    if (!c.frontiers_valid) return GPIS_ERR_STATE;
    if (npoints) *npoints = c.npoints;
    if (ncomponents) *ncomponents = c.ncomponents;
    if (nclusters) *nclusters = (long long)c.label.size();
    return GPIS_OK;
}
int gpis_cover_get_frontiers(void* cover, int* label, int* count, long long* sums, int* box, int* rep, int* points, int* point_label) {
    if (!cover) return GPIS_ERR_ARG;
    Coverage& c = *(Coverage*)cover;
    if (!c.frontiers_valid) return GPIS_ERR_STATE;
    const size_t nc = c.label.size();
    if (label && nc) std::memcpy(label, c.label.data(), sizeof(int) * nc);
    if (count && nc) std::memcpy(count, c.count.data(), sizeof(int) * nc);
    if (sums && nc) std::memcpy(sums, c.sums.data(), sizeof(long long) * 3 * nc);
    if (box && nc) std::memcpy(box, c.box.data(), sizeof(int) * 6 * nc);
    if (rep && nc) std::memcpy(rep, c.rep.data(), sizeof(int) * nc);
    if ((points || point_label) && c.npoints > 0) {
        DeviceScope ds(c.device);
        const size_t m = (size_t)c.npoints;
        if (points) GPIS_HIP(hipMemcpyAsync(points, c.comp.d_list, sizeof(int) * m, hipMemcpyDeviceToHost, c.own));
        if (point_label) GPIS_HIP(hipMemcpyAsync(point_label, c.d_plabel, sizeof(int) * m, hipMemcpyDeviceToHost, c.own));
        GPIS_HIP(hipStreamSynchronize(c.own));
    }
    return GPIS_OK;
}
int gpis_cover_restrict(void* cover, void* d_in, void* d_out, float unseen_dist, void* stream) {
    if (!cover || !d_in || !d_out || d_in == d_out || !std::isfinite(unseen_dist)) return GPIS_ERR_ARG;
    Coverage& c = *(Coverage*)cover;
    const DistanceField& in = *(const DistanceField*)d_in;
    DistanceField& out = *(DistanceField*)d_out;
    if (!c.has_lattice || !in.valid) return GPIS_ERR_STATE;
    if (!c.same_lattice(in)) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    try {
        const int rc = c.restrict_field(in, out, unseen_dist, stream ? (hipStream_t)stream : c.own);
        if (rc != GPIS_OK) out.clear_result();
        return rc;
    } catch (...) { out.clear_result(); return GPIS_ERR_STATE; }
}
int gpis_cover_info(void* cover, double* out, int n) {
    if (!cover || !out || n < 0) return GPIS_ERR_ARG;
    const Coverage& c = *(const Coverage*)cover;
    const bool v = c.has_lattice;
    const double w[14] = {v ? 1.0 : 0.0, v ? (double)c.dim : 0.0, v ? (double)c.n[0] : 0.0, v ? (double)c.n[1] : 0.0, v ? (double)c.n[2] : 0.0,
                          v ? (double)c.step : 0.0, (double)c.frames, c.frontiers_valid ? 1.0 : 0.0, (double)c.npoints,
                          (double)c.ncomponents, (double)c.label.size(), (double)c.rounds, c.integrate_ms, c.frontiers_ms};
    for (int i = 0; i < n && i < 14; ++i) out[i] = w[i];
    return GPIS_OK;
}

// ---- moving obstacles detected from a frame's residual against a field -----------------------------------------------------
static void detect_opts_out(const DetectOpts& c, gpis_detect_opts* o) {
    o->min_dist = c.min_dist; o->link = c.link; o->pad = c.pad; o->max_radius = c.max_radius; o->gate = c.gate;
    o->max_speed = c.max_speed; o->alpha = c.alpha; o->min_points = c.min_points; o->max_missed = c.max_missed; o->stride = c.stride;
    o->max_rounds = c.max_rounds;
}
int gpis_detect_default_opts(int dim, float step, gpis_detect_opts* o) {
    DetectOpts c;
    if (!o) return GPIS_ERR_ARG;
    if (int rc = detect_default_opts(dim, step, &c)) return rc;
    detect_opts_out(c, o);
    return GPIS_OK;
}
void* gpis_detect_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Detector* d = new (std::nothrow) Detector();
    if (d && !d->trk.own) { delete d; return nullptr; }
    return d;
}
void gpis_detect_destroy(void* det) { delete (Detector*)det; }
int gpis_detect_set_schedule(void* det, int check_every, int profile) {
    if (!det || check_every < 0) return GPIS_ERR_ARG;
    Detector& d = *(Detector*)det;
    if (check_every > 0) d.comp.check_every = std::min(check_every, kCompMaxBatch);
    d.profile = profile != 0;
    return GPIS_OK;
}
int gpis_detect_reset_tracks(void* det) {
    if (!det) return GPIS_ERR_ARG;
    ((Detector*)det)->tracks.reset();
    return GPIS_OK;
}
// every refusal comes before the previous result is touched: the options (the caller's, or the defaults for the field's step),
// the frame, then Detector::check
static int detect_call(void* d, void* det, void* cover, const SensorFrame& f, const float* in, const double* pose, double t,
                       const gpis_detect_opts* opts, void* stream) {
    const DistanceField& df = *(const DistanceField*)d;
    Detector& dt = *(Detector*)det;
    DetectOpts o;
    if (opts) {
        o.min_dist = opts->min_dist; o.link = opts->link; o.pad = opts->pad; o.max_radius = opts->max_radius; o.gate = opts->gate;
        o.max_speed = opts->max_speed; o.alpha = opts->alpha; o.min_points = opts->min_points; o.max_missed = opts->max_missed;
        o.stride = opts->stride; o.max_rounds = opts->max_rounds;
    } else if (!df.valid) return GPIS_ERR_STATE;
    else (void)detect_default_opts(df.dim, df.step, &o);
    if (int rc = dt.check(df, (const Coverage*)cover, f.geo, f.n, pose, o, t)) return rc;
    DeviceScope ds(df.device);
    try {
        if (int rc = dt.bind(df.device)) { dt.clear_result(); return rc; }
        const int rc = dt.detect(df, (const Coverage*)cover, f.geo, in, f.cs_or_null(), f.n, pose, o, t, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) dt.clear_result();
        return rc;
    } catch (...) { dt.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_detect_depth_field(void* m, void* df, void* det, void* cover, const gpis_cam* cam, const float* depth, const double* pose12,
                             double t, const gpis_detect_opts* opts, void* stream) {
    if (!df || !det || !depth || !pose12 || (!cam && !m)) return GPIS_ERR_ARG;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return detect_call(df, det, cover, f, depth, pose12, t, opts, stream);
}
int gpis2_detect_scan_field(void* m, void* df, void* det, void* cover, const float* thetas, const float* ranges, int n, const float* off2,
                            const double* pose6, double t, const gpis_detect_opts* opts, void* stream) {
    if (!df || !det || !thetas || !ranges || !pose6 || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) return rc;
    return detect_call(df, det, cover, f, ranges, pose6, t, opts, stream);
}
int gpis_detect_counts(void* det, long long* grid, long long* components, long long* balls) {
    if (!det) return GPIS_ERR_ARG;
    const Detector& d = *(const Detector*)det;
    if (!d.valid) return GPIS_ERR_STATE;
    if (grid) *grid = d.grid;
    if (components) *components = d.ncomp;
    if (balls) *balls = (long long)d.balls.size();
    return GPIS_OK;
}
int gpis_detect_get_balls(void* det, double* centre, double* velocity, double* radius, int* count, float* box, int* label, int* id,
                          int* age, int* missed) {
    if (!det) return GPIS_ERR_ARG;
    const Detector& d = *(const Detector*)det;
    if (!d.valid) return GPIS_ERR_STATE;
    for (size_t i = 0; i < d.balls.size(); ++i) {
        const DetBall& b = d.balls[i];
        for (int a = 0; a < d.dim; ++a) {
            if (centre) centre[i * d.dim + a] = b.c[a];
            if (velocity) velocity[i * d.dim + a] = b.v[a];
        }
        if (radius) radius[i] = b.r;
        if (count) count[i] = b.comp >= 0 ? d.c_count[b.comp] : 0;
        if (label) label[i] = b.comp >= 0 ? d.c_label[b.comp] : -1;
        if (box) for (int a = 0; a < 6; ++a) box[i * 6 + a] = b.comp >= 0 ? d.c_box[(size_t)b.comp * 6 + a] : 0.f;
        if (id) id[i] = b.id;
        if (age) age[i] = b.age;
        if (missed) missed[i] = b.missed;
    }
    return GPIS_OK;
}
int gpis_detect_get_components(void* det, int* label, int* count, float* box, double* centre, double* r2, int* flag) {
    if (!det) return GPIS_ERR_ARG;
    const Detector& d = *(const Detector*)det;
    if (!d.valid) return GPIS_ERR_STATE;
    const size_t nc = (size_t)d.ncomp;
    if (label && nc) std::memcpy(label, d.c_label.data(), sizeof(int) * nc);
    if (count && nc) std::memcpy(count, d.c_count.data(), sizeof(int) * nc);
    if (box && nc) std::memcpy(box, d.c_box.data(), sizeof(float) * 6 * nc);
    if (centre && nc) std::memcpy(centre, d.c_centre.data(), sizeof(double) * 3 * nc);
    if (r2 && nc) std::memcpy(r2, d.c_r2.data(), sizeof(double) * nc);
    if (flag && nc) std::memcpy(flag, d.c_flag.data(), sizeof(int) * nc);
    return GPIS_OK;
}
int gpis_detect_get_samples(void* det, int* label, float* dist, float* x, unsigned char* foreign) {
    if (!det) return GPIS_ERR_ARG;
    Detector& d = *(Detector*)det;
    if (!d.valid) return GPIS_ERR_STATE;
    if (d.grid < 1) return GPIS_OK;
    DeviceScope ds(d.device);
    const size_t g = (size_t)d.grid;
    hipStream_t s = d.trk.own;
    if (label) GPIS_HIP(hipMemcpyAsync(label, d.d_limg, sizeof(int) * g, hipMemcpyDeviceToHost, s));
    if (dist) GPIS_HIP(hipMemcpyAsync(dist, d.d_d, sizeof(float) * g, hipMemcpyDeviceToHost, s));
    if (x) GPIS_HIP(hipMemcpyAsync(x, d.d_x, sizeof(float) * g * d.dim, hipMemcpyDeviceToHost, s));
    if (foreign) GPIS_HIP(hipMemcpyAsync(foreign, d.d_flag, g, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}
int gpis_detect_to_obstacles(void* det, void* obst) {
    if (!det || !obst) return GPIS_ERR_ARG;
    try { return ((const Detector*)det)->to_obstacles(*(Obstacles*)obst); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_detect_info(void* det, double* out, int n) {
    if (!det || !out || n < 0) return GPIS_ERR_ARG;
    const Detector& d = *(const Detector*)det;
    const double v[22] = {d.valid ? 1.0 : 0.0, (double)d.dim, (double)d.grid, (double)d.gw, (double)d.gh, (double)d.samples, (double)d.foreign,
                          (double)d.ncomp, (double)d.balls.size(), (double)d.noise, (double)d.large, (double)d.dropped, (double)d.rounds,
                          (double)d.tracks.balls.size(), d.tracks.held ? 1.0 : 0.0, d.tracks.t_prev, d.ms, d.setup_ms, d.flag_ms,
                          d.compact_ms, d.label_ms, d.table_ms};
    for (int i = 0; i < n && i < 22; ++i) out[i] = v[i];
    return GPIS_OK;
}

// ---- candidate viewpoints scored by the unseen space they would reveal ------------------------------------------------------
int gpis_view_default_opts(int dim, float step, gpis_view_opts* o) {
    if (!o) return GPIS_ERR_ARG;
    if (int rc = gpis_render_field_default_opts(dim, step, &o->march)) return rc;
    return view_default_tail(dim, step, o);
}
void* gpis_view_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    ViewScorer* v = new (std::nothrow) ViewScorer();
    if (v && !v->own) { delete v; return nullptr; }
    return v;
}
void gpis_view_destroy(void* view) { delete (ViewScorer*)view; }
// the options of a call: the caller's, or the defaults for the field's step; the march's checks and the rule's
static int view_args(void* d, int dim, const gpis_view_opts* opts, gpis_view_opts* o) {
    if (opts) *o = *opts;
    else {
        const DistanceField& df = *(const DistanceField*)d;
        if (!df.valid) return GPIS_ERR_STATE;
        if (int rc = gpis_view_default_opts(dim, df.step, o)) return rc;
    }
    RenderFieldOpts r;
    r.tnear = o->march.tnear; r.tfar = o->march.tfar; r.min_step = o->march.min_step; r.max_step = o->march.max_step;
    r.slack = o->march.slack; r.refine = o->march.refine; r.max_steps = o->march.max_steps;
    if (int rc = render_field_check_opts(r)) return rc;
    return view_check_tail(*o);
}
// the batch's limits (before the poses are read), the poses, the field's and the coverage's state, then the call on the field's
// device: every refusal leaves the previous result readable
static int view_call(void* d, void* cover, ViewScorer& v, const SensorFrame& f, const float* poses, int m, const gpis_view_opts& o,
                     void* stream) {
    if (int rc = view_check_batch(m, f.n)) return rc;
    const size_t np = (size_t)(f.geo.dim == 3 ? 12 : 6) * (size_t)m;
    for (size_t k = 0; k < np; ++k) if (!std::isfinite(poses[k])) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    const Coverage& c = *(const Coverage*)cover;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != f.geo.dim) return GPIS_ERR_ARG;
    if (!c.same_lattice(df)) return GPIS_ERR_STATE;
    DeviceScope ds(df.device);
    try {
        if (int rc = v.bind(df.device)) { v.clear_result(); return rc; }
        const int rc = v.score(df, c, f, poses, m, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) v.clear_result();
        return rc;
    } catch (...) { v.clear_result(); return GPIS_ERR_STATE; }
}
int gpis3_view_gain_depth(void* m, void* df, void* cover, void* view, const gpis_cam* cam, const float* poses12, int np,
                          const gpis_view_opts* opts, void* stream) {
    if (!df || !cover || !view || !poses12 || np < 1 || (!cam && !m)) return GPIS_ERR_ARG;
    gpis_view_opts o;
    if (int rc = view_args(df, 3, opts, &o)) return rc;
    SensorFrame f;
    if (int rc = depth_frame(m, cam, &f)) return rc;
    return view_call(df, cover, *(ViewScorer*)view, f, poses12, np, o, stream);
}
int gpis2_view_gain_scan(void* m, void* df, void* cover, void* view, const float* thetas, int n, const float* off2, const float* poses6,
                         int np, const gpis_view_opts* opts, void* stream) {
    if (!df || !cover || !view || !thetas || !poses6 || n < 1 || np < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    gpis_view_opts o;
    if (int rc = view_args(df, 2, opts, &o)) return rc;
    if (int rc = view_check_batch(np, n)) return rc;         // (before the angles are read, too)
    SensorFrame f;
    if (int rc = scan_frame(m, thetas, n, off2, &f)) return rc;
    return view_call(df, cover, *(ViewScorer*)view, f, poses6, np, o, stream);
}
int gpis_view_get(void* view, long long* gain, int* hits, int m) {
    if (!view) return GPIS_ERR_ARG;
    const ViewScorer& v = *(const ViewScorer*)view;
    if (!v.valid) return GPIS_ERR_STATE;
    if ((long long)m != v.poses) return GPIS_ERR_ARG;
    if (gain) std::memcpy(gain, v.gain.data(), sizeof(long long) * v.gain.size());
    if (hits) std::memcpy(hits, v.hits.data(), sizeof(int) * v.hits.size());
    return GPIS_OK;
}
int gpis_view_get_predicted(void* view, int pose, float* out, long long n) {
    if (!view || !out) return GPIS_ERR_ARG;
    ViewScorer& v = *(ViewScorer*)view;
    if (!v.valid) return GPIS_ERR_STATE;
    if (pose < 0 || (long long)pose >= v.poses || n != v.rays) return GPIS_ERR_ARG;
    DeviceScope ds(v.device);
    return v.predicted(pose, out);
}
int gpis_view_info(void* view, double* out, int n) {
    if (!view || !out || n < 0) return GPIS_ERR_ARG;
    const ViewScorer& v = *(const ViewScorer*)view;
    const double w[10] = {v.valid ? 1.0 : 0.0, (double)v.dim, (double)v.poses, (double)v.rays, (double)v.targets, (double)v.samples,
                          v.predict_ms, v.table_ms, v.target_ms, v.gather_ms};
    for (int i = 0; i < n && i < 10; ++i) out[i] = w[i];
    return GPIS_OK;
}

// ---- the particle filter --------------------------------------------------------------------------------------------------
int gpis_pf_default_opts(int dim, gpis_pf_opts* o) {
    if (!o || (dim != 2 && dim != 3)) return GPIS_ERR_ARG;
    if (dim == 3) {
        o->max_residual = 0.05; o->beta = 100.0; o->sigma_t[0] = o->sigma_t[1] = o->sigma_t[2] = 0.003; o->sigma_r = 0.003; o->stride = 8;
    } else {
        o->max_residual = 0.5; o->beta = 2.0; o->sigma_t[0] = o->sigma_t[1] = 0.03; o->sigma_t[2] = 0.0; o->sigma_r = 0.03; o->stride = 1;
    }
    o->resample_below = 0.5;
    return GPIS_OK;
}
void* gpis_pf_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    ParticleFilter* f = new (std::nothrow) ParticleFilter();
    if (f && !f->trk.own) { delete f; return nullptr; }
    return f;
}
void gpis_pf_destroy(void* pf) { delete (ParticleFilter*)pf; }
int gpis_pf_init(void* pf, int dim, const float* poses, int m, unsigned long long seed) {
    if (!pf || !poses || (dim != 2 && dim != 3) || m < 1) return GPIS_ERR_ARG;
    if ((long long)m > ParticleFilter::kMaxParticles) return GPIS_ERR_LIMIT;
    const size_t np = (size_t)(dim == 3 ? 12 : 6) * (size_t)m;
    for (size_t k = 0; k < np; ++k) if (!std::isfinite(poses[k])) return GPIS_ERR_ARG;
    ParticleFilter& f = *(ParticleFilter*)pf;
    try { return f.init(dim, poses, m, seed); } catch (...) { f.inited = false; return GPIS_ERR_STATE; }
}
// the options of a call (NULL: the defaults of the filter's dim), checked
static int pf_args(const ParticleFilter& f, const gpis_pf_opts* opts, PfOpts* o) {
    gpis_pf_opts d;
    if (!opts) { (void)gpis_pf_default_opts(f.dim, &d); opts = &d; }
    o->max_residual = opts->max_residual; o->beta = opts->beta; o->sigma_r = opts->sigma_r; o->resample_below = opts->resample_below;
    for (int a = 0; a < 3; ++a) o->sigma_t[a] = opts->sigma_t[a];
    o->stride = opts->stride;
    return pf_check_opts(*o);
}
int gpis_pf_predict(void* pf, const double* motion, const gpis_pf_opts* opts, void* stream) {
    if (!pf || !motion) return GPIS_ERR_ARG;
    ParticleFilter& f = *(ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    PfOpts o;
    if (int rc = pf_args(f, opts, &o)) return rc;
    for (int k = 0; k < (f.dim == 3 ? 12 : 6); ++k) if (!std::isfinite(motion[k])) return GPIS_ERR_ARG;
    double mo[7];
    for (int k = 0; k < f.dim; ++k) mo[k] = motion[k];
    if (f.dim == 3) pf_mat_to_quat(motion + 3, mo + 3);
    else { mo[2] = motion[2]; mo[3] = motion[3]; }
    DeviceScope ds(f.device);
    return f.predict(mo, o, f.stream_or_own((hipStream_t)stream));
}
// the filter's and the field's state, dim and device (before anything is touched), then the call on that device
static int pf_update_call(void* d, ParticleFilter& f, const SensorFrame& fr, const float* in, const PfOpts& o, void* stream) {
    const DistanceField& df = *(const DistanceField*)d;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != fr.geo.dim || df.device != f.device) return GPIS_ERR_ARG;
    DeviceScope ds(f.device);
    try { return f.update(df, fr.geo, in, fr.cs_or_null(), fr.n, o, f.stream_or_own((hipStream_t)stream)); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis3_pf_update_depth(void* m, void* df, void* pf, const gpis_cam* cam, const float* depth, const gpis_pf_opts* opts, void* stream) {
    if (!df || !pf || !depth || (!cam && !m)) return GPIS_ERR_ARG;
    ParticleFilter& f = *(ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    if (f.dim != 3) return GPIS_ERR_ARG;
    PfOpts o;
    if (int rc = pf_args(f, opts, &o)) return rc;
    SensorFrame fr;
    if (int rc = depth_frame(m, cam, &fr)) return rc;
    return pf_update_call(df, f, fr, depth, o, stream);
}
int gpis2_pf_update_scan(void* m, void* df, void* pf, const float* thetas, const float* ranges, int n, const float* off2,
                         const gpis_pf_opts* opts, void* stream) {
    if (!df || !pf || !thetas || !ranges || n < 1 || (!off2 && !m)) return GPIS_ERR_ARG;
    ParticleFilter& f = *(ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    if (f.dim != 2) return GPIS_ERR_ARG;
    PfOpts o;
    if (int rc = pf_args(f, opts, &o)) return rc;
    SensorFrame fr;
    if (int rc = scan_frame(m, thetas, n, off2, &fr)) return rc;
    return pf_update_call(df, f, fr, ranges, o, stream);
}
int gpis_pf_resample(void* pf, void* stream) {
    if (!pf) return GPIS_ERR_ARG;
    ParticleFilter& f = *(ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    DeviceScope ds(f.device);
    return f.resample(f.stream_or_own((hipStream_t)stream));
}
int gpis_pf_estimate(void* pf, double* pose, double* neff, unsigned long long* totals, int* resampled) {
    if (!pf) return GPIS_ERR_ARG;
    const ParticleFilter& f = *(const ParticleFilter*)pf;
    if (!f.inited || !f.have_estimate) return GPIS_ERR_STATE;
    if (pose) for (int k = 0; k < (f.dim == 3 ? 12 : 6); ++k) pose[k] = f.est_pose[k];
    if (neff) *neff = f.neff;
    if (totals) { totals[0] = f.stats.T; totals[1] = f.stats.Th; totals[2] = f.stats.S2; }
    if (resampled) *resampled = f.resampled ? 1 : 0;
    return GPIS_OK;
}
int gpis_pf_get(void* pf, double* state, double* L, unsigned long long* q, double* cost, int* inliers, int* ancestors, float* poses) {
    if (!pf) return GPIS_ERR_ARG;
    const ParticleFilter& f = *(const ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    DeviceScope ds(f.device);
    const size_t n = (size_t)f.m;
    hipStream_t s = f.trk.own;
    if (state) GPIS_HIP(hipMemcpyAsync(state, f.state(), sizeof(double) * (f.dim == 3 ? 7 : 4) * n, hipMemcpyDeviceToHost, s));
    if (L) GPIS_HIP(hipMemcpyAsync(L, f.d_L, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (q) GPIS_HIP(hipMemcpyAsync(q, f.d_q, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, s));
    if (cost) GPIS_HIP(hipMemcpyAsync(cost, f.d_cost, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (inliers) GPIS_HIP(hipMemcpyAsync(inliers, f.d_inl, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (ancestors) GPIS_HIP(hipMemcpyAsync(ancestors, f.d_anc, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (poses) GPIS_HIP(hipMemcpyAsync(poses, f.poses(), sizeof(float) * (f.dim == 3 ? 12 : 6) * n, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}
int gpis_pf_device(void* pf, void** ptrs, int n) {
    if (!pf || !ptrs || n < 0) return GPIS_ERR_ARG;
    const ParticleFilter& f = *(const ParticleFilter*)pf;
    if (!f.inited) return GPIS_ERR_STATE;
    void* v[7] = {(void*)f.state(), (void*)f.poses(), (void*)f.d_L, (void*)f.d_q, (void*)f.d_cost, (void*)f.d_inl, (void*)f.d_anc};
    for (int i = 0; i < n && i < 7; ++i) ptrs[i] = v[i];
    return GPIS_OK;
}
int gpis_pf_info(void* pf, double* out, int n) {
    if (!pf || !out || n < 0) return GPIS_ERR_ARG;
    const ParticleFilter& f = *(const ParticleFilter*)pf;
    const double v[11] = {f.inited ? 1.0 : 0.0, (double)f.dim, (double)f.m, (double)f.tick, (double)f.npoints, (double)f.pixels,
                          (double)f.updates, (double)f.resamples, f.resampled ? 1.0 : 0.0, f.neff, f.ms};
    for (int i = 0; i < n && i < 11; ++i) out[i] = v[i];
    return GPIS_OK;
}

// ---- the sampling controller ----------------------------------------------------------------------------------------------
static void mppi_opts_out(const MppiOpts& d, gpis_mppi_opts* o) {
    o->dt = d.dt; o->lambda = d.lambda; o->gamma = d.gamma; o->clearance = d.clearance; o->margin = d.margin;
    o->w_obs = d.w_obs; o->w_col = d.w_col; o->w_off = d.w_off; o->w_goal = d.w_goal;
    for (int u = 0; u < 4; ++u) { o->sigma[u] = d.sigma[u]; o->umin[u] = d.umin[u]; o->umax[u] = d.umax[u]; }
}
int gpis_mppi_default_opts(int dim, float step, gpis_mppi_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !std::isfinite(step) || !(step > 0.f)) return GPIS_ERR_ARG;
    MppiOpts d;
    mppi_default_opts(dim, step, &d);
    mppi_opts_out(d, o);
    return GPIS_OK;
}
void* gpis_mppi_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Controller* c = new (std::nothrow) Controller();
    if (c && !c->own) { delete c; return nullptr; }
    return c;
}
void gpis_mppi_destroy(void* mppi) { delete (Controller*)mppi; }
int gpis_mppi_init(void* mppi, int dim, int K, int T, unsigned long long seed) {
    if (!mppi || (dim != 2 && dim != 3) || K < 1 || T < 1) return GPIS_ERR_ARG;
    if (K > Controller::kMaxRollouts || T > Controller::kMaxSteps) return GPIS_ERR_LIMIT;
    Controller& c = *(Controller*)mppi;
    try { return c.init(dim, K, T, seed); } catch (...) { c.inited = false; return GPIS_ERR_STATE; }
}
int gpis_mppi_set_nominal(void* mppi, const double* U) {
    if (!mppi || !U) return GPIS_ERR_ARG;
    Controller& c = *(Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    for (int k = 0; k < c.T * c.nu(); ++k) if (!std::isfinite(U[k])) return GPIS_ERR_ARG;
    DeviceScope ds(c.device);
    return c.set_nominal(U);
}
// gpis_mppi_step, gpis_obst_mppi_step and gpis_body_mppi_step: obst NULL or empty and body NULL or empty is the plain step, launch
// for launch
static int mppi_step_checked(void* mppi, void* df, void* plan, const Obstacles* ob, double t_now, const double* pose, const double* goal,
                             const gpis_mppi_opts* opts, double* u0, void* stream, const Footprint* body = nullptr) {
    if (!mppi || !df || !pose || (plan != nullptr) == (goal != nullptr)) return GPIS_ERR_ARG;
    Controller& c = *(Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    const DistanceField& f = *(const DistanceField*)df;
    if (!f.valid) return GPIS_ERR_STATE;
    if (f.dim != c.dim || f.device != c.device) return GPIS_ERR_ARG;
    if (!std::isfinite(t_now)) return GPIS_ERR_ARG;
    if (ob && (ob->device != c.device || (ob->inited && ob->dim != c.dim))) return GPIS_ERR_ARG;
    if (body && (body->device != c.device || (body->inited && body->dim != c.dim))) return GPIS_ERR_ARG;
    MppiOpts o;
    if (opts) {
        o.dt = opts->dt; o.lambda = opts->lambda; o.gamma = opts->gamma; o.clearance = opts->clearance; o.margin = opts->margin;
        o.w_obs = opts->w_obs; o.w_col = opts->w_col; o.w_off = opts->w_off; o.w_goal = opts->w_goal;
        for (int u = 0; u < 4; ++u) { o.sigma[u] = opts->sigma[u]; o.umin[u] = opts->umin[u]; o.umax[u] = opts->umax[u]; }
    } else mppi_default_opts(c.dim, f.step, &o);
    if (int rc = mppi_check_opts(o)) return rc;
    const int dim = c.dim;
    double start[5];
    for (int a = 0; a < dim + 2; ++a) if (!std::isfinite(pose[a])) return GPIS_ERR_ARG;
    const double r0 = pose[dim], r1 = pose[dim + 1], n = std::sqrt(r0 * r0 + r1 * r1);
    if (!(n > 0.0) || !std::isfinite(n)) return GPIS_ERR_ARG;
    for (int a = 0; a < dim; ++a) start[a] = pose[a];
    start[dim] = r0 / n; start[dim + 1] = r1 / n;
    if (goal) for (int a = 0; a < dim; ++a) if (!std::isfinite(goal[a])) return GPIS_ERR_ARG;
    const Planner* pl = (const Planner*)plan;
    if (pl) {
        if (!pl->valid) return GPIS_ERR_STATE;
        if (pl->dim != dim || pl->device != c.device || pl->step != f.step) return GPIS_ERR_ARG;
        for (int a = 0; a < 3; ++a) if (pl->n[a] != f.n[a] || pl->origin[a] != f.origin[a]) return GPIS_ERR_ARG;
    }
    ObstArgs oa{};
    const bool seen = ob && ob->n > 0;
    if (seen) {
        oa.tab = ob->d_tab; oa.n = ob->n; oa.E0 = t_now - ob->epoch;
        oa.clearance = ob->opts.clearance; oa.band = ob->opts.clearance + ob->opts.margin; oa.margin = ob->opts.margin;
        oa.w_obs = ob->opts.w_obs; oa.w_col = ob->opts.w_col;
    }
    const bool wide = body && body->m > 0;
    const BodyArgs ba{wide ? body->d_tab : nullptr, wide ? body->m : 0};
    DeviceScope ds(c.device);
    try {
        const int rc = c.step(f, pl, start, goal, o, c.stream_or_own((hipStream_t)stream), seen ? &oa : nullptr, wide ? &ba : nullptr);
        if (rc == GPIS_OK && u0) for (int u = 0; u < c.nu(); ++u) u0[u] = c.stats.u0[u];
        return rc;
    } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_mppi_step(void* mppi, void* df, void* plan, const double* pose, const double* goal, const gpis_mppi_opts* opts, double* u0,
                   void* stream) {
    return mppi_step_checked(mppi, df, plan, nullptr, 0.0, pose, goal, opts, u0, stream);
}
int gpis_mppi_shift(void* mppi) {
    if (!mppi) return GPIS_ERR_ARG;
    Controller& c = *(Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    DeviceScope ds(c.device);
    return c.shift();
}
int gpis_mppi_get(void* mppi, double* U, double* J, unsigned long long* q, int* hits, double* nominal_states, double* stats) {
    if (!mppi) return GPIS_ERR_ARG;
    const Controller& c = *(const Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    DeviceScope ds(c.device);
    const size_t k = (size_t)c.K;
    hipStream_t s = c.own;
    if (U) GPIS_HIP(hipMemcpyAsync(U, c.d_U[c.cur], sizeof(double) * (size_t)c.T * c.nu(), hipMemcpyDeviceToHost, s));
    if (J) GPIS_HIP(hipMemcpyAsync(J, c.d_J, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    if (q) GPIS_HIP(hipMemcpyAsync(q, c.d_q, sizeof(unsigned long long) * k, hipMemcpyDeviceToHost, s));
    if (hits) GPIS_HIP(hipMemcpyAsync(hits, c.d_hits, sizeof(int) * k, hipMemcpyDeviceToHost, s));
    if (nominal_states)
        GPIS_HIP(hipMemcpyAsync(nominal_states, c.d_nom, sizeof(double) * (size_t)(c.T + 1) * (c.dim + 2), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    if (stats) {
        const double v[10] = {c.stats.jmin, (double)c.stats.best, c.neff, (double)c.stats.T, (double)c.stats.Th, (double)c.stats.S2,
                              (double)c.stats.nhit, c.stats.nominal_cost, (double)c.stats.nominal_hits, c.have_step ? 1.0 : 0.0};
        for (int i = 0; i < 10; ++i) stats[i] = v[i];
    }
    return GPIS_OK;
}
int gpis_mppi_device(void* mppi, void** ptrs, int n) {
    if (!mppi || !ptrs || n < 0) return GPIS_ERR_ARG;
    const Controller& c = *(const Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    void* v[5] = {(void*)c.d_U[c.cur], (void*)c.d_J, (void*)c.d_q, (void*)c.d_hits, (void*)c.d_nom};
    for (int i = 0; i < n && i < 5; ++i) ptrs[i] = v[i];
    return GPIS_OK;
}
int gpis_mppi_info(void* mppi, double* out, int n) {
    if (!mppi || !out || n < 0) return GPIS_ERR_ARG;
    const Controller& c = *(const Controller*)mppi;
    const double v[8] = {c.inited ? 1.0 : 0.0, (double)c.dim, (double)c.K, (double)c.T, (double)c.tick, (double)c.steps,
                         c.have_step ? 1.0 : 0.0, c.ms};
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return GPIS_OK;
}

// ---- moving obstacles -----------------------------------------------------------------------------------------------------
int gpis_obst_default_opts(int dim, float step, gpis_obst_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !std::isfinite(step) || !(step > 0.f)) return GPIS_ERR_ARG;
    ObstOpts d;
    obst_default_opts(dim, step, &d);
    o->clearance = d.clearance; o->margin = d.margin; o->w_obs = d.w_obs; o->w_col = d.w_col;
    return GPIS_OK;
}
void* gpis_obst_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Obstacles* b = new (std::nothrow) Obstacles();
    if (b && !b->ok()) { delete b; return nullptr; }
    return b;
}
void gpis_obst_destroy(void* obst) { delete (Obstacles*)obst; }
int gpis_obst_set(void* obst, int dim, int n, const double* centre, const double* velocity, const double* radius, double epoch) {
    if (!obst || (dim != 2 && dim != 3) || n < 0) return GPIS_ERR_ARG;
    if (n > Obstacles::kMax) return GPIS_ERR_LIMIT;
    if (n > 0 && (!centre || !velocity || !radius)) return GPIS_ERR_ARG;
    if (!std::isfinite(epoch)) return GPIS_ERR_ARG;
    for (int i = 0; i < n * dim; ++i) if (!std::isfinite(centre[i]) || !std::isfinite(velocity[i])) return GPIS_ERR_ARG;
    for (int i = 0; i < n; ++i) if (!std::isfinite(radius[i]) || radius[i] < 0.0) return GPIS_ERR_ARG;
    try { return ((Obstacles*)obst)->set(dim, n, centre, velocity, radius, epoch); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_obst_set_opts(void* obst, const gpis_obst_opts* opts) {
    if (!obst || !opts) return GPIS_ERR_ARG;
    const ObstOpts o = {opts->clearance, opts->margin, opts->w_obs, opts->w_col};
    if (int rc = obst_check_opts(o)) return rc;
    ((Obstacles*)obst)->opts = o;
    return GPIS_OK;
}
int gpis_obst_get(void* obst, double* centre, double* velocity, double* radius, gpis_obst_opts* opts) {
    if (!obst) return GPIS_ERR_ARG;
    const Obstacles& b = *(const Obstacles*)obst;
    for (int i = 0; i < b.n; ++i) {
        for (int a = 0; a < b.dim; ++a) {
            if (centre) centre[(size_t)i * b.dim + a] = b.c[i][a];
            if (velocity) velocity[(size_t)i * b.dim + a] = b.v[i][a];
        }
        if (radius) radius[i] = b.r[i];
    }
    if (opts) { opts->clearance = b.opts.clearance; opts->margin = b.opts.margin; opts->w_obs = b.opts.w_obs; opts->w_col = b.opts.w_col; }
    return GPIS_OK;
}
int gpis_obst_info(void* obst, double* out, int n) {
    if (!obst || !out || n < 0) return GPIS_ERR_ARG;
    const Obstacles& b = *(const Obstacles*)obst;
    const double v[5] = {b.inited ? 1.0 : 0.0, (double)b.dim, (double)b.n, b.epoch, (double)b.device};
    for (int i = 0; i < n && i < 5; ++i) out[i] = v[i];
    return GPIS_OK;
}
int gpis_obst_at(void* obst, double t, double* centre_out) {
    if (!obst || !std::isfinite(t) || (!centre_out && ((const Obstacles*)obst)->n > 0)) return GPIS_ERR_ARG;
    ((const Obstacles*)obst)->at(t, centre_out);
    return GPIS_OK;
}
int gpis_obst_mppi_step(void* mppi, void* df, void* plan, void* obst, double t_now, const double* pose, const double* goal,
                        const gpis_mppi_opts* opts, double* u0, void* stream) {
    return mppi_step_checked(mppi, df, plan, (const Obstacles*)obst, t_now, pose, goal, opts, u0, stream);
}
int gpis_obst_check_timing(void* traj, void* obst, double dt, int steps, double t0, double t_begin, double clearance, double* min_sep,
                           double* min_time, int* min_obstacle, int* first_hit, int* collides) {
    if (!traj || !obst) return GPIS_ERR_ARG;
    if (!std::isfinite(dt) || !std::isfinite(t0) || !std::isfinite(t_begin) || !std::isfinite(clearance)) return GPIS_ERR_ARG;
    if (steps < 1 || steps > 4096 || !(dt > 0.0) || t0 < 0.0 || clearance < 0.0) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    if (!t.has_timing()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try { return t.check_obst(b, dt, steps, t0, t_begin, clearance, min_sep, min_time, min_obstacle, first_hit, collides); }
    catch (...) { return GPIS_ERR_STATE; }
}
// ---- re-timing: schedules that wait for moving balls, and what reads them -------------------------------------------------------
int gpis_retime_default_opts(int dim, float step, gpis_retime_opts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->slot = 0.1; o->max_pause = 63; o->clearance = (double)step; o->press_on = 0;
    return GPIS_OK;
}
// Everything is checked before the previous schedule is dropped; a failure after that leaves the timing without one.
int gpis_retime_solve(void* traj, void* obst, double t_begin, const gpis_retime_opts* opts, void* stream) {
    if (!traj || !obst || !opts || !std::isfinite(t_begin)) return GPIS_ERR_ARG;
    RetimeOpts o;
    o.slot = opts->slot; o.max_pause = opts->max_pause; o.clearance = opts->clearance; o.press_on = opts->press_on;
    if (int rc = retime_check_opts(o)) return rc;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    if (!t.has_timing()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try { return t.retime(b, o, t_begin, (hipStream_t)stream); } catch (...) { t.retimed = false; return GPIS_ERR_STATE; }
}
int gpis_retime_get(void* traj, int* status, int* arrive, int* pauses, int* own_slots, int* first_pause, int* own,
                    gpis_retime_opts* opts, double* info) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    if (!t.has_schedule()) return GPIS_ERR_STATE;
    DeviceScope ds(t.device);
    if (own) {
        GPIS_HIP(hipMemcpyAsync(own, t.d_rown, sizeof(int) * Trajectories::kOwnLen * (size_t)t.m, hipMemcpyDeviceToHost, t.own));
        GPIS_HIP(hipStreamSynchronize(t.own));
    }
    int* outs[5] = {status, arrive, pauses, own_slots, first_pause};
    for (size_t k = 0; k < (size_t)t.m; ++k)
        for (int c = 0; c < 5; ++c)
            if (outs[c]) outs[c][k] = t.h_rres[Trajectories::kSchedRes * k + c];
    if (opts) { opts->slot = t.ropts.slot; opts->max_pause = t.ropts.max_pause; opts->clearance = t.ropts.clearance; opts->press_on = t.ropts.press_on; }
    if (info) { info[0] = t.r_begin; info[1] = t.retime_ms; }
    return GPIS_OK;
}
int gpis_retime_controls(void* traj, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                         int* clamped) {
    if (!traj || k0 < 0 || k0 > (1 << 20)) return GPIS_ERR_ARG;
    if (int rc = timing_check_args(1.0, T, 0.0, w_limit, min_move)) return rc;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.retime_controls(T, k0, w_limit, min_move, U, heading0, p0, clamped); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_retime_follow(void* mppi, void* traj, int index, int k0, double w_limit, double min_move, double* heading0, double* p0) {
    if (!mppi || !traj || k0 < 0 || k0 > (1 << 20)) return GPIS_ERR_ARG;
    Controller& c = *(Controller*)mppi;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.retime_follow(c, index, k0, w_limit, min_move, heading0, p0); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_retime_check(void* traj, void* obst, int steps, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                      int* first_hit, int* collides) {
    if (!traj || !obst) return GPIS_ERR_ARG;
    if (!std::isfinite(clearance) || steps < 1 || steps > 4096 || clearance < 0.0) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    if (!t.has_schedule()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try { return t.retime_check(b, steps, clearance, min_sep, min_time, min_obstacle, first_hit, collides); }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis_obst_mppi_get(void* mppi, int* dyn_hits, double* min_sep, double* stats) {
    if (!mppi) return GPIS_ERR_ARG;
    const Controller& c = *(const Controller*)mppi;
    if (!c.inited) return GPIS_ERR_STATE;
    const size_t k = (size_t)c.K;
    if (c.obst_n > 0) {
        DeviceScope ds(c.device);
        if (dyn_hits) GPIS_HIP(hipMemcpyAsync(dyn_hits, c.d_dyn, sizeof(int) * k, hipMemcpyDeviceToHost, c.own));
        if (min_sep) GPIS_HIP(hipMemcpyAsync(min_sep, c.d_msep, sizeof(double) * k, hipMemcpyDeviceToHost, c.own));
        GPIS_HIP(hipStreamSynchronize(c.own));
    } else {
        for (size_t i = 0; i < k; ++i) { if (dyn_hits) dyn_hits[i] = 0; if (min_sep) min_sep[i] = INFINITY; }
    }
    if (stats) {
        const bool on = c.obst_n > 0;
        stats[0] = on ? (double)c.ostats.ndyn : 0.0; stats[1] = on ? (double)c.ostats.nominal_dyn_hits : 0.0;
        stats[2] = on ? c.ostats.nominal_min_sep : (double)INFINITY; stats[3] = (double)c.obst_n;
    }
    return GPIS_OK;
}

// ---- the robot's footprint ---------------------------------------------------------------------------------------------------
void* gpis_body_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    Footprint* b = new (std::nothrow) Footprint();
    if (b && !b->ok()) { delete b; return nullptr; }
    return b;
}
void gpis_body_destroy(void* body) { delete (Footprint*)body; }
int gpis_body_set(void* body, int dim, int m, const double* offset, const double* radius) {
    if (!body || (dim != 2 && dim != 3) || m < 0) return GPIS_ERR_ARG;
    if (m > Footprint::kMax) return GPIS_ERR_LIMIT;
    if (m > 0 && (!offset || !radius)) return GPIS_ERR_ARG;
    for (int i = 0; i < m * dim; ++i) if (!std::isfinite(offset[i])) return GPIS_ERR_ARG;
    for (int i = 0; i < m; ++i) if (!std::isfinite(radius[i]) || radius[i] < 0.0) return GPIS_ERR_ARG;
    try { return ((Footprint*)body)->set(dim, m, offset, radius); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_body_get(void* body, double* offset, double* radius) {
    if (!body) return GPIS_ERR_ARG;
    const Footprint& b = *(const Footprint*)body;
    for (int j = 0; j < b.m; ++j) {
        if (offset) for (int a = 0; a < b.dim; ++a) offset[(size_t)j * b.dim + a] = b.b[j][a];
        if (radius) radius[j] = b.rho[j];
    }
    return GPIS_OK;
}
int gpis_body_info(void* body, double* out, int n) {
    if (!body || !out || n < 0) return GPIS_ERR_ARG;
    const Footprint& b = *(const Footprint*)body;
    const double v[4] = {b.inited ? 1.0 : 0.0, (double)b.dim, (double)b.m, (double)b.device};
    for (int i = 0; i < n && i < 4; ++i) out[i] = v[i];
    return GPIS_OK;
}
int gpis_body_clearance(void* df, void* body, const double* states, long long n, double clearance, double* D_out, int* ball_out,
                        int* counts, void* stream) {
    if (!df || !body || !states || n < 1 || !std::isfinite(clearance)) return GPIS_ERR_ARG;
    if (n > Footprint::kMaxStates) return GPIS_ERR_LIMIT;
    DistanceField& f = *(DistanceField*)df;
    Footprint& b = *(Footprint*)body;
    if (!f.valid) return GPIS_ERR_STATE;
    if (b.m == 0) return GPIS_ERR_STATE;
    if (b.dim != f.dim || b.device != f.device) return GPIS_ERR_ARG;
    const int ns = f.dim + 2;
    for (long long i = 0; i < n; ++i) {
        const double* S = states + (size_t)i * ns;
        for (int a = 0; a < ns; ++a) if (!std::isfinite(S[a])) return GPIS_ERR_ARG;
        const double nn = std::sqrt(S[f.dim] * S[f.dim] + S[f.dim + 1] * S[f.dim + 1]);
        if (!(nn > 0.0) || !std::isfinite(nn)) return GPIS_ERR_ARG;
    }
    DeviceScope ds(f.device);
    try { return b.clearance(f, states, n, clearance, D_out, ball_out, counts, stream ? (hipStream_t)stream : f.own); }
    catch (...) { return GPIS_ERR_STATE; }
}
int gpis_body_mppi_step(void* mppi, void* df, void* plan, void* body, void* obst, double t_now, const double* pose, const double* goal,
                        const gpis_mppi_opts* opts, double* u0, void* stream) {
    return mppi_step_checked(mppi, df, plan, (const Obstacles*)obst, t_now, pose, goal, opts, u0, stream, (const Footprint*)body);
}
int gpis_body_traj_clearance(void* traj, void* df, void* body, double clearance, double* D_min, int* waypoint, int* ball, int* collides) {
    if (!traj || !df || !body || !std::isfinite(clearance)) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const DistanceField& f = *(const DistanceField*)df;
    const Footprint& b = *(const Footprint*)body;
    if (!t.valid || !f.valid || b.m == 0) return GPIS_ERR_STATE;
    if (f.dim != t.dim || f.device != t.device || b.dim != t.dim || b.device != t.device) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try { return t.check_body(f, BodyArgs{b.d_tab, b.m}, clearance, D_min, waypoint, ball, collides); }
    catch (...) { return GPIS_ERR_STATE; }
}

// ---- the footprint against moving balls: the timed check, the re-timing and its check ------------------------------------------
// what every timed entry with a footprint refuses before anything else: no body, an empty one, one of another dim or device
static int body_time_args(const Trajectories& t, const Footprint* b) {
    if (!b || b->m == 0) return GPIS_ERR_ARG;
    if (t.valid && (b->dim != t.dim || b->device != t.device)) return GPIS_ERR_ARG;
    return GPIS_OK;
}
int gpis_timed_body_check(void* traj, void* obst, void* body, double dt, int steps, double t0, double t_begin, double clearance,
                           double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides) {
    if (!traj || !obst || !body) return GPIS_ERR_ARG;
    if (!std::isfinite(dt) || !std::isfinite(t0) || !std::isfinite(t_begin) || !std::isfinite(clearance)) return GPIS_ERR_ARG;
    if (steps < 1 || steps > 4096 || !(dt > 0.0) || t0 < 0.0 || clearance < 0.0) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    const Footprint& f = *(const Footprint*)body;
    if (int rc = body_time_args(t, &f)) return rc;
    if (!t.has_timing()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try {
        return t.check_body_obst(b, BodyArgs{f.d_tab, f.m}, dt, steps, t0, t_begin, clearance, min_sep, min_time, min_obstacle, min_ball,
                                 first_hit, collides);
    } catch (...) { return GPIS_ERR_STATE; }
}
// Everything is checked before the previous schedule is dropped; a failure after that leaves the timing without one.
int gpis_timed_body_retime(void* traj, void* obst, void* body, double t_begin, const gpis_retime_opts* opts, void* stream) {
    if (!traj || !obst || !body || !opts || !std::isfinite(t_begin)) return GPIS_ERR_ARG;
    RetimeOpts o;
    o.slot = opts->slot; o.max_pause = opts->max_pause; o.clearance = opts->clearance; o.press_on = opts->press_on;
    if (int rc = retime_check_opts(o)) return rc;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    const Footprint& f = *(const Footprint*)body;
    if (int rc = body_time_args(t, &f)) return rc;
    if (!t.has_timing()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try { return t.retime_body(b, BodyArgs{f.d_tab, f.m}, o, t_begin, (hipStream_t)stream); }
    catch (...) { t.retimed = false; return GPIS_ERR_STATE; }
}
int gpis_timed_body_info(void* traj, double* out, int n) {
    if (!traj || !out || n < 0) return GPIS_ERR_ARG;
    const Trajectories& t = *(const Trajectories*)traj;
    if (!t.has_schedule()) return GPIS_ERR_STATE;
    const double v[1] = {(double)t.r_body};
    for (int i = 0; i < n && i < 1; ++i) out[i] = v[i];
    return GPIS_OK;
}
int gpis_timed_body_retime_check(void* traj, void* obst, void* body, int steps, double clearance, double* min_sep, double* min_time,
                           int* min_obstacle, int* min_ball, int* first_hit, int* collides) {
    if (!traj || !obst || !body) return GPIS_ERR_ARG;
    if (!std::isfinite(clearance) || steps < 1 || steps > 4096 || clearance < 0.0) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const Obstacles& b = *(const Obstacles*)obst;
    const Footprint& f = *(const Footprint*)body;
    if (int rc = body_time_args(t, &f)) return rc;
    if (!t.has_schedule()) return GPIS_ERR_STATE;
    if (b.device != t.device || (b.inited && b.dim != t.dim)) return GPIS_ERR_ARG;
    DeviceScope ds(t.device);
    try {
        return t.retime_body_check(b, BodyArgs{f.d_tab, f.m}, steps, clearance, min_sep, min_time, min_obstacle, min_ball, first_hit,
                                   collides);
    } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_timed_body_states(void* traj, double dt, int steps, double t0, int retimed, double* states_out) {
    if (!traj || !states_out || (retimed != 0 && retimed != 1)) return GPIS_ERR_ARG;
    if (steps < 1 || steps > 4096) return GPIS_ERR_ARG;
    if (!retimed && (!std::isfinite(dt) || !std::isfinite(t0) || !(dt > 0.0) || t0 < 0.0)) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    DeviceScope ds(t.device);
    try { return t.timed_states(dt, steps, t0, retimed != 0, states_out); } catch (...) { return GPIS_ERR_STATE; }
}

// ---- smoothing for the robot's footprint ---------------------------------------------------------------------------------------
int gpis_smooth_body_default_opts(int dim, float step, int balls, gpis_traj_opts* o, float* w_turn) {
    if (balls < 1 || balls > Footprint::kMax) return GPIS_ERR_ARG;
    if (int rc = gpis_traj_default_opts(dim, step, o)) return rc;
    o->w_obs = (0.25f * step) / (float)balls;
    if (w_turn) *w_turn = 1.f;
    return GPIS_OK;
}
int gpis_smooth_body_optimize(void* traj, void* d, void* body, const gpis_traj_opts* opts, float w_turn, void* stream) {
    if (!traj || !d || !body) return GPIS_ERR_ARG;
    if (!std::isfinite(w_turn) || w_turn < 0.f) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const DistanceField& df = *(const DistanceField*)d;
    const Footprint& b = *(const Footprint*)body;
    if (b.m == 0) return GPIS_ERR_ARG;
    gpis_traj_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_smooth_body_default_opts(df.dim, df.step, b.m, &dflt, nullptr);
        opts = &dflt;
    }
    TrajOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.w_smooth = opts->w_smooth; o.w_obs = opts->w_obs; o.rate = opts->rate;
    o.max_move = opts->max_move; o.tol = opts->tol; o.iters = opts->iters; o.sub = opts->sub;
    if (int rc = traj_check_opts(o)) return rc;
    if (!df.valid || !t.has_input) return GPIS_ERR_STATE;
    if (b.dim != df.dim || df.dim != t.dim || b.device != df.device) return GPIS_ERR_ARG;
    const BodyArgs bd{b.d_tab, b.m};
    DeviceScope ds(df.device);
    try { return t.optimize(df, o, stream ? (hipStream_t)stream : df.own, &bd, w_turn); }
    catch (...) { t.valid = t.body_valid = false; return GPIS_ERR_STATE; }
}
int gpis_smooth_body_get(void* traj, double* D_min, int* waypoint, int* ball, int* collides) {
    if (!traj) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    if (!t.valid || !t.body_valid) return GPIS_ERR_STATE;
    DeviceScope ds(t.device);
    try { return t.body_result(D_min, waypoint, ball, collides); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_smooth_from_pose_paths(void* traj, void* pplan, int N) {
    if (!traj || !pplan) return GPIS_ERR_ARG;
    Trajectories& t = *(Trajectories*)traj;
    const PosePlanner& p = *(const PosePlanner*)pplan;
    DeviceScope ds(p.device);
    try { return t.from_pose_paths(p, N); } catch (...) { t.has_input = t.valid = t.body_valid = false; return GPIS_ERR_STATE; }
}

// ---- routes for the robot's footprint: the pose planner ------------------------------------------------------------------------
int gpis_pplan_default_opts(float step, int H, gpis_pplan_opts* o) {
    if (!o || !(std::isfinite(step) && step > 0.f) || (H != 8 && H != 16 && H != 32 && H != 64)) return GPIS_ERR_ARG;
    o->clearance = 0.f; o->margin = 4.f * step; o->gain = 4.f; o->turn = step; o->max_rounds = 0;
    return GPIS_OK;
}
void* gpis_pplan_create(void) {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    PosePlanner* p = new (std::nothrow) PosePlanner();
    if (p && !p->own) { delete p; return nullptr; }
    return p;
}
void gpis_pplan_destroy(void* pplan) { delete (PosePlanner*)pplan; }
int gpis_pplan_set_schedule(void* pplan, int check_every, int inner_cap) {
    if (!pplan || check_every < 0 || inner_cap < 0) return GPIS_ERR_ARG;
    ((PosePlanner*)pplan)->sched.set(check_every, inner_cap);
    return GPIS_OK;
}
// a heading index of a goal or a start: an integer in -1 .. H - 1
static bool pplan_heading_ok(float h, int H) { return std::isfinite(h) && h == std::floor(h) && h >= -1.f && h <= (float)(H - 1); }
// the argument and state checks come before anything is dropped: such an error leaves the previous result readable
int gpis_pplan_solve(void* pplan, void* d, void* body, const double* headings, const unsigned short* moves, int H, const float* goals,
                     int ngoals, const gpis_pplan_opts* opts, void* stream) {
    if (!pplan || !d || !body || !headings || !moves || !goals || ngoals < 1) return GPIS_ERR_ARG;
    if (H != 8 && H != 16 && H != 32 && H != 64) return GPIS_ERR_ARG;
    for (int h = 0; h < H; ++h) {
        const double c = headings[2 * h], s = headings[2 * h + 1];
        if (!std::isfinite(c) || !std::isfinite(s) || (c == 0.0 && s == 0.0) || (moves[h] & ~0x1efu)) return GPIS_ERR_ARG;
    }
    for (int g = 0; g < ngoals; ++g) if (!pplan_heading_ok(goals[(size_t)g * 3 + 2], H)) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    const Footprint& b = *(const Footprint*)body;
    if (df.valid && df.dim != 2) return GPIS_ERR_ARG;
    gpis_pplan_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_pplan_default_opts(df.step, H, &dflt);
        opts = &dflt;
    }
    PPlanOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.gain = opts->gain; o.turn = opts->turn; o.max_rounds = opts->max_rounds;
    if (int rc = pplan_check_opts(o, df.valid ? df.step : 0.f)) return rc;
    if (!df.valid || b.m == 0 || b.dim != 2) return GPIS_ERR_STATE;
    if (b.device != df.device) return GPIS_ERR_ARG;
    if ((long long)df.n[0] * df.n[1] * H > PosePlanner::kMaxStates) return GPIS_ERR_LIMIT;
    PosePlanner& p = *(PosePlanner*)pplan;
    DeviceScope ds(df.device);
    try {
        if (int rc = p.bind(df.device)) { p.clear_result(); return rc; }
        const int rc = p.solve(df, b, headings, moves, H, goals, ngoals, o, stream ? (hipStream_t)stream : df.own);
        if (rc != GPIS_OK) p.clear_result();
        return rc;
    } catch (...) { p.clear_result(); return GPIS_ERR_STATE; }
}
int gpis_pplan_info(void* pplan, double* out, int n) {
    if (!pplan || !out || n < 0) return GPIS_ERR_ARG;
    const PosePlanner& p = *(PosePlanner*)pplan;
    const bool v = p.valid;
    const PlanCounters& c = p.cnt;
    const double w[14] = {v ? 1.0 : 0.0, v ? (double)p.n[0] : 0.0, v ? (double)p.n[1] : 0.0, v ? (double)p.H : 0.0, v ? (double)p.step : 0.0,
                          (double)c.goals_given, (double)c.goals_kept, (double)c.nfree, (double)c.nreach, (double)c.rounds,
                          (double)c.launches, c.solve_ms, (double)c.max_cost, p.setup_ms};
    for (int i = 0; i < n && i < 14; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_pplan_get(void* pplan, float* cost, unsigned char* policy, float* c) {
    if (!pplan) return GPIS_ERR_ARG;
    PosePlanner& p = *(PosePlanner*)pplan;
    if (!p.valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t n = (size_t)p.nstates;
    if (cost) GPIS_HIP(hipMemcpyAsync(cost, p.d_cost, sizeof(float) * n, hipMemcpyDeviceToHost, p.own));
    if (policy) GPIS_HIP(hipMemcpyAsync(policy, p.d_policy, n, hipMemcpyDeviceToHost, p.own));
    if (c) GPIS_HIP(hipMemcpyAsync(c, p.d_c, sizeof(float) * n, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    return GPIS_OK;
}
int gpis_pplan_device(void* pplan, const float** d_cost, const unsigned char** d_policy, const float** d_c) {
    if (!pplan) return GPIS_ERR_ARG;
    const PosePlanner& p = *(PosePlanner*)pplan;
    if (d_cost) *d_cost = p.valid ? p.d_cost : nullptr;
    if (d_policy) *d_policy = p.valid ? p.d_policy : nullptr;
    if (d_c) *d_c = p.valid ? p.d_c : nullptr;
    return GPIS_OK;
}
int gpis_pplan_paths(void* pplan, const float* starts, int m, int max_points, void* stream) {
    if (!pplan || !starts || m < 1 || max_points < 2) return GPIS_ERR_ARG;
    PosePlanner& p = *(PosePlanner*)pplan;
    if (!p.valid) return GPIS_ERR_STATE;
    if (m > PosePlanner::kMaxStarts) return GPIS_ERR_LIMIT;
    for (int t = 0; t < m; ++t) if (!pplan_heading_ok(starts[(size_t)t * 3 + 2], p.H)) return GPIS_ERR_ARG;
    DeviceScope ds(p.device);
    try {
        const int rc = p.paths(starts, m, max_points, stream ? (hipStream_t)stream : p.own);
        if (rc != GPIS_OK) p.paths_valid = false;
        return rc;
    } catch (...) { p.paths_valid = false; return GPIS_ERR_STATE; }
}
int gpis_pplan_path_counts(void* pplan, long long* npaths, long long* npoints) {
    if (!pplan) return GPIS_ERR_ARG;
    const PosePlanner& p = *(PosePlanner*)pplan;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (npaths) *npaths = p.npaths;
    if (npoints) *npoints = p.npoints;
    return GPIS_OK;
}
int gpis_pplan_get_paths(void* pplan, long long* off, float* points, int* heading, float* start_cost, unsigned char* status) {
    if (!pplan) return GPIS_ERR_ARG;
    PosePlanner& p = *(PosePlanner*)pplan;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t m = (size_t)p.npaths;
    if (off) GPIS_HIP(hipMemcpyAsync(off, p.d_off, sizeof(long long) * (m + 1), hipMemcpyDeviceToHost, p.own));
    if (points && p.npoints > 0) GPIS_HIP(hipMemcpyAsync(points, p.d_points, sizeof(float) * 2 * (size_t)p.npoints, hipMemcpyDeviceToHost, p.own));
    if (heading && p.npoints > 0) GPIS_HIP(hipMemcpyAsync(heading, p.d_pheading, sizeof(int) * (size_t)p.npoints, hipMemcpyDeviceToHost, p.own));
    if (start_cost) GPIS_HIP(hipMemcpyAsync(start_cost, p.d_scost, sizeof(float) * m, hipMemcpyDeviceToHost, p.own));
    if (status) GPIS_HIP(hipMemcpyAsync(status, p.d_status, m, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    return GPIS_OK;
}
int gpis_pplan_project(void* pplan, void* plan, unsigned char* heading2) {
    if (!pplan || !plan) return GPIS_ERR_ARG;
    PosePlanner& p = *(PosePlanner*)pplan;
    if (!p.valid) return GPIS_ERR_STATE;
    Planner& q = *(Planner*)plan;
    DeviceScope ds(p.device);
    try {
        const int rc = p.project(q, heading2);
        if (rc != GPIS_OK) q.clear_result();
        return rc;
    } catch (...) { q.clear_result(); return GPIS_ERR_STATE; }
}

// ---- planning through space and time: what gpis_tplan_* and gpis_tpplan_* share, over the handle type -------------------------------
}  // extern "C"

namespace {

template <class P>
int tp_check_size(long long states, int horizon, int keep_cost) {
    return states * (long long)(horizon + 1) > (keep_cost ? P::kMaxStatesKept : P::kMaxStates) ? GPIS_ERR_LIMIT : GPIS_OK;
}
template <class P>
void* tp_create() {
    if (gpis_device_count() < 1) { fprintf(stderr, "[gpismap_amd] no HIP device\n"); return nullptr; }
    P* p = new (std::nothrow) P();
    if (p && !p->own) { delete p; return nullptr; }
    return p;
}
// bind to the field's device and solve; whatever fails, the handle holds no result afterwards
template <class P, class Solve>
int tp_solve(P& p, int device, Solve solve) {
    DeviceScope ds(device);
    try {
        if (int rc = p.bind(device)) { p.clear_result(); return rc; }
        const int rc = solve();
        if (rc != GPIS_OK) p.clear_result();
        return rc;
    } catch (...) { p.clear_result(); return GPIS_ERR_STATE; }
}
template <class P>
int tp_get(void* h, float* cost0, unsigned char* policy, float* cost_all, float* c) {
    if (!h) return GPIS_ERR_ARG;
    P& p = *(P*)h;
    if (!p.valid || (cost_all && !p.kept)) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t n = (size_t)p.ns, ns = n * (size_t)(p.S + 1);
    if (cost0) GPIS_HIP(hipMemcpyAsync(cost0, p.d_cost0, sizeof(float) * n, hipMemcpyDeviceToHost, p.own));
    if (policy) GPIS_HIP(hipMemcpyAsync(policy, p.d_policy, ns, hipMemcpyDeviceToHost, p.own));
    if (cost_all) GPIS_HIP(hipMemcpyAsync(cost_all, p.d_all, sizeof(float) * ns, hipMemcpyDeviceToHost, p.own));
    if (c) GPIS_HIP(hipMemcpyAsync(c, p.d_c, sizeof(float) * n, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    return GPIS_OK;
}
// the checks of a paths call that do not look at the starts' values
template <class P>
int tp_paths_args(void* h, const float* starts, int m) {
    if (!h || !starts || m < 1) return GPIS_ERR_ARG;
    if (!((P*)h)->valid) return GPIS_ERR_STATE;
    return m > P::kMaxStarts ? GPIS_ERR_LIMIT : GPIS_OK;
}
template <class P>
int tp_paths(P& p, const float* starts, int m, void* stream) {
    DeviceScope ds(p.device);
    try {
        const int rc = p.paths(starts, m, stream ? (hipStream_t)stream : p.own);
        if (rc != GPIS_OK) p.paths_valid = false;
        return rc;
    } catch (...) { p.paths_valid = false; return GPIS_ERR_STATE; }
}
template <class P>
int tp_path_counts(void* h, long long* npaths, long long* npoints) {
    if (!h) return GPIS_ERR_ARG;
    const P& p = *(P*)h;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (npaths) *npaths = p.npaths;
    if (npoints) *npoints = p.npoints;
    return GPIS_OK;
}
// d_heading: the handle's device buffer of a heading index per point, where it has one (heading: host [npoints] or null)
template <class P>
int tp_get_paths(void* h, long long* off, float* points, int* heading, const int* d_heading, int* arrive, float* start_cost,
                 unsigned char* status) {
    if (!h) return GPIS_ERR_ARG;
    P& p = *(P*)h;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    const size_t m = (size_t)p.npaths;
    std::vector<long long> ho(m + 1);
    std::vector<unsigned char> hs(m);
    GPIS_HIP(hipMemcpyAsync(ho.data(), p.d_off, sizeof(long long) * (m + 1), hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipMemcpyAsync(hs.data(), p.d_status, m, hipMemcpyDeviceToHost, p.own));
    if (points && p.npoints > 0)
        GPIS_HIP(hipMemcpyAsync(points, p.d_points, sizeof(float) * (size_t)p.npoints * 2, hipMemcpyDeviceToHost, p.own));
    if (heading && d_heading && p.npoints > 0)
        GPIS_HIP(hipMemcpyAsync(heading, d_heading, sizeof(int) * (size_t)p.npoints, hipMemcpyDeviceToHost, p.own));
    if (start_cost) GPIS_HIP(hipMemcpyAsync(start_cost, p.d_scost, sizeof(float) * m, hipMemcpyDeviceToHost, p.own));
    GPIS_HIP(hipStreamSynchronize(p.own));
    for (size_t k = 0; k < m; ++k) {
        if (off) off[k] = ho[k];
        if (status) status[k] = hs[k];
        if (arrive) arrive[k] = hs[k] == 0 ? (int)(ho[k + 1] - ho[k]) - 1 : -1;
    }
    if (off) off[m] = ho[m];
    return GPIS_OK;
}
template <class P>
int tp_controls(void* h, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    if (!h || k0 < 0 || k0 > (1 << 20) || T < 1 || T > P::kMaxT) return GPIS_ERR_ARG;
    if (!std::isfinite(w_limit) || !std::isfinite(min_move) || w_limit < 0.0 || min_move < 0.0) return GPIS_ERR_ARG;
    P& p = *(P*)h;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    DeviceScope ds(p.device);
    try { return p.controls(T, k0, w_limit, min_move, U, heading0, p0, clamped); } catch (...) { return GPIS_ERR_STATE; }
}

}  // namespace

extern "C" {

// ---- planning through space and time around moving balls -----------------------------------------------------------------------
int gpis_tplan_default_opts(float step, gpis_tplan_opts* o) {
    if (!o || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->clearance = 0.f; o->margin = 4.f * step; o->gain = 4.f; o->connectivity = 1;
    o->slot = 0.1; o->horizon = 256; o->dyn_clearance = (double)step; o->wait = 0.5f; o->keep_cost = 0;
    return GPIS_OK;
}
static TimePlanOpts tplan_opts_of(const gpis_tplan_opts* opts) {
    TimePlanOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.gain = opts->gain; o.connectivity = opts->connectivity;
    o.slot = opts->slot; o.horizon = opts->horizon; o.dyn_clearance = opts->dyn_clearance; o.wait = opts->wait;
    o.keep_cost = opts->keep_cost;
    return o;
}
int gpis_tplan_check_opts(const gpis_tplan_opts* opts, int nx, int ny) {
    if (!opts || nx < 0 || ny < 0) return GPIS_ERR_ARG;
    const TimePlanOpts o = tplan_opts_of(opts);
    if (int rc = tplan_check_opts(o)) return rc;
    return tp_check_size<TimePlanner>((long long)nx * ny, o.horizon, o.keep_cost);
}
void* gpis_tplan_create(void) { return tp_create<TimePlanner>(); }
void gpis_tplan_destroy(void* tplan) { delete (TimePlanner*)tplan; }
int gpis_tplan_set_schedule(void* tplan, int layers_per_launch, int cull) {
    if (!tplan || layers_per_launch < 0 || layers_per_launch > TimePlanner::kMaxLayers || (cull != 0 && cull != 1)) return GPIS_ERR_ARG;
    TimePlanner& p = *(TimePlanner*)tplan;
    p.layers_per_launch = layers_per_launch;
    p.cull = cull;
    return GPIS_OK;
}
// every check comes before anything is written: such an error leaves the previous result readable
int gpis_tplan_solve(void* tplan, void* d, void* obst, const float* goals, int ngoals, double t_begin, const gpis_tplan_opts* opts,
                     void* stream) {
    if (!tplan || !d || !goals || ngoals < 1 || !std::isfinite(t_begin)) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    gpis_tplan_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_tplan_default_opts(df.step, &dflt);
        opts = &dflt;
    }
    const TimePlanOpts o = tplan_opts_of(opts);
    if (int rc = tplan_check_opts(o)) return rc;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != 2) return GPIS_ERR_ARG;
    const Obstacles* ob = (const Obstacles*)obst;
    if (ob && (ob->device != df.device || (ob->inited && ob->n > 0 && ob->dim != 2))) return GPIS_ERR_ARG;
    if (int rc = tp_check_size<TimePlanner>(df.ngrid, o.horizon, o.keep_cost)) return rc;
    TimePlanner& p = *(TimePlanner*)tplan;
    return tp_solve(p, df.device, [&] { return p.solve(df, ob, goals, ngoals, t_begin, o, stream ? (hipStream_t)stream : df.own); });
}
int gpis_tplan_info(void* tplan, double* out, int n) {
    if (!tplan || !out || n < 0) return GPIS_ERR_ARG;
    const TimePlanner& p = *(TimePlanner*)tplan;
    const bool v = p.valid;
    const double w[16] = {v ? 1.0 : 0.0, v ? (double)p.nx : 0.0, v ? (double)p.ny : 0.0, v ? (double)p.S : 0.0, v ? p.opts.slot : 0.0,
                          (double)p.n, (double)p.goals_given, (double)p.goals_kept, (double)p.nfree, (double)p.nfinite,
                          (double)p.launches, (double)p.skipped, p.solve_ms, (double)p.max_cost0, p.t_begin, p.kept ? 1.0 : 0.0};
    for (int i = 0; i < n && i < 16; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_tplan_get(void* tplan, float* cost0, unsigned char* policy, float* cost_all, float* c) {
    return tp_get<TimePlanner>(tplan, cost0, policy, cost_all, c);
}
int gpis_tplan_device(void* tplan, const float** d_cost0, const unsigned char** d_policy) {
    if (!tplan) return GPIS_ERR_ARG;
    const TimePlanner& p = *(TimePlanner*)tplan;
    if (d_cost0) *d_cost0 = p.valid ? p.d_cost0 : nullptr;
    if (d_policy) *d_policy = p.valid ? p.d_policy : nullptr;
    return GPIS_OK;
}
int gpis_tplan_paths(void* tplan, const float* starts, int m, void* stream) {
    if (int rc = tp_paths_args<TimePlanner>(tplan, starts, m)) return rc;
    return tp_paths(*(TimePlanner*)tplan, starts, m, stream);
}
int gpis_tplan_path_counts(void* tplan, long long* npaths, long long* npoints) { return tp_path_counts<TimePlanner>(tplan, npaths, npoints); }
int gpis_tplan_get_paths(void* tplan, long long* off, float* points, int* arrive, float* start_cost, unsigned char* status) {
    return tp_get_paths<TimePlanner>(tplan, off, points, nullptr, nullptr, arrive, start_cost, status);
}
int gpis_tplan_check(void* tplan, void* obst, double clearance, double* min_sep, double* min_time, int* min_obstacle, int* first_hit,
                     int* collides) {
    if (!tplan || !obst || !std::isfinite(clearance) || clearance < 0.0) return GPIS_ERR_ARG;
    TimePlanner& p = *(TimePlanner*)tplan;
    const Obstacles& b = *(const Obstacles*)obst;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (b.device != p.device || (b.inited && b.n > 0 && b.dim != 2)) return GPIS_ERR_ARG;
    DeviceScope ds(p.device);
    try { return p.check(b, clearance, min_sep, min_time, min_obstacle, first_hit, collides); } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_tplan_controls(void* tplan, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                        int* clamped) {
    return tp_controls<TimePlanner>(tplan, T, k0, w_limit, min_move, U, heading0, p0, clamped);
}

// ---- planning through space and time for the robot's footprint ------------------------------------------------------------------
static bool tpplan_h_ok(int H) { return H == 8 || H == 16 || H == 32 || H == 64; }
int gpis_tpplan_default_opts(float step, int H, gpis_tpplan_opts* o) {
    if (!o || !(std::isfinite(step) && step > 0.f) || !tpplan_h_ok(H)) return GPIS_ERR_ARG;
    o->clearance = 0.f; o->margin = 4.f * step; o->gain = 4.f; o->turn = step;
    o->slot = 0.1; o->horizon = 256; o->dyn_clearance = (double)step; o->wait = 0.5f; o->keep_cost = 0;
    return GPIS_OK;
}
static TimePosePlanOpts tpplan_opts_of(const gpis_tpplan_opts* opts) {
    TimePosePlanOpts o;
    o.clearance = opts->clearance; o.margin = opts->margin; o.gain = opts->gain; o.turn = opts->turn;
    o.slot = opts->slot; o.horizon = opts->horizon; o.dyn_clearance = opts->dyn_clearance; o.wait = opts->wait;
    o.keep_cost = opts->keep_cost;
    return o;
}
int gpis_tpplan_check_opts(const gpis_tpplan_opts* opts, int H, int nx, int ny) {
    if (!opts || !tpplan_h_ok(H) || nx < 0 || ny < 0) return GPIS_ERR_ARG;
    const TimePosePlanOpts o = tpplan_opts_of(opts);
    if (int rc = tpplan_check_opts(o, 0.f)) return rc;
    return tp_check_size<TimePosePlanner>((long long)nx * ny * H, o.horizon, o.keep_cost);
}
void* gpis_tpplan_create(void) { return tp_create<TimePosePlanner>(); }
void gpis_tpplan_destroy(void* tpp) { delete (TimePosePlanner*)tpp; }
int gpis_tpplan_set_schedule(void* tpp, int cull) {
    if (!tpp || (cull != 0 && cull != 1)) return GPIS_ERR_ARG;
    ((TimePosePlanner*)tpp)->cull = cull;
    return GPIS_OK;
}
// every check comes before anything is written: such an error leaves the previous result readable
int gpis_tpplan_solve(void* tpp, void* d, void* obst, void* body, const double* headings, const unsigned short* moves, int H,
                      const float* goals, int ngoals, double t_begin, const gpis_tpplan_opts* opts, void* stream) {
    if (!tpp || !d || !body || !headings || !moves || !goals || ngoals < 1 || !std::isfinite(t_begin)) return GPIS_ERR_ARG;
    if (!tpplan_h_ok(H)) return GPIS_ERR_ARG;
    for (int h = 0; h < H; ++h) {
        const double c = headings[2 * h], s = headings[2 * h + 1];
        if (!std::isfinite(c) || !std::isfinite(s) || (c == 0.0 && s == 0.0) || (moves[h] & ~0x1efu)) return GPIS_ERR_ARG;
    }
    for (int g = 0; g < ngoals; ++g) if (!pplan_heading_ok(goals[(size_t)g * 3 + 2], H)) return GPIS_ERR_ARG;
    const DistanceField& df = *(const DistanceField*)d;
    const Footprint& b = *(const Footprint*)body;
    if (df.valid && df.dim != 2) return GPIS_ERR_ARG;
    gpis_tpplan_opts dflt;
    if (!opts) {
        if (!df.valid) return GPIS_ERR_STATE;
        (void)gpis_tpplan_default_opts(df.step, H, &dflt);
        opts = &dflt;
    }
    const TimePosePlanOpts o = tpplan_opts_of(opts);
    if (int rc = tpplan_check_opts(o, df.valid ? df.step : 0.f)) return rc;
    if (!df.valid || b.m == 0 || b.dim != 2) return GPIS_ERR_STATE;
    if (b.device != df.device) return GPIS_ERR_ARG;
    const Obstacles* ob = (const Obstacles*)obst;
    if (ob && (ob->device != df.device || (ob->inited && ob->n > 0 && ob->dim != 2))) return GPIS_ERR_ARG;
    if (int rc = tp_check_size<TimePosePlanner>(df.ngrid * H, o.horizon, o.keep_cost)) return rc;
    TimePosePlanner& p = *(TimePosePlanner*)tpp;
    return tp_solve(p, df.device, [&] {
        return p.solve(df, ob, b, headings, moves, H, goals, ngoals, t_begin, o, stream ? (hipStream_t)stream : df.own);
    });
}
int gpis_tpplan_info(void* tpp, double* out, int n) {
    if (!tpp || !out || n < 0) return GPIS_ERR_ARG;
    const TimePosePlanner& p = *(TimePosePlanner*)tpp;
    const bool v = p.valid;
    const double w[18] = {v ? 1.0 : 0.0, v ? (double)p.nx : 0.0, v ? (double)p.ny : 0.0, v ? (double)p.H : 0.0, v ? (double)p.S : 0.0,
                          v ? p.opts.slot : 0.0, (double)p.n, (double)p.mb, (double)p.goals_given, (double)p.goals_kept, (double)p.nfree,
                          (double)p.nfinite, (double)p.max_cost0, p.t_begin, p.kept ? 1.0 : 0.0, (double)p.launches, (double)p.skipped,
                          p.solve_ms};
    for (int i = 0; i < n && i < 18; ++i) out[i] = w[i];
    return GPIS_OK;
}
int gpis_tpplan_get(void* tpp, float* cost0, unsigned char* policy, float* cost_all, float* c) {
    return tp_get<TimePosePlanner>(tpp, cost0, policy, cost_all, c);
}
int gpis_tpplan_paths(void* tpp, const float* starts, int m, void* stream) {
    if (int rc = tp_paths_args<TimePosePlanner>(tpp, starts, m)) return rc;
    TimePosePlanner& p = *(TimePosePlanner*)tpp;
    for (int t = 0; t < m; ++t) if (!pplan_heading_ok(starts[(size_t)t * 3 + 2], p.H)) return GPIS_ERR_ARG;
    return tp_paths(p, starts, m, stream);
}
int gpis_tpplan_path_counts(void* tpp, long long* npaths, long long* npoints) { return tp_path_counts<TimePosePlanner>(tpp, npaths, npoints); }
int gpis_tpplan_get_paths(void* tpp, long long* off, float* points, int* heading, int* arrive, float* start_cost, unsigned char* status) {
    return tp_get_paths<TimePosePlanner>(tpp, off, points, heading, tpp ? ((TimePosePlanner*)tpp)->d_pheading : nullptr, arrive, start_cost, status);
}
int gpis_tpplan_check(void* tpp, void* obst, void* body, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                      int* min_ball, int* first_hit, int* collides) {
    if (!tpp || !obst || !std::isfinite(clearance) || clearance < 0.0) return GPIS_ERR_ARG;
    TimePosePlanner& p = *(TimePosePlanner*)tpp;
    const Obstacles& b = *(const Obstacles*)obst;
    const Footprint* f = (const Footprint*)body;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (b.device != p.device || (b.inited && b.n > 0 && b.dim != 2)) return GPIS_ERR_ARG;
    if (f && (f->m == 0 || f->dim != 2)) return GPIS_ERR_STATE;
    if (f && f->device != p.device) return GPIS_ERR_ARG;
    DeviceScope ds(p.device);
    try {
        return p.check(b, f, clearance, min_sep, min_time, min_obstacle, min_ball, first_hit, collides);
    } catch (...) { return GPIS_ERR_STATE; }
}
int gpis_tpplan_controls(void* tpp, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    return tp_controls<TimePosePlanner>(tpp, T, k0, w_limit, min_move, U, heading0, p0, clamped);
}

}  // extern "C"
