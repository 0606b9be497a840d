// Ray-marching renderer (render.h).  Memory-bound passes of a few bytes per ray: grid-stride loops over at most
// kGridCap blocks of 256 threads (cdna_hip_programming.md Guideline 11); the compaction is a three-kernel exclusive scan of one
// byte flag per entry over contiguous per-block segments (ballot ranks inside a block), so it keeps the order of the list.
//
// Ray k of a 3-D render is pixel (col, row) = (k / height, k % height), update()'s column-major layout; u = ((float)col - cx) / fx,
// v = ((float)row - cy) / fy; the parameter is the depth z; the world point R[i] (u z) + R[3+i] (v z) + R[6+i] z + t[i] left to
// right (no FMA: -ffp-contract=off), update()'s expression.  A 2-D ray is a beam with host-double (c, s): local point
// ((float)(r c) + off0, (float)(r s) + off1), world R local + t; the parameter is the range r.
#include <algorithm>
#include <chrono>
#include <cmath>
#include "dfield.h"
#include "map_query.h"
#include "render.h"
#include "block_ops.h"
#include "field_march.h"

namespace gpis {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlocks = kCompactBlocks;   // compaction segments (one thread each in the top scan)
constexpr uint8_t kRunning = kRayRunning;

__device__ __forceinline__ void world_point(const RayGeom& g, const float* __restrict__ ray, const double* __restrict__ cs, int i,
                                            float z, float& p0, float& p1, float& p2) {
    if (g.dim == 3) world_point_at(g, ray[4 * (size_t)i], ray[4 * (size_t)i + 1], 0.0, 0.0, z, p0, p1, p2);
    else world_point_at(g, 0.f, 0.f, cs[2 * (size_t)i], cs[2 * (size_t)i + 1], z, p0, p1, p2);
}

// Per ray: ray_setup's direction terms and clip, the march state, NaN outputs.  flag = 1 for the rays whose clipped interval is
// not empty.
__global__ void __launch_bounds__(kBlock) render_setup_kernel(RayGeom g, const double* __restrict__ cs, int n, bool empty, float tnear,
                                                              float tfar, float lx, float ly, float lz, float hx, float hy, float hz,
                                                              float* __restrict__ ray, float* __restrict__ z, float* __restrict__ zend,
                                                              int* __restrict__ nstep, uint8_t* __restrict__ state,
                                                              uint8_t* __restrict__ status, uint8_t* __restrict__ flag,
                                                              float* __restrict__ depth, float* __restrict__ rec) {
    const int nc = 2 * (1 + g.dim);
    const float lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float u, v, il, t0, t1;
        double cd, sd;
        ray_setup(g, cs, i, tnear, tfar, lo, hi, u, v, il, cd, sd, t0, t1);
        if (g.dim == 3) { ray[4 * (size_t)i] = u; ray[4 * (size_t)i + 1] = v; ray[4 * (size_t)i + 2] = il; ray[4 * (size_t)i + 3] = 0.f; }
        const bool go = !empty && t0 <= t1;
        z[i] = t0; zend[i] = t1; nstep[i] = 0; state[i] = 0;
        status[i] = go ? kRunning : 1;
        flag[i] = go ? 1 : 0;
        depth[i] = __int_as_float(0x7fc00000);
        for (int c = 0; c < nc; ++c) rec[(size_t)i * nc + c] = __int_as_float(0x7fc00000);
    }
}

// Positions of the listed rays and their pre-filled records (f = NaN, zeros elsewhere).  mode 0: the march sample z; 1: the
// bracket's midpoint lo + (hi - lo) * 0.5; 2: the secant point of the bracket, clamped into it (hi when g(lo) is NaN).  Modes 1, 2
// keep the parameter in q.
__global__ void __launch_bounds__(kBlock) render_query_kernel(RayGeom g, const float* __restrict__ ray, const double* __restrict__ cs,
                                                              const int* __restrict__ list, int m, int mode, const float* __restrict__ z,
                                                              const float* __restrict__ zlo, const float* __restrict__ glo,
                                                              const float* __restrict__ ghi, float* __restrict__ q,
                                                              float* __restrict__ x, float* __restrict__ rec) {
    const int nc = 2 * (1 + g.dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int i = list[j];
        float zq = z[i];
        if (mode == 1) {
            zq = zlo[i] + (z[i] - zlo[i]) * 0.5f;
            q[i] = zq;
        } else if (mode == 2) {
            const float a = zlo[i], b = z[i], ga = glo[i];
            if (isnan(ga)) {
                zq = b;
            } else {
                zq = a + (b - a) * (ga / (ga - ghi[i]));
                zq = fminf(fmaxf(zq, a), b);
            }
            q[i] = zq;
        }
        float p0, p1, p2;
        world_point(g, ray, cs, i, zq, p0, p1, p2);
        x[(size_t)j * g.dim] = p0;
        x[(size_t)j * g.dim + 1] = p1;
        if (g.dim == 3) x[(size_t)j * g.dim + 2] = p2;
        rec[(size_t)j * nc] = __int_as_float(0x7fc00000);
        for (int c = 1; c < nc; ++c) rec[(size_t)j * nc + c] = 0.f;
    }
}

// One march step of the listed rays from their records: a crossing outside -> inside with both var_f <= max_var is a hit
// (status 0, bracket [zlo, z]); otherwise the ray advances by clamp(|g|, min_step, max_step) (far_step where f is NaN) of arc
// length, stops with status 2 after max_steps samples or with status 1 past the end of its interval.  flag[j] = keeps marching.
__global__ void __launch_bounds__(kBlock) render_march_kernel(int dim, const float* __restrict__ ray, const int* __restrict__ list, int m,
                                                              const float* __restrict__ rec, RenderOpts o, float* __restrict__ z,
                                                              const float* __restrict__ zend, float* __restrict__ zlo,
                                                              float* __restrict__ glo, float* __restrict__ ghi, int* __restrict__ nstep,
                                                              uint8_t* __restrict__ state, uint8_t* __restrict__ status,
                                                              uint8_t* __restrict__ flag) {
    const int nc = 2 * (1 + dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int i = list[j];
        const float f = rec[(size_t)j * nc], var = rec[(size_t)j * nc + 1 + dim];
        const float gv = f - o.level;
        const bool ok = var <= o.max_var;
        const unsigned st = state[i];
        const float zc = z[i];
        if ((st & 1u) && (st & 2u) && ok && gv < 0.f && !(glo[i] < 0.f)) {
            ghi[i] = gv;
            status[i] = 0;
            flag[j] = 0;
            continue;
        }
        zlo[i] = zc; glo[i] = gv;
        state[i] = (uint8_t)(1u | (ok ? 2u : 0u));
        const int ns = nstep[i] + 1;
        nstep[i] = ns;
        if (ns >= o.max_steps) { status[i] = 2; flag[j] = 0; continue; }
        const float ds = isnan(gv) ? o.far_step : fminf(fmaxf(fabsf(gv), o.min_step), o.max_step);
        const float zn = zc + (dim == 3 ? ds * ray[4 * (size_t)i + 2] : ds);
        if (!(zn <= zend[i])) { status[i] = 1; flag[j] = 0; continue; }
        z[i] = zn;
        flag[j] = 1;
    }
}

// One bisection round from the midpoint records: NaN counts as outside
__global__ void __launch_bounds__(kBlock) render_bisect_kernel(int dim, const int* __restrict__ list, int m, const float* __restrict__ rec,
                                                               float level, const float* __restrict__ q, float* __restrict__ z,
                                                               float* __restrict__ zlo, float* __restrict__ glo, float* __restrict__ ghi) {
    const int nc = 2 * (1 + dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int i = list[j];
        const float gv = rec[(size_t)j * nc] - level;
        if (gv < 0.f) { z[i] = q[i]; ghi[i] = gv; }
        else { zlo[i] = q[i]; glo[i] = gv; }
    }
}

// the output of the hit rays: parameter and record at the secant point
__global__ void __launch_bounds__(kBlock) render_emit_kernel(int dim, const int* __restrict__ list, int m, const float* __restrict__ rec,
                                                             const float* __restrict__ q, float* __restrict__ depth,
                                                             float* __restrict__ out) {
    const int nc = 2 * (1 + dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int i = list[j];
        depth[i] = q[i];
        for (int c = 0; c < nc; ++c) out[(size_t)i * nc + c] = rec[(size_t)j * nc + c];
    }
}

__global__ void __launch_bounds__(kBlock) render_hitflag_kernel(const uint8_t* __restrict__ status, int n, uint8_t* __restrict__ flag) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) flag[i] = status[i] == 0 ? 1 : 0;
}

// ---- deterministic compaction: per-segment counts, one block over the counts, per-segment scatter --------------------------
__global__ void __launch_bounds__(kBlock) render_count_kernel(const uint8_t* __restrict__ flag, int n, int seg, int* __restrict__ part) {
    const int lo = blockIdx.x * seg, hi = min(n, lo + seg);
    int acc = 0;
    for (int t = lo; t < hi; t += kBlock) {
        const int e = t + threadIdx.x;
        acc += __syncthreads_count(e < hi && flag[e]);
    }
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// exclusive prefix of the nb (<= 1024) counts in place; part[nb] = the total.  A one-shot scan with one barrier: block_ops.h's
// block_incl_scan, made for loops, pays a second barrier and 11 more VGPRs here and measured slower.
__global__ void __launch_bounds__(1024) render_top_kernel(int* __restrict__ part, int nb) {
    __shared__ int sh[1024 / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = threadIdx.x < nb ? part[threadIdx.x] : 0;
    int v = a;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < 1024 / 64; ++k) { if (k < w) before += sh[k]; all += sh[k]; }
    if (threadIdx.x < nb) part[threadIdx.x] = before + v - a;
    if (threadIdx.x == 0) part[nb] = all;
}

__global__ void __launch_bounds__(kBlock) render_scatter_kernel(const int* __restrict__ in, const uint8_t* __restrict__ flag, int n,
                                                                int seg, const int* __restrict__ part, int* __restrict__ out) {
    __shared__ int sh[kBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lo = blockIdx.x * seg, hi = min(n, lo + seg);
    int carry = part[blockIdx.x];
    for (int t = lo; t < hi; t += kBlock) {
        const int e = t + threadIdx.x;
        const bool keep = e < hi && flag[e];
        const unsigned long long b = __ballot(keep);
        if (lane == 0) sh[w] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < kBlock / 64; ++k) { if (k < w) before += sh[k]; all += sh[k]; }
        __syncthreads();
        if (keep) out[carry + before + __popcll(b & ((1ull << lane) - 1ull))] = in ? in[e] : e;
        carry += all;
    }
}

// ---- rendering from a distance field --------------------------------------------------------------------------
// Thread -> ray.  Linear: thread t owns ray t.  Tiled (3-D): wavefront w owns the 8 x 8 pixel tile (w / tiles_r, w % tiles_r),
// lane l its pixel (8 (w / tiles_r) + l / 8, 8 (w % tiles_r) + l % 8); -1 where the tile hangs over the image.  The rays of a
// wavefront then end close together and sample neighbouring cells.
__device__ __forceinline__ int field_ray_of_thread(const RayGeom& g, int n, bool tiled) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (!tiled) return t < n ? (int)t : -1;
    const int tiles_r = (g.height + 7) >> 3;
    const long long w = t >> 6;
    const int l = (int)(t & 63);
    const long long col = (w / tiles_r) * 8 + (l >> 3);
    const int row = (int)(w % tiles_r) * 8 + (l & 7);
    return (col < g.width && row < g.height) ? (int)(col * g.height + row) : -1;
}

// One thread marches one ray from set-up to output (sphere tracing): ray_setup's terms and clip, then field_march
// (field_march.h), which the batched prediction of view.hip shares.  Step, hit, refinement and status: tests/render_field_ref.py.
// Nothing is written per sample.  part[3 b ..]: the block's samples, hits and largest per-ray sample count, reduced in a fixed
// order (wave shuffles, then the four waves in order).
template <int D>
__global__ void __launch_bounds__(kBlock) render_field_kernel(RayGeom g, const double* __restrict__ cs, int n, bool tiled,
                                                              RenderFieldOpts o, float lx, float ly, float lz, float hx, float hy,
                                                              float hz, const float* __restrict__ F, DfLattice Lrt,
                                                              float* __restrict__ depth, float* __restrict__ rec,
                                                              uint8_t* __restrict__ status, unsigned long long* __restrict__ part) {
    constexpr int NC = 1 + D;
    __shared__ unsigned long long sh[3][kBlock / 64];
    const float nanf_ = __int_as_float(0x7fc00000);
    const int i = field_ray_of_thread(g, n, tiled);
    DfLattice L = Lrt;
    L.dim = D;                                   // (checked by the host: the sampler's loops unroll, the sample stays in registers)
    int ns = 0, hit = 0;
    if (i >= 0) {
        const float lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
        float u, v, il, z, zend;
        double cd, sd;
        ray_setup(g, cs, i, o.tnear, o.tfar, lo, hi, u, v, il, cd, sd, z, zend);
        float q, smp[NC];
        const int st = field_march<D>(g, u, v, il, cd, sd, z, zend, o, F, L, q, smp, ns);
        hit = st == 0;
        depth[i] = hit ? q : nanf_;
#pragma unroll
        for (int c = 0; c < NC; ++c) rec[(size_t)i * NC + c] = hit ? smp[c] : nanf_;
        status[i] = (uint8_t)st;
    }
    // the block's counters
    unsigned long long a = (unsigned long long)ns, b = (unsigned long long)hit, m = (unsigned long long)ns;
    for (int s = 32; s >= 1; s >>= 1) {
        a += __shfl_down(a, s, 64);
        b += __shfl_down(b, s, 64);
        const unsigned long long y = __shfl_down(m, s, 64);
        m = y > m ? y : m;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[0][w] = a; sh[1][w] = b; sh[2][w] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sa = 0, sb = 0, sm = 0;
        for (int k = 0; k < kBlock / 64; ++k) { sa += sh[0][k]; sb += sh[1][k]; sm = sh[2][k] > sm ? sh[2][k] : sm; }
        part[3 * (size_t)blockIdx.x] = sa; part[3 * (size_t)blockIdx.x + 1] = sb; part[3 * (size_t)blockIdx.x + 2] = sm;
    }
}

// the block partials reduced by one block: thread t takes the blocks t, t + 1024, ... in order, then block_reduce over the
// threads (integers: any order gives the same bits); out = samples, hits, largest per-ray count
__global__ void __launch_bounds__(1024) render_field_top_kernel(const unsigned long long* __restrict__ part, int nb,
                                                                unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[1024 / 64];
    unsigned long long a = 0, b = 0, m = 0;
    for (int k = threadIdx.x; k < nb; k += 1024) {
        a += part[3 * (size_t)k]; b += part[3 * (size_t)k + 1];
        const unsigned long long y = part[3 * (size_t)k + 2];
        m = y > m ? y : m;
    }
    a = block_reduce(a, OpAdd(), sh, 1024, 0ull);
    b = block_reduce(b, OpAdd(), sh, 1024, 0ull);
    m = block_reduce(m, OpMax(), sh, 1024, 0ull);
    if (threadIdx.x == 0) { out[0] = a; out[1] = b; out[2] = m; }
}

}  // namespace

int render_field_check_opts(const RenderFieldOpts& o) {
    if (!std::isfinite(o.tnear) || !std::isfinite(o.tfar) || !(o.tnear >= 0.f) || !(o.tnear < o.tfar)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.min_step) && o.min_step > 0.f) || std::isnan(o.max_step) || !(o.min_step <= o.max_step)) return GPIS_ERR_ARG;
    if (!std::isfinite(o.slack) || o.slack < 0.f || o.refine < 0 || o.refine > 64 || o.max_steps < 1) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int render_check_opts(const RenderOpts& o) {
    auto pos = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (!std::isfinite(o.tnear) || !std::isfinite(o.tfar) || !(o.tnear >= 0.f) || !(o.tnear < o.tfar)) return GPIS_ERR_ARG;
    if (!pos(o.min_step) || !pos(o.max_step) || !(o.min_step <= o.max_step) || !pos(o.far_step)) return GPIS_ERR_ARG;
    if (!std::isfinite(o.level) || std::isnan(o.max_var) || o.refine < 0 || o.refine > 64 || o.max_steps < 1) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int render_check_geom(const RayGeom& g, long long n) {
    if (g.dim == 3) {
        if (g.width < 1 || g.height < 1 || !std::isfinite(g.fx) || !std::isfinite(g.fy) || g.fx == 0.f || g.fy == 0.f ||
            !std::isfinite(g.cx) || !std::isfinite(g.cy))
            return GPIS_ERR_ARG;
    } else if (g.dim != 2 || n < 1) {
        return GPIS_ERR_ARG;
    }
    const int nr = g.dim == 3 ? 9 : 4, nt = g.dim;
    for (int k = 0; k < nr; ++k) if (!std::isfinite(g.R[k])) return GPIS_ERR_ARG;
    for (int k = 0; k < nt; ++k) if (!std::isfinite(g.t[k])) return GPIS_ERR_ARG;
    if (g.dim == 2 && (!std::isfinite(g.off[0]) || !std::isfinite(g.off[1]))) return GPIS_ERR_ARG;
    if (n > Renderer::kMaxRays) return GPIS_ERR_LIMIT;
    return GPIS_OK;
}

Renderer::Renderer() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Renderer::~Renderer() { (void)bind(-1); }

int Renderer::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_ray, (void*)d_cs, (void*)d_z, (void*)d_zend, (void*)d_zlo, (void*)d_glo, (void*)d_ghi, (void*)d_q,
                        (void*)d_nstep, (void*)d_state, (void*)d_flag, (void*)d_list[0], (void*)d_list[1], (void*)d_list[2],
                        (void*)d_x, (void*)d_qrec, (void*)d_part, (void*)d_depth, (void*)d_rec, (void*)d_status})
            (void)hipFree(p);
        if (h_cs) (void)hipHostFree(h_cs);
        if (h_cnt) (void)hipHostFree(h_cnt);
        (void)hipFree(d_fpart);
        if (h_fcnt) (void)hipHostFree(h_fcnt);
        if (own) (void)hipStreamDestroy(own);
    }
    d_ray = nullptr; d_cs = nullptr; d_z = d_zend = d_zlo = d_glo = d_ghi = d_q = nullptr; d_nstep = nullptr;
    d_state = d_flag = nullptr; d_list[0] = d_list[1] = d_list[2] = nullptr; d_x = d_qrec = nullptr; d_part = nullptr;
    d_depth = d_rec = nullptr; d_status = nullptr; h_cs = nullptr; h_cnt = nullptr; own = nullptr;
    d_fpart = nullptr; h_fcnt = nullptr;
    cap = cap_hcs = cap_fpart = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

// every per-ray buffer sized for 3-D (the larger of the two layouts), grown together
int Renderer::ensure(long long n, int dm) {
    const size_t need = (size_t)n;
    if (need > cap) {
        for (void* p : {(void*)d_ray, (void*)d_cs, (void*)d_z, (void*)d_zend, (void*)d_zlo, (void*)d_glo, (void*)d_ghi, (void*)d_q,
                        (void*)d_nstep, (void*)d_state, (void*)d_flag, (void*)d_list[0], (void*)d_list[1], (void*)d_list[2],
                        (void*)d_x, (void*)d_qrec, (void*)d_depth, (void*)d_rec, (void*)d_status})
            (void)hipFree(p);
        d_ray = nullptr; d_cs = nullptr; d_z = d_zend = d_zlo = d_glo = d_ghi = d_q = nullptr; d_nstep = nullptr;
        d_state = d_flag = nullptr; d_list[0] = d_list[1] = d_list[2] = nullptr; d_x = d_qrec = nullptr;
        d_depth = d_rec = nullptr; d_status = nullptr; cap = 0;
        GPIS_HIP(hipMalloc((void**)&d_ray, sizeof(float) * 4 * need));
        GPIS_HIP(hipMalloc((void**)&d_cs, sizeof(double) * 2 * need));
        for (float** p : {&d_z, &d_zend, &d_zlo, &d_glo, &d_ghi, &d_q, &d_depth}) GPIS_HIP(hipMalloc((void**)p, sizeof(float) * need));
        GPIS_HIP(hipMalloc((void**)&d_nstep, sizeof(int) * need));
        GPIS_HIP(hipMalloc((void**)&d_state, need));
        GPIS_HIP(hipMalloc((void**)&d_flag, need));
        GPIS_HIP(hipMalloc((void**)&d_status, need));
        for (int k = 0; k < 3; ++k) GPIS_HIP(hipMalloc((void**)&d_list[k], sizeof(int) * need));
        GPIS_HIP(hipMalloc((void**)&d_x, sizeof(float) * 3 * need));
        GPIS_HIP(hipMalloc((void**)&d_qrec, sizeof(float) * 8 * need));
        GPIS_HIP(hipMalloc((void**)&d_rec, sizeof(float) * 8 * need));
        cap = need;
    }
    if (dm == 2 && need > cap_hcs) {
        if (h_cs) (void)hipHostFree(h_cs);
        h_cs = nullptr; cap_hcs = 0;
        GPIS_HIP(hipHostMalloc((void**)&h_cs, sizeof(double) * 2 * need));
        cap_hcs = need;
    }
    if (!d_part) GPIS_HIP(hipMalloc((void**)&d_part, sizeof(int) * (kScanBlocks + 1)));
    if (!h_cnt) GPIS_HIP(hipHostMalloc((void**)&h_cnt, sizeof(int)));
    return GPIS_OK;
}

int Renderer::compact(const int* in, long long n, int* out, hipStream_t s, long long* count) {
    return compact_flags(d_flag, in, n, out, d_part, h_cnt, s, count);
}

int compact_flags(const uint8_t* flag, const int* in, long long n, int* out, int* d_part, int* h_cnt, hipStream_t s, long long* count) {
    *count = 0;
    if (n <= 0) return GPIS_OK;
    const long long per = (n + kScanBlocks - 1) / kScanBlocks;
    const int seg = (int)std::max((long long)kBlock, (per + kBlock - 1) / kBlock * kBlock);
    const int nb = (int)((n + seg - 1) / seg);
    hipLaunchKernelGGL(render_count_kernel, dim3(nb), dim3(kBlock), 0, s, flag, (int)n, seg, d_part);
    hipLaunchKernelGGL(render_top_kernel, dim3(1), dim3(1024), 0, s, d_part, nb);
    hipLaunchKernelGGL(render_scatter_kernel, dim3(nb), dim3(kBlock), 0, s, in, flag, (int)n, seg, d_part, out);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_cnt, d_part + nb, sizeof(int), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));       // (the one synchronisation a march pass adds to test()'s own)
    *count = *h_cnt;
    return GPIS_OK;
}

// positions + pre-fill of the listed rays, test() on them in calls of at most `chunk` rays
int Renderer::pass(MapQuery& mq, OnGPISStore& store, int mode, const int* list, long long m, const RayGeom& geo, const RenderOpts& o,
                   hipStream_t s) {
    hipLaunchKernelGGL(render_query_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, geo, d_ray, d_cs, list, (int)m, mode, d_z, d_zlo,
                       d_glo, d_ghi, d_q, d_x, d_qrec);
    GPIS_HIP(hipGetLastError());
    const int nc = 2 * (1 + geo.dim);
    const long long C = std::max(1, chunk);
    for (long long off = 0; off < m; off += C) {
        const int len = (int)std::min(C, m - off);
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = mq.run_prepared(store, d_x + (size_t)off * geo.dim, len, d_qrec + (size_t)off * nc, s)) return rc;
        mq_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        evals += mq.last_evals;
        k4_ms += mq.last_eval_ms;
    }
    ++passes;
    samples += m;
    return GPIS_OK;
}

int Renderer::render(MapQuery& mq, OnGPISStore& store, const RayGeom& geo, const double* cs, long long n, const RenderOpts& o,
                     hipStream_t s) {
    clear_result();
    if (int rc = render_check_opts(o)) return rc;
    if (int rc = render_check_geom(geo, n)) return rc;
    if (int rc = ensure(n, geo.dim)) return rc;
    const int dm = geo.dim;
    float lo[3], hi[3];
    const bool empty = !mq.cluster_box(lo, hi);      // (an empty table: every ray misses, the box is reported as NaN)
    for (int a = 0; a < 3; ++a) {
        const float h = mq.search_half();
        lo[a] = empty ? NAN : lo[a] - h;
        hi[a] = empty ? NAN : hi[a] + h;
    }
    if (dm == 2) {
        for (long long i = 0; i < 2 * n; ++i) h_cs[i] = cs[i];
        GPIS_HIP(hipMemcpyAsync(d_cs, h_cs, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(render_setup_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, geo, d_cs, (int)n, empty, o.tnear, o.tfar, lo[0], lo[1],
                       lo[2], hi[0], hi[1], hi[2], d_ray, d_z, d_zend, d_nstep, d_state, d_status, d_flag, d_depth, d_rec);
    GPIS_HIP(hipGetLastError());
    long long nact = 0;
    if (int rc = compact(nullptr, n, d_list[0], s, &nact)) return rc;
    if (nact > 0)
        if (int rc = mq.prepare(store, s)) return rc;
    int cur = 0;
    while (nact > 0) {
        if (int rc = pass(mq, store, 0, d_list[cur], nact, geo, o, s)) return rc;
        ++march_passes;
        hipLaunchKernelGGL(render_march_kernel, dim3(grid_for(nact)), dim3(kBlock), 0, s, dm, d_ray, d_list[cur], (int)nact, d_qrec, o,
                           d_z, d_zend, d_zlo, d_glo, d_ghi, d_nstep, d_state, d_status, d_flag);
        GPIS_HIP(hipGetLastError());
        long long next = 0;
        if (int rc = compact(d_list[cur], nact, d_list[1 - cur], s, &next)) return rc;
        cur = 1 - cur;
        nact = next;
    }
    // the hit rays, in ray order: refinement rounds, the secant point, the output
    hipLaunchKernelGGL(render_hitflag_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, d_status, (int)n, d_flag);
    GPIS_HIP(hipGetLastError());
    long long nh = 0;
    if (int rc = compact(nullptr, n, d_list[2], s, &nh)) return rc;
    if (nh > 0) {
        for (int r = 0; r < o.refine; ++r) {
            if (int rc = pass(mq, store, 1, d_list[2], nh, geo, o, s)) return rc;
            hipLaunchKernelGGL(render_bisect_kernel, dim3(grid_for(nh)), dim3(kBlock), 0, s, dm, d_list[2], (int)nh, d_qrec, o.level, d_q,
                               d_z, d_zlo, d_glo, d_ghi);
            GPIS_HIP(hipGetLastError());
        }
        if (int rc = pass(mq, store, 2, d_list[2], nh, geo, o, s)) return rc;
        hipLaunchKernelGGL(render_emit_kernel, dim3(grid_for(nh)), dim3(kBlock), 0, s, dm, d_list[2], (int)nh, d_qrec, d_q, d_depth, d_rec);
        GPIS_HIP(hipGetLastError());
    }
    GPIS_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) { box_lo[a] = lo[a]; box_hi[a] = hi[a]; }
    dim = dm; nrays = n; hits = nh; valid = true;
    return GPIS_OK;
}

// The whole field render: one fused kernel over the rays, the top reduction of its counters, one page-locked copy
int Renderer::render_field(const DistanceField& df, const RayGeom& geo, const double* cs, long long n, const RenderFieldOpts& o,
                           hipStream_t s) {
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != geo.dim) return GPIS_ERR_ARG;
    if (int rc = render_field_check_opts(o)) return rc;
    if (int rc = render_check_geom(geo, n)) return rc;
    clear_result();
    if (int rc = ensure(n, geo.dim)) return rc;
    const int dm = geo.dim;
    const bool tiled = dm == 3 && field_tiles;
    const long long waves = tiled ? (long long)((geo.width + 7) / 8) * ((geo.height + 7) / 8) : (n + 63) / 64;
    const int nb = (int)((waves + kBlock / 64 - 1) / (kBlock / 64));
    if ((size_t)nb > cap_fpart) {
        (void)hipFree(d_fpart);
        d_fpart = nullptr; cap_fpart = 0;
        GPIS_HIP(hipMalloc((void**)&d_fpart, sizeof(unsigned long long) * 3 * ((size_t)nb + 1)));
        cap_fpart = (size_t)nb;
    }
    if (!h_fcnt) GPIS_HIP(hipHostMalloc((void**)&h_fcnt, sizeof(unsigned long long) * 3));
    const DfLattice L = df.lattice();
    float lo[3] = {L.ox, L.oy, L.oz}, hi[3];
    const int ln[3] = {L.nx, L.ny, L.nz};
    for (int a = 0; a < 3; ++a) hi[a] = lo[a] + (float)(ln[a] - 1) * L.st;
    if (dm == 2) {
        for (long long i = 0; i < 2 * n; ++i) h_cs[i] = cs[i];
        GPIS_HIP(hipMemcpyAsync(d_cs, h_cs, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(render_field_kernel<2>, dim3(nb), dim3(kBlock), 0, s, geo, d_cs, (int)n, tiled, o, lo[0], lo[1], lo[2], hi[0],
                           hi[1], hi[2], df.d_dist, L, d_depth, d_rec, d_status, d_fpart);
    } else {
        hipLaunchKernelGGL(render_field_kernel<3>, dim3(nb), dim3(kBlock), 0, s, geo, d_cs, (int)n, tiled, o, lo[0], lo[1], lo[2], hi[0],
                           hi[1], hi[2], df.d_dist, L, d_depth, d_rec, d_status, d_fpart);
    }
    GPIS_HIP(hipGetLastError());
    unsigned long long* d_out = d_fpart + 3 * (size_t)cap_fpart;
    hipLaunchKernelGGL(render_field_top_kernel, dim3(1), dim3(1024), 0, s, d_fpart, nb, d_out);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_fcnt, d_out, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) { box_lo[a] = lo[a]; box_hi[a] = hi[a]; }
    dim = dm; nrays = n; field = true; valid = true;
    passes = 1; march_passes = 1;
    samples = (long long)h_fcnt[0]; hits = (long long)h_fcnt[1]; max_samples = (long long)h_fcnt[2];
    return GPIS_OK;
}

}  // namespace gpis
