// Depth images and laser scans rendered from the map on the device: rays marched through the map's test(), one
// MapQuery pass over the rays still active per step, the crossing refined by bisection and a secant point.  The active rays are
// compacted by a deterministic exclusive scan after every pass (no atomics), so the result is the same bits on every run.
// The same views from a distance field (§7g): sphere tracing through the field's sampler, one thread per ray in one fused kernel.
#pragma once
#include <cstdint>
#include "dev_common.h"
#include "frame.h"

namespace gpis {

class MapQuery;
class OnGPISStore;
struct DistanceField;

struct RenderOpts {
    float tnear, tfar;          // ray interval: depth z (3-D) / range r (2-D)
    float min_step, max_step;   // clamp of |f - level| as the arc-length step (metres)
    float far_step;             // arc-length step after a sample without a GP answer (f NaN)
    float level;                // surface level (inside iff f < level)
    float max_var;              // both samples of a crossing need var_f <= max_var
    int refine;                 // bisection rounds on the bracket of a hit
    int max_steps;              // samples per ray before it stops with status 2
};

// the march through a distance field (§7g): no level and no variance gate (the field's level is zero, its gate was applied when
// it was built)
struct RenderFieldOpts {
    float tnear, tfar;          // ray interval: depth z (3-D) / range r (2-D)
    float min_step, max_step;   // clamp of the arc-length step |d| - slack * step (metres); max_step may be +inf
    float slack;                // lattice steps taken off |d| before it is used as a step
    int refine;                 // bisection rounds on the bracket of a hit
    int max_steps;              // samples per ray before it stops with status 2
};

// pinhole camera / pose of one render (3-D: pose [t(3), R(9) column-major]; 2-D: pose [t(2), R(4)], sensor offset)
struct RayGeom {
    int dim, width, height;
    float fx, fy, cx, cy;
    float R[9], t[3], off[2];
};

struct Renderer {
    static constexpr long long kMaxRays = 1ll << 26;
    static_assert(kMaxRays == kMaxFramePoints, "frame.h checks a frame against the renderer's limit");

    int device = -1;             // buffers live here (the device current at creation; rebound to a map's device on use)
    hipStream_t own = nullptr;   // stream used when the caller passes none
    int chunk = 1 << 22;         // rays per test() call within a pass (the results do not depend on it)

    // grow-only device buffers, per ray
    float* d_ray = nullptr;      // 3-D: u, v, 1/sqrt(u^2 + v^2 + 1), - per ray
    double* d_cs = nullptr;      // 2-D: cos, sin of the beam angle (host double)
    float* d_z = nullptr;        // current sample / bracket top
    float* d_zend = nullptr;     // far end of the clipped interval
    float* d_zlo = nullptr;      // previous sample / bracket bottom
    float* d_glo = nullptr;      // g at d_zlo
    float* d_ghi = nullptr;      // g at d_z (from the hit on)
    float* d_q = nullptr;        // parameter of the last refinement query
    int* d_nstep = nullptr;      // samples taken
    uint8_t* d_state = nullptr;  // bit 0: d_zlo holds a sample, bit 1: its var_f <= max_var
    uint8_t* d_flag = nullptr;   // compaction flags
    int* d_list[3] = {nullptr, nullptr, nullptr};   // active lists (two, swapped per pass) and the hit list
    float* d_x = nullptr;        // positions of the queried rays [m][dim]
    float* d_qrec = nullptr;     // their test() records [m][2(1+dim)]
    size_t cap = 0;
    double* h_cs = nullptr; size_t cap_hcs = 0;      // page-locked staging of the 2-D directions
    int* d_part = nullptr;       // compaction: per-block counts (kScanBlocks + 1)
    int* h_cnt = nullptr;        // page-locked: the count of the last compaction
    unsigned long long* d_fpart = nullptr; size_t cap_fpart = 0;   // field render: per-block counters (3 each) and their sums
    unsigned long long* h_fcnt = nullptr;                          // page-locked: samples, hits, largest per-ray sample count
    bool field_tiles = true;     // field render, 3-D: a wavefront owns an 8 x 8 pixel tile (false: 64 consecutive rays of the
                                 // column-major image); the results do not depend on it
    // outputs
    float* d_depth = nullptr; float* d_rec = nullptr; uint8_t* d_status = nullptr;

    // the last result
    int dim = 0;
    long long nrays = 0;
    bool valid = false;
    bool field = false;          // the result is a field render: d_rec is [n][1 + dim] (d, gradient), else [n][2(1 + dim)]
    long long passes = 0, march_passes = 0, samples = 0, evals = 0, hits = 0;
    long long max_samples = 0;   // field render: the largest number of samples a single ray took
    double k4_ms = 0.0;
    double mq_ms = 0.0;          // host wall time inside MapQuery::run_prepared (each call ends with its stream synchronised)
    float box_lo[3] = {0.f, 0.f, 0.f}, box_hi[3] = {0.f, 0.f, 0.f};   // the clip box used (search half-width included)

    Renderer();
    ~Renderer();
    void clear_result() { valid = field = false; nrays = 0; dim = 0; passes = march_passes = samples = evals = hits = max_samples = 0; k4_ms = mq_ms = 0.0; }
    int rec_width() const { return field ? 1 + dim : 2 * (1 + dim); }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // The whole render: set-up and clip, the march, refinement, the output; synchronises `s`.  cs: 2-D beam cos / sin (host,
    // 2n doubles), ignored in 3-D.  Arguments are checked by the caller (render_check_*).
    int render(MapQuery& mq, OnGPISStore& store, const RayGeom& geo, const double* cs, long long n, const RenderOpts& o,
               hipStream_t s);
    // The same views from a distance field: one fused kernel, a thread per ray; synchronises `s`.  The field must
    // live on this renderer's device.  A field without a result: GPIS_ERR_STATE; one of another dim, bad options or geometry:
    // GPIS_ERR_ARG / GPIS_ERR_LIMIT; all before the previous result is dropped.  passes = march_passes = 1, evals = 0.
    int render_field(const DistanceField& df, const RayGeom& geo, const double* cs, long long n, const RenderFieldOpts& o,
                     hipStream_t s);

private:
    int ensure(long long n, int dm);
    int compact(const int* in, long long n, int* out, hipStream_t s, long long* count);
    int pass(MapQuery& mq, OnGPISStore& store, int mode, const int* list, long long m, const RayGeom& geo, const RenderOpts& o,
             hipStream_t s);
};

// The renderer's deterministic compaction, shared with the tracker (track.hip): out[0 .. count) = the entries e < n of `in` (the
// identity when in is null) whose flag[e] is set, in order; one exclusive scan over at most kCompactBlocks contiguous segments
// (no atomics).  d_part: kCompactBlocks + 1 device ints; h_cnt: one page-locked int.  Synchronises `s`.
constexpr int kCompactBlocks = 1024;
int compact_flags(const uint8_t* flag, const int* in, long long n, int* out, int* d_part, int* h_cnt, hipStream_t s, long long* count);

// Argument checks shared by the C-ABI entries: GPIS_OK, GPIS_ERR_ARG, or GPIS_ERR_LIMIT (more than kMaxRays rays).
int render_check_opts(const RenderOpts& o);
int render_field_check_opts(const RenderFieldOpts& o);
int render_check_geom(const RayGeom& g, long long n);

// the rays of a checked frame seen from `pose` (3-D [t(3), R(9) column-major], 2-D [t(2), R(4)])
inline RayGeom ray_geom(const SensorFrame& f, const float* pose) {
    const TrackGeom& g = f.geo;
    RayGeom r{g.dim, g.width, g.height, g.fx, g.fy, g.cx, g.cy, {}, {}, {g.off[0], g.off[1]}};
    for (int k = 0; k < g.dim; ++k) r.t[k] = pose[k];
    for (int k = 0; k < g.dim * g.dim; ++k) r.R[k] = pose[g.dim + k];
    return r;
}

}  // namespace gpis
