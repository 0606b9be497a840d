// Sensor tracking against the map on the device: damped Gauss-Newton on SE(3) (3-D) / SE(2) (2-D) of a depth
// image / laser scan against the map's zero level, or against a distance field's (§7f).  One MapQuery pass (a field: one fused
// kernel) per iteration over the frame's valid points; the residual
// and Jacobian terms are reduced to the normal equations on the device by a fixed two-stage halving tree (no atomics), and only
// the sums (29 / 11 doubles) leave it.  The host solves the 6x6 / 3x3 system and moves the pose.
#pragma once
#include <chrono>
#include <cstdint>
#include <functional>
#include "dev_common.h"
#include "frame.h"

namespace gpis {

class MapQuery;
class OnGPISStore;
struct DistanceField;

struct TrackOpts {
    double max_residual;   // inlier: |r| <= max_residual
    double huber;          // Huber threshold delta: w = 1 for |r| <= delta, else delta / |r|
    double max_var;        // inlier: var_f <= max_var
    double damping;        // lambda of (H + lambda diag(H)) delta = -b
    double eps_t, eps_r;   // converged: |v| < eps_t and |omega| < eps_r
    float level;           // surface level (r = f - level)
    int stride;            // 3-D: pixel stride (update()'s obs_skip); ignored in 2-D
    int max_iters;         // 0: evaluate the given pose only
    int min_inliers;       // fewer: status 2
};

struct Tracker {
    static constexpr long long kMaxPoints = 1ll << 26;
    static_assert(kMaxPoints == kMaxFramePoints, "frame.h checks a frame against the tracker's limit");
    static constexpr int kSeg = 256;             // points per segment of the first reduction stage
    static constexpr int kSums3 = 29, kSums2 = 11;

    int device = -1;             // buffers live here (the device current at creation; rebound to a map's device on use)
    hipStream_t own = nullptr;   // stream used when the caller passes none
    int chunk = 1 << 22;         // points per test() call within a pass (the results do not depend on it)

    // grow-only device buffers
    float* d_in = nullptr;       // the depth image / ranges (per pixel)
    double* d_cs = nullptr;      // 2-D: cos, sin of the beam angles (per beam)
    uint8_t* d_flag = nullptr;   // compaction flags (per sample of the grid)
    int* d_list = nullptr;       // the valid samples, in order
    float* d_loc = nullptr;      // per point: local x, y, z (2-D: x, y, 0) and the pixel index (int bits)
    float* d_x = nullptr;        // world points of the pass [m][dim]
    float* d_rec = nullptr;      // their test() records [m][2(1+dim)]
    double* d_part = nullptr;    // segment partials [kSums3][P] (P = segments rounded up to a power of two)
    double* d_sum = nullptr;     // the reduced sums (kSums3)
    float* d_resid = nullptr;    // per-pixel residual of the final pass
    size_t cap_pix = 0, cap_grid = 0, cap_part = 0;
    int* d_scan = nullptr;       // compaction: per-block counts
    int* h_cnt = nullptr;        // page-locked: the count of the compaction
    double* h_sum = nullptr;     // page-locked: the sums of the last pass
    float* h_in = nullptr; size_t cap_hin = 0;       // page-locked staging of the input
    double* h_cs = nullptr; size_t cap_hcs = 0;      // page-locked staging of the 2-D directions

    // the last result
    int dim = 0;
    bool valid = false;
    long long pixels = 0, points = 0, passes = 0, evals = 0;
    int status = 0, iterations = 0;
    double inliers = 0.0, cost0 = 0.0, cost = 0.0;
    double H[36] = {}, b[6] = {};   // the normal equations at the returned pose (full symmetric n x n, row-major)
    double pose[12] = {};           // the returned pose (3-D [t(3), R(9)], 2-D [t(2), R(4)])
    double k4_ms = 0.0;
    double pass_ms = 0.0;           // host wall time of the passes (transform, test(), terms, reduction, sum read-back)

    Tracker();
    ~Tracker();
    void clear_result() { valid = false; dim = 0; pixels = points = passes = evals = 0; status = iterations = 0; inliers = cost0 = cost = 0.0; k4_ms = pass_ms = 0.0; }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // The whole call: back-projection and compaction, the iterations, the final pass and the residual image; synchronises `s`.
    // in: depth [width * height] (3-D) / ranges [n] (2-D), host.  cs: 2-D beam cos / sin (host, 2n doubles).  pose0: double.
    // have_map false: no tree yet (every record keeps f = NaN: status 2).  Arguments are checked by the caller (track_check_*).
    int track(MapQuery& mq, OnGPISStore& store, bool have_map, const TrackGeom& geo, const float* in, const double* cs, long long n,
              const double* pose0, const TrackOpts& o, hipStream_t s);
    // The same call against a distance field: r = the sampled distance, one fused kernel per pass; o.level and
    // o.max_var are not read; evals and k4_ms stay 0.  The field must live on this tracker's device.  A field without a result:
    // GPIS_ERR_STATE, one of another dim: GPIS_ERR_ARG, both before the previous result is dropped.
    int track_field(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n,
                    const double* pose0, const TrackOpts& o, hipStream_t s);
    // The set-up shared by every call, also the locator's (locate.h): drops the result, checks, uploads the input, flags,
    // compacts and gathers the valid samples into d_loc (`points` of them; synchronises `s`).  Only o.stride is read beyond the checks.
    int setup(const TrackGeom& geo, const float* in, const double* cs, long long n, const TrackOpts& o, hipStream_t s);

private:
    using PassFn = std::function<int(const double* pose, double* sums)>;
    int ensure(long long npix, long long ngrid, int dm);
    int iterate(int dm, const double* pose0, const TrackOpts& o, const PassFn& pass_at, double* cur, double* S, int& st, int& it);
    void finish(int dm, long long n, const double* cur, const double* S, int st, int it);
    int pass(MapQuery& mq, OnGPISStore& store, bool have_map, const TrackGeom& geo, const double* pose, const TrackOpts& o,
             hipStream_t s, double* sums);
    int field_pass(const DistanceField& df, int dm, const double* pose, const TrackOpts& o, hipStream_t s, double* sums);
    int pass_sums(int dm, long long np, hipStream_t s, double* sums, std::chrono::steady_clock::time_point t0);
};

// Argument checks shared by the C-ABI entries: GPIS_OK, GPIS_ERR_ARG, or GPIS_ERR_LIMIT (more than kMaxPoints pixels / beams).
int track_check_opts(const TrackOpts& o);
int track_check_geom(const TrackGeom& g, long long n);

// The host half of one iteration (tests/track_ref.py restates both):
// solve (H + lambda diag(H)) delta = -b by Cholesky; false on a non-positive pivot.  n = 6 (3-D) / 3 (2-D).
bool track_solve(int n, const double* H, const double* b, double lambda, double* delta);
// pose <- (Exp(omega) R, t + v), delta = (v, omega)
void track_apply(int dim, const double* delta, double* pose);

}  // namespace gpis
