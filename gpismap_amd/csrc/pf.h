// Monte-Carlo localisation against a distance field, resident on the device: a particle set (SE(2) / SE(3)
// states in double, the float32 poses the scorer reads, accumulated negative log weights) that is moved (predict), weighed
// against a frame (update: the pose scorer's cost of locate.h on the tracker's points), summarised (integer totals, N_eff, the
// weighted mean pose by the tracker's fixed tree) and resampled (systematic, all-integer) without leaving the device; a step
// copies back one small block (PfStats).  Every stage but one exp has exactly one result (tests/pf_ref.py states them); no
// kernel waits on another workgroup, no floating-point atomics.
#pragma once
#include <cstdint>
#include "dev_common.h"
#include "track.h"

namespace gpis {

struct DistanceField;

struct PfOpts {
    double max_residual;     // the scorer's truncation
    double beta;             // L += beta * cost
    double sigma_t[3];       // motion noise of the translation, body frame (2-D: the first two)
    double sigma_r;          // motion noise of the rotation (radians for small angles)
    double resample_below;   // update resamples iff neff < resample_below * m
    int stride;              // 3-D: pixel stride of the tracker's points; ignored in 2-D (but checked)
};

// what comes back from the device after an update
struct PfStats {
    double sums[7];                  // the tree sums of (double)q * state column (4 in 2-D)
    double lmin;                     // min L
    unsigned long long T, Th, S2;    // sum q, sum (q >> 16), sum (q >> 16)^2
    unsigned long long qmax;         // max q
    int best, pad;                   // the lowest index of maximal q
};

struct ParticleFilter {
    static constexpr long long kMaxParticles = 1ll << 24;
    static constexpr int kBlock = 256;           // threads per workgroup; points per segment of the estimate's tree

    int device = -1;             // buffers live here (the device current at init; an update needs a field of this device)
    Tracker trk;                 // the frame's points: the tracker's set-up and its buffers (its own result is never used)

    // grow-only device buffers (cap_m particles)
    double* d_state[2] = {nullptr, nullptr};     // [m][4 / 7], ping-pong
    float* d_pose[2] = {nullptr, nullptr};       // [m][6 / 12], ping-pong
    double* d_L = nullptr;                       // [m]
    unsigned long long* d_q = nullptr;           // [m] the last update's weights (2^32 each after init)
    unsigned long long* d_C = nullptr;           // [m] their inclusive prefix sum (resample)
    double* d_cost = nullptr;                    // [m]
    int* d_inl = nullptr;                        // [m]
    int* d_anc = nullptr;                        // [m] ancestors of the last resampling (the identity after init)
    // per-block partials (nb = ceil(m / 256) blocks), the scan's levels, the estimate's segment partials
    double* d_bmin = nullptr;                    // [nb] block minima of L
    unsigned long long* d_bsum = nullptr;        // [3][nb] block sums of q, q >> 16, (q >> 16)^2
    unsigned long long* d_bkey = nullptr;        // [nb] block maxima of (q << 24) | (2^24 - 1 - index)
    unsigned long long* d_s1 = nullptr;          // [nb] block sums of the scan, then their scan
    unsigned long long* d_s2 = nullptr;          // [257] the next two levels
    double* d_part = nullptr;                    // [7][P], P = nb rounded up to a power of two
    PfStats* d_stats = nullptr;
    PfStats* h_stats = nullptr;                  // page-locked
    char* h_stage = nullptr;                     // page-locked staging of init's upload
    size_t cap_m = 0;

    // the state
    bool inited = false, have_estimate = false;
    int dim = 0, cur = 0;        // cur: which half of the ping-pong buffers holds the set
    long long m = 0, npoints = 0, pixels = 0, updates = 0, resamples = 0;
    uint32_t tick = 0;
    uint64_t seed = 0;
    bool resampled = false;      // by the last update
    double neff = 0.0, est[7] = {}, est_pose[12] = {};
    PfStats stats = {};
    double ms = 0.0;             // host wall time of the last update

    ParticleFilter();
    ~ParticleFilter();
    int bind(int dev);           // move to `dev` (frees the buffers of another device and drops the set)
    // poses: m x 12 / 6 floats (host), finite (checked by the caller); on the device current in the caller
    int init(int dm, const float* poses, long long m, uint64_t seed);
    // motion: 2-D (dx, dy, cu, su), 3-D (d(3), Qu(4)); o checked by the caller; synchronises `s`
    int predict(const double* motion, const PfOpts& o, hipStream_t s);
    // The measurement update: the tracker's set-up on the frame, the scoring launch, weights, totals, estimate, one copy back,
    // then the resampling if N_eff asks for it; synchronises `s`.  in, cs, n: as Tracker::track_field.  Arguments are checked by
    // the caller; the field holds a result of geo.dim on this device.
    int update(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n, const PfOpts& o,
               hipStream_t s);
    int resample(hipStream_t s); // synchronises `s`
    const double* state() const { return d_state[cur]; }
    const float* poses() const { return d_pose[cur]; }
    hipStream_t stream_or_own(hipStream_t s) const { return s ? s : trk.own; }

private:
    int ensure(long long m);
    int resample_launch(hipStream_t s);
};

// GPIS_OK or GPIS_ERR_ARG: stride < 1, a negative or non-finite sigma, beta, max_residual or resample_below
int pf_check_opts(const PfOpts& o);
// (w, x, y, z) of a column-major rotation matrix R[9]: the trace / largest-diagonal branches in double, then normalised
// (tests/pf_ref.py: mat_to_quat)
void pf_mat_to_quat(const double* R, double* q);
// R[9] column-major of a quaternion (w, x, y, z), in double
void pf_quat_to_mat(const double* q, double* R);
// Philox4x32-10 of one counter (host; the device uses the same rounds)
void pf_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

}  // namespace gpis
