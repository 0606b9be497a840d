// Scoring batches of pose hypotheses against a distance field on the device: which of these poses explains this
// frame?  The frame's points are the tracker's (its set-up: flag, compaction, gather); one kernel scores every pose -- one
// wavefront per pose walks the points, samples the field at each world point and sums the truncated squared distances in one
// fixed order (64 lane slots, then a halving tree through lane shuffles); cost and inlier count come back in one copy of 12 bytes
// per pose and the host ranks them.  No atomics; the same bits for a pose alone, in any batch, at any batch position.
#pragma once
#include <vector>
#include "dev_common.h"
#include "track.h"

namespace gpis {

struct DistanceField;

struct LocateOpts {
    double max_residual;   // inlier: |d| <= max_residual; every other point pays max_residual^2
    int stride;            // 3-D: pixel stride of the tracker's points; ignored in 2-D
    int top_k;             // poses ranked (0: all)
};

struct Locator {
    static constexpr long long kMaxPoses = 1ll << 24;
    static constexpr int kWaves = 4;             // poses per workgroup of 256 threads

    int device = -1;             // buffers live here (the device current at creation; rebound to a field's device on use)
    Tracker trk;                 // the frame's points: the tracker's set-up and its buffers (its own result is never used)

    // grow-only buffers
    float* d_pose = nullptr;     // the poses [m][12 / 6]
    char* d_out = nullptr;       // cost [m] doubles, then inliers [m] ints
    float* h_pose = nullptr;     // page-locked staging of the poses
    char* h_out = nullptr;       // page-locked: the copy back
    size_t cap_m = 0;

    // the last result
    bool valid = false;
    int dim = 0;
    long long poses = 0, npoints = 0, pixels = 0;
    double ms = 0.0;             // host wall time of the call
    std::vector<double> cost;
    std::vector<int> inliers, order;

    Locator();
    ~Locator();
    void clear_result() { valid = false; dim = 0; poses = npoints = pixels = 0; ms = 0.0; cost.clear(); inliers.clear(); order.clear(); }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // The whole call: the tracker's set-up on the frame, the poses uploaded, one scoring launch, the copy back, the ranking;
    // synchronises `s`.  in, cs, n: as Tracker::track_field.  pose: m x 12 / 6 floats (host).  Arguments are checked by the
    // caller (locate_check_opts, track_check_geom, m in [1, kMaxPoses]); the field holds a result of geo.dim on this device.
    int score(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n, const float* pose, int m,
              const LocateOpts& o, hipStream_t s);
    const double* d_cost() const { return valid ? (const double*)d_out : nullptr; }
    const int* d_inliers() const { return valid ? (const int*)(d_out + sizeof(double) * (size_t)poses) : nullptr; }

private:
    int ensure(long long m);
};

// One launch of the scoring kernel on `s`, also the particle filter's (pf.h): cost [m] and inliers [m] (device) of the device poses
// d_pose [m][12 / 6] against the device points d_loc [p] (float4 each, the tracker's) and the field's result.  dim = df.dim in
// {2, 3}; m >= 1; nothing is synchronised.  GPIS_OK / GPIS_ERR_HIP.
int locate_score_launch(const DistanceField& df, int dim, const float* d_pose, int m, const float* d_loc, long long p,
                        double max_residual, double* d_cost, int* d_inliers, hipStream_t s);

// GPIS_OK or GPIS_ERR_ARG: stride < 1, top_k < 0, a negative, NaN or infinite max_residual
int locate_check_opts(const LocateOpts& o);

}  // namespace gpis
