// Trajectory smoothing through a distance field on the device: a batch of m trajectories of N waypoints, either
// resampled by arc length from a planner's last paths or given by the caller, run through a fixed-order covariant gradient
// descent (smoothness + obstacle term from the field's sampler, the inverse of tridiag(-1, 2, -1) in closed form, a trust
// region) and an evaluation pass that doubles as a collision check.  float32, no FMA; every sum has one order, so the bits are
// those of tests/traj_ref.py.  One workgroup per trajectory, every iteration inside one launch.  The optimiser keeps its input and
// its result apart: a call always starts from the input, and a result outlives the field and the planner it came from.
#pragma once
#include <cstdint>
#include "dev_common.h"

namespace gpis {

struct DistanceField;
struct Planner;

struct TrajOpts {
    float clearance = 0.f, margin = 1.f, w_smooth = 1.f, w_obs = 0.f, rate = 0.f, max_move = 0.f, tol = 0.f;
    int iters = 0, sub = 0;
};

struct Trajectories {
    static constexpr int kMinN = 3, kMaxN = 256;     // waypoints per trajectory (the reduction tree's width)
    static constexpr int kMaxSub = 16;               // evaluation points inside a segment
    static constexpr int kMaxTraj = 1 << 20;

    int device = -1;
    hipStream_t own = nullptr;

    // grow-only device buffers
    float* d_in = nullptr;                           // [m][N][dim] the input waypoints
    float* d_x = nullptr;                            // [m][N][dim] the result's
    size_t cap_x = 0;
    unsigned char* d_instat = nullptr;               // [m] 0: input present, 2: none
    float* d_fres = nullptr;                         // [m][4] length, smoothness, obstacle cost, min_dist
    int* d_ires = nullptr;                           // [m][4] status, iterations, non-finite samples, collides
    size_t cap_m = 0;
    float* d_arc = nullptr; size_t cap_arc = 0;      // cumulative lengths, one float per path point

    int m = 0, N = 0, dim = 0;
    bool has_input = false, valid = false;
    double opt_ms = 0.0;

    Trajectories();
    ~Trajectories();
    int bind(int dev);                               // move to `dev`, the input carried along (the result is dropped)
    // the input from the planner's last paths, N waypoints each; moves to the planner's device; synchronises the own stream
    int from_paths(const Planner& p, int N);
    // the input from host waypoints [m][N][dim]
    int set(const float* x, int m, int N, int dim);
    // descent and evaluation from the input on df's dist; synchronises `s`
    int optimize(const DistanceField& df, const TrajOpts& o, hipStream_t s);

private:
    int ensure(int m, int N, int dim);
};

// GPIS_ERR_ARG on anything gpis_traj_optimize documents as an argument error of the options
int traj_check_opts(const TrajOpts& o);

}  // namespace gpis
