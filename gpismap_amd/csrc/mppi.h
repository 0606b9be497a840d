// Sampled model-predictive control (MPPI) against a distance field, resident on the device: K noisy control
// sequences around a nominal one are rolled through a kinematic model for T steps (one thread per rollout), charged the field's
// obstacle cost along the way and the planner's cost-to-go (or the distance to a goal point) at the end, weighed (integer
// weights q = floor(exp(-(J - Jmin) / lambda) 2^32)), and the nominal sequence moves to their weighted mean by the tracker's
// fixed tree.  A step copies back one small block (MppiStats).  Every stage but one exp has exactly one result
// (tests/mppi_ref.py states them); no kernel waits on another workgroup, no atomics.
#pragma once
#include <cstdint>
#include "dev_common.h"

namespace gpis {

struct DistanceField;
struct Planner;
struct ObstArgs;
struct BodyArgs;

struct MppiOpts {
    double dt, lambda, gamma;
    double sigma[4], umin[4], umax[4];
    double clearance, margin;
    double w_obs, w_col, w_off, w_goal;
};

// what comes back from the device after a step (88 bytes)
struct MppiStats {
    double jmin;                     // min J
    unsigned long long T, Th, S2;    // sum q, sum (q >> 16), sum (q >> 16)^2
    double nominal_cost;             // the cost of the new nominal sequence's rollout
    int best, nhit;                  // the lowest index of minimal J; rollouts with a hit count > 0
    int nominal_hits, pad;
    double u0[4];                    // the new Ubar[0]
};

// what a step that saw moving balls (obst.h) copies back besides
struct ObstStats {
    double nominal_min_sep;          // the nominal rollout's least separation
    int nominal_dyn_hits, ndyn;      // its steps nearer than the set's clearance; rollouts with such a step
};

struct Controller {
    static constexpr int kMaxRollouts = 65536, kMaxSteps = 256;
    static constexpr int kRollBlock = 64;        // threads per workgroup of the rollout kernel
    static constexpr int kBlock = 256;           // threads per workgroup elsewhere; rollouts per segment of the update's tree
    static constexpr int kCols = 8;              // (t, u) columns per workgroup of the update kernel

    int device = -1;
    hipStream_t own = nullptr;

    // grow-only device buffers
    double* d_U[2] = {nullptr, nullptr};         // [T][U], ping-pong: the update reads one half and writes the other
    size_t cap_u = 0;
    double* d_J = nullptr;                       // [K]
    unsigned long long* d_q = nullptr;           // [K]
    int* d_hits = nullptr;                       // [K]
    double* d_bmin = nullptr;                    // [ceil(K / 64)] block minima of J
    unsigned long long* d_bsum = nullptr;        // [5][ceil(K / 256)] block sums of q, q >> 16, (q >> 16)^2, hit > 0; the best key
    size_t cap_k = 0;
    double* d_part = nullptr;                    // [columns rounded up to kCols][P], P = segments rounded up to a power of two
    size_t cap_part = 0;
    double* d_nom = nullptr;                     // [T + 1][dim + 2] the nominal rollout's states
    size_t cap_nom = 0;
    MppiStats* d_stats = nullptr;
    MppiStats* h_stats = nullptr;                // page-locked
    // allocated by the first step that sees a non-empty set of moving balls
    int* d_dyn = nullptr;                        // [K] steps nearer a ball than the set's clearance
    double* d_msep = nullptr;                    // [K] the least separation
    int* d_bdyn = nullptr;                       // [ceil(K / 64)] rollouts of the block with dyn > 0
    size_t cap_dyn = 0;
    ObstStats* d_ostats = nullptr;
    ObstStats* h_ostats = nullptr;               // page-locked

    // the state
    bool inited = false, have_step = false;
    int dim = 0, K = 0, T = 0, cur = 0;          // cur: which half of d_U holds the nominal sequence
    uint32_t tick = 0;
    uint64_t seed = 0;
    long long steps = 0;
    MppiStats stats = {};
    double neff = 0.0, ms = 0.0;                 // ms: host wall time of the last step
    int obst_n = 0;                              // balls the last step saw (0: d_dyn and d_msep hold nothing of it)
    ObstStats ostats = {};

    Controller();
    ~Controller();
    int bind(int dev);           // move to `dev` (frees the buffers of another device and drops the state)
    int init(int dm, int k, int t, uint64_t sd);                 // on the device current in the caller
    int set_nominal(const double* U);                            // host [T][U]
    // start: (x, y[, z], c, s); goal: [dim] or nullptr; pl: nullptr or a planner holding a cost-to-go on df's lattice.
    // ob: nullptr, or the moving balls' table and constants (n > 0): the kernels with their term run in place of the plain ones.
    // bd: nullptr, or a footprint's table (m > 0; body.h): the kernels with the body rule run in place of those.
    // Arguments are checked by the caller.  Synchronises `s`.
    int step(const DistanceField& df, const Planner* pl, const double* start, const double* goal, const MppiOpts& o, hipStream_t s,
             const ObstArgs* ob = nullptr, const BodyArgs* bd = nullptr);
    int shift();
    int nu() const { return dim == 3 ? 4 : 2; }
    hipStream_t stream_or_own(hipStream_t s) const { return s ? s : own; }

private:
    int ensure(int dm, int k, int t);
};

// GPIS_OK or GPIS_ERR_ARG: a non-finite entry, dt <= 0, lambda <= 0, a negative sigma / weight / margin, umin[u] > umax[u]
int mppi_check_opts(const MppiOpts& o);
void mppi_default_opts(int dim, float step, MppiOpts* o);

}  // namespace gpis
