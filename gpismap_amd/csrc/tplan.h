// Routes through space and time around moving balls on the device (the contract: tests/tplan_ref.py): a planner on
// the time-expanded lattice (lattice point x real slot) of a 2-D field.  The static part is the planner's (plan.h): free space,
// point costs, the translations, their weights and the no-corner-cutting rule; the clock and the separation of a move from a ball
// are the re-timing's (traj.h, §7w).  The graph is acyclic: layer s depends on layer s + 1 alone, so there is no fixed point to
// iterate to and the bits are unique by construction.  The handle copies the lattice geometry and the ball table during solve():
// a result outlives its field and its set.  What the handle shares with the time-pose planner's (tpplan.h) is TimePlanCore
// (tplan_host.h), the kernels' shared rules are tplan_dev.h.
#pragma once
#include "tplan_host.h"

namespace gpis {

struct DistanceField;

struct TimePlanOpts {
    float clearance = 0.f, margin = 0.f, gain = 4.f;
    int connectivity = 1;
    double slot = 0.1;
    int horizon = 256;
    double dyn_clearance = 0.0;
    float wait = 0.5f;
    int keep_cost = 0;
};

struct TimePlanner : TimePlanCore {
    static constexpr int kMaxHorizon = 1024, kMaxLayers = 16, kLayersNoBalls = 4, kTile = 32, kMaxT = 256;
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr long long kMaxStates = 1ll << 30, kMaxStatesKept = 1ll << 28;
    static constexpr float kMaxWait = 1e4f;

    int layers_per_launch = 0;               // the schedule (test hook: the results do not depend on it); 0: chosen per solve
    TimePlanOpts opts;                       // of the last result

    // ob: nullptr or a set of this device (2-D where it holds balls); goals: host [ngoals][2]; synchronises `s`
    int solve(const DistanceField& df, const Obstacles* ob, const float* goals, int ngoals, double t_begin, const TimePlanOpts& o,
              hipStream_t s);
    int paths(const float* starts, int m, hipStream_t s);
    // the last paths against any 2-D set at the solve's t_begin and slot; outputs host [npaths], any may be null
    int check(const Obstacles& ob, double clearance, double* min_sep, double* min_time, int* min_obstacle, int* first_hit, int* collides);
    // U [npaths][T][2], heading0 [npaths][2], p0 [npaths][2], clamped [npaths]: host, any may be null
    int controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped);
};

// GPIS_OK or GPIS_ERR_ARG
int tplan_check_opts(const TimePlanOpts& o);

}  // namespace gpis
