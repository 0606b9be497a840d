// Routes through space and time for the robot's footprint on the device (the contract: tests/tpplan_ref.py): the
// time planner's layer recursion (tplan.h, §7y) on the pose planner's lattice (pplan.h, §7s).  States are (lattice point, heading
// index, real slot).  The static part is the pose planner's: the body rule's free space and point costs, the directed
// translations, the two turns and their weights.  The clock, the wait and the separation of a body ball from a moving ball over
// one interval are the timed body check's (traj.h, §7x).  The graph is acyclic: layer s depends on layer s + 1 alone, so the bits
// are unique by construction.  The handle copies the lattice geometry, the ball table, the footprint and both caller tables during
// solve(): a result outlives its field, its set and its footprint.  What the handle shares with the time planner's is TimePlanCore
// (tplan_host.h), the kernels' shared rules are tplan_dev.h.
#pragma once
#include "body.h"
#include "tplan_host.h"

namespace gpis {

struct DistanceField;

struct TimePosePlanOpts {
    float clearance = 0.f, margin = 0.f, gain = 4.f, turn = 0.f;
    double slot = 0.1;
    int horizon = 256;
    double dyn_clearance = 0.0;
    float wait = 0.5f;
    int keep_cost = 0;
};

struct TimePosePlanner : TimePlanCore {
    static constexpr int kMaxHorizon = 1024, kTile = 8, kMaxH = 64, kMaxT = 256;
    static constexpr int kTurnUp = 27, kTurnDown = 28, kWait = 29;
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr long long kMaxStates = 1ll << 30, kMaxStatesKept = 1ll << 28;
    static constexpr float kMaxWait = 1e4f;

    // grow-only device buffers on top of the shared ones (bind() frees them)
    double* d_body = nullptr;                                      // [Footprint::kMax][kRow]: the solve's copy of the footprint
    double* d_head = nullptr;                                      // [kMaxH][2]
    double* d_rot = nullptr;                                       // [kMaxH][Footprint::kMax][2]: the rotated offsets
    unsigned short* d_moves = nullptr;                             // [kMaxH]
    int* d_pheading = nullptr;                                     // [total], under cap_points with d_points

    // the last result: ns = nx ny H
    int H = 0, mb = 0;
    TimePosePlanOpts opts;

    ~TimePosePlanner() { (void)bind(-1); }
    int bind(int dev) {
        return TimePlanCore::bind(dev, {(void**)&d_body, (void**)&d_head, (void**)&d_rot, (void**)&d_moves, (void**)&d_pheading});
    }
    // Arguments are checked by the caller.  ob: nullptr or a set of this device (2-D where it holds balls); body: a 2-D
    // footprint of this device with m > 0; goals: host [ngoals][3]; synchronises `s`
    int solve(const DistanceField& df, const Obstacles* ob, const Footprint& body, const double* headings, const unsigned short* move_bits,
              int nh, const float* goals, int ngoals, double t_begin, const TimePosePlanOpts& o, hipStream_t s);
    // pose paths from host starts [m][3], each at slot 0: count, scan, write; synchronises `s`
    int paths(const float* starts, int m, hipStream_t s);
    // the last paths against any 2-D set with any 2-D footprint (nullptr: the solve's) at the solve's t_begin, slot and heading
    // table; outputs host [npaths], any may be null
    int check(const Obstacles& ob, const Footprint* body, double clearance, double* min_sep, double* min_time, int* min_obstacle,
              int* min_ball, int* first_hit, int* collides);
    // U [npaths][T][2], heading0 [npaths][2], p0 [npaths][2], clamped [npaths]: host, any may be null
    int controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped);
};

// GPIS_OK or GPIS_ERR_ARG for a lattice of step `step` (0: the lattice is not known, turn is only asked to be positive)
int tpplan_check_opts(const TimePosePlanOpts& o, float step);

}  // namespace gpis
