// Routes through space and time for the robot's footprint on the device (the contract: tests/tpplan_ref.py): the
// time planner's layer recursion (tplan.h, §7y) on the pose planner's lattice (pplan.h, §7s).  States are (lattice point, heading
// index, real slot).  The static part is the pose planner's: the body rule's free space and point costs, the directed
// translations, the two turns and their weights.  The clock, the wait and the separation of a body ball from a moving ball over
// one interval are the timed body check's (traj.h, §7x).  The graph is acyclic: layer s depends on layer s + 1 alone, so the bits
// are unique by construction.  The handle copies the lattice geometry, the ball table, the footprint and both caller tables during
// solve(): a result outlives its field, its set and its footprint.
#pragma once
#include "dev_common.h"
#include "body.h"
#include "obst.h"

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

struct TimePosePlanner {
    static constexpr int kMaxHorizon = 1024, kTile = 8, kMaxH = 64, kMaxT = 256;
    static constexpr int kTurnUp = 27, kTurnDown = 28, kWait = 29;
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr long long kMaxStates = 1ll << 30, kMaxStatesKept = 1ll << 28;
    static constexpr float kMaxWait = 1e4f;

    int device = -1;
    hipStream_t own = nullptr;
    int cull = 1;                            // the broad phase (test hook: the results do not depend on it)

    // grow-only device buffers
    unsigned char* d_policy = nullptr; size_t cap_policy = 0;     // [S + 1][ns]
    float* d_c = nullptr;                                          // [ns] point cost; 0 = not free
    float* d_cost0 = nullptr;                                      // [ns] the cost of slot 0
    float* d_lay = nullptr;      size_t cap_n = 0;                 // [2][ns] two cost layers in turn
    float* d_all = nullptr;      size_t cap_all = 0;               // [S + 1][ns] with keep_cost
    double* d_tab = nullptr;                                       // [Obstacles::kMax][kRow]: the solve's copy of the set
    double* d_body = nullptr;                                      // [Footprint::kMax][kRow]: the solve's copy of the footprint
    double* d_head = nullptr;                                      // [kMaxH][2]
    double* d_rot = nullptr;                                       // [kMaxH][Footprint::kMax][2]: the rotated offsets
    unsigned short* d_moves = nullptr;                             // [kMaxH]
    unsigned long long* d_stat = nullptr;
    float* d_goals = nullptr;    size_t cap_goals = 0;
    // paths
    float* d_starts = nullptr;   size_t cap_starts = 0;            // [m][3]
    long long* d_off = nullptr;                                    // [m + 1]
    float* d_scost = nullptr;
    unsigned char* d_status = nullptr;
    float* d_points = nullptr;                                     // [total][2]
    int* d_pheading = nullptr;                                     // [total]
    size_t cap_points = 0;
    // check and controls
    double* d_cd = nullptr;      size_t cap_cd = 0;                // [m][2]
    int* d_ci = nullptr;         size_t cap_ci = 0;                // [m][4]
    double* d_u = nullptr;       size_t cap_u = 0;                 // [m][T][2]
    double* d_hp = nullptr;      size_t cap_hp = 0;                // [m][4]: heading0, p0
    int* d_cl = nullptr;         size_t cap_cl = 0;                // [m]

    // the last result
    bool valid = false, kept = false, paths_valid = false;
    int nx = 0, ny = 0, H = 0, S = 0, n = 0, mb = 0;
    float origin[2] = {0.f, 0.f};
    float step = 0.f;
    long long ns = 0;                        // nx ny H
    TimePosePlanOpts opts;
    double t_begin = 0.0;
    long long goals_given = 0, goals_kept = 0, nfree = 0, nfinite = 0, launches = 0, skipped = 0;
    double solve_ms = 0.0;
    float max_cost0 = 0.f;
    long long npaths = 0, npoints = 0;

    TimePosePlanner();
    ~TimePosePlanner();
    void clear_result() { valid = kept = paths_valid = false; npaths = npoints = 0; }
    int bind(int dev);
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
