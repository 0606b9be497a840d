// Routes through space and time around moving balls on the device (the contract: tests/tplan_ref.py): a planner on
// the time-expanded lattice (lattice point x real slot) of a 2-D field.  The static part is the planner's (plan.h): free space,
// point costs, the translations, their weights and the no-corner-cutting rule; the clock and the separation of a move from a ball
// are the re-timing's (traj.h, §7w).  The graph is acyclic: layer s depends on layer s + 1 alone, so there is no fixed point to
// iterate to and the bits are unique by construction.  The handle copies the lattice geometry and the ball table during solve():
// a result outlives its field and its set.
#pragma once
#include "dev_common.h"
#include "obst.h"

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

struct TimePlanner {
    static constexpr int kMaxHorizon = 1024, kMaxLayers = 16, kLayersNoBalls = 4, kTile = 32, kMaxT = 256;
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr long long kMaxStates = 1ll << 30, kMaxStatesKept = 1ll << 28;
    static constexpr float kMaxWait = 1e4f;

    int device = -1;
    hipStream_t own = nullptr;
    int layers_per_launch = 0, cull = 1;     // the schedule (test hook: the results do not depend on it); 0: chosen per solve

    // grow-only device buffers
    unsigned char* d_policy = nullptr; size_t cap_policy = 0;     // [S + 1][np]
    float* d_c = nullptr;                                          // [np] point cost; 0 = not free
    float* d_cost0 = nullptr;                                      // [np] the cost of slot 0
    float* d_lay = nullptr;      size_t cap_n = 0;                 // [2][np] two cost layers in turn
    float* d_all = nullptr;      size_t cap_all = 0;               // [S + 1][np] with keep_cost
    double* d_tab = nullptr;                                       // [Obstacles::kMax][kRow]: the solve's copy of the set
    unsigned long long* d_stat = nullptr;
    float* d_goals = nullptr;    size_t cap_goals = 0;
    // paths
    float* d_starts = nullptr;   size_t cap_starts = 0;            // [m][2]
    long long* d_off = nullptr;                                    // [m + 1]
    float* d_scost = nullptr;
    unsigned char* d_status = nullptr;
    float* d_points = nullptr;   size_t cap_points = 0;            // [total][2]
    // check and controls
    double* d_cd = nullptr;      size_t cap_cd = 0;                // [m][2]
    int* d_ci = nullptr;         size_t cap_ci = 0;                // [m][3]
    double* d_u = nullptr;       size_t cap_u = 0;                 // [m][T][2]
    double* d_hp = nullptr;      size_t cap_hp = 0;                // [m][4]: heading0, p0
    int* d_cl = nullptr;         size_t cap_cl = 0;                // [m]

    // the last result
    bool valid = false, kept = false, paths_valid = false;
    int nx = 0, ny = 0, S = 0, n = 0;
    float origin[2] = {0.f, 0.f};
    float step = 0.f;
    long long np = 0;
    TimePlanOpts opts;
    double t_begin = 0.0;
    long long goals_given = 0, goals_kept = 0, nfree = 0, nfinite = 0, launches = 0, skipped = 0;
    double solve_ms = 0.0;
    float max_cost0 = 0.f;
    long long npaths = 0, npoints = 0;

    TimePlanner();
    ~TimePlanner();
    void clear_result() { valid = kept = paths_valid = false; npaths = npoints = 0; }
    int bind(int dev);
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
