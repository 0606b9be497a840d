// Shortest collision-free paths through a distance field on the device: a cost-to-go grid over the free space of
// the field's lattice (the greatest fixed point of cost[p] = min over edges fl(cost[q] + w), 0 at the goals), a policy byte per
// point, and the lattice paths from a batch of starts.  float32, no FMA; the fixed point does not depend on the relaxation order,
// so the bits are those of a float32 Dijkstra.  Free iff dist >= clearance: unknown space was made "outside" when the field was
// built and is therefore free.  The planner copies the lattice geometry and reads dist only during solve().
#pragma once
#include <cstdint>
#include "dev_common.h"

namespace gpis {

struct DistanceField;

struct PlanOpts {
    float clearance = 0.f, margin = 0.f, gain = 4.f;
    int connectivity = 1, max_rounds = 0;
};

// The schedule of a solve (test hook: the results do not depend on it): outer rounds per read-back, inner iterations per launch
struct PlanSchedule {
    static constexpr int kMaxBatch = 64;
    int check_every = 8, inner_cap = 256;
    void set(int every, int inner) {             // 0: the default
        check_every = every > 0 ? (every < kMaxBatch ? every : kMaxBatch) : PlanSchedule().check_every;
        inner_cap = inner > 0 ? inner : PlanSchedule().inner_cap;
    }
};

// what a solve leaves besides the arrays; shared by the planner and the pose planner (filled by plan_host.h)
struct PlanCounters {
    long long goals_given = 0, goals_kept = 0, nfree = 0, nreach = 0, rounds = 0, launches = 0;
    double solve_ms = 0.0;
    float max_cost = 0.f;
};

struct Planner {
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr float kMaxGain = 1e4f;
    static constexpr int kTile2 = 32, kTile3 = 8;

    int device = -1;
    hipStream_t own = nullptr;
    PlanSchedule sched;

    // grow-only device buffers, 10 B per lattice point
    float* d_cost = nullptr;
    float* d_c = nullptr;                        // point cost; 0 = not free
    unsigned char* d_policy = nullptr;
    size_t cap_n = 0;
    int* d_flags = nullptr;   size_t cap_tiles = 0;   // [2][tiles]: active this round / next round
    unsigned long long* d_stat = nullptr;        // kStatWords counters (plan_dev.h)
    float* d_goals = nullptr; size_t cap_goals = 0;
    // paths
    float* d_starts = nullptr; size_t cap_starts = 0;    // [m][dim]
    long long* d_off = nullptr;                          // [m + 1]; counts, then their exclusive scan
    float* d_scost = nullptr;
    unsigned char* d_status = nullptr;
    float* d_points = nullptr; size_t cap_points = 0;    // [total][dim]

    // the last result
    int dim = 0;
    int n[3] = {1, 1, 1};
    float origin[3] = {0.f, 0.f, 0.f};
    float step = 0.f;
    long long ngrid = 0;
    bool valid = false;
    PlanCounters cnt;
    bool paths_valid = false;
    long long npaths = 0, npoints = 0;

    Planner();
    ~Planner();
    void clear_result() { valid = paths_valid = false; dim = 0; ngrid = 0; npaths = npoints = 0; }
    int bind(int dev);
    // cost and policy from df's dist; goals: host [ngoals][dim]; synchronises `s`.  GPIS_ERR_LIMIT: max_rounds exceeded.
    int solve(const DistanceField& df, const float* goals, int ngoals, const PlanOpts& o, hipStream_t s);
    // paths from host starts [m][dim]: count, scan, write; synchronises `s`
    int paths(const float* starts, int m, int max_points, hipStream_t s);
    // A 2-D result computed elsewhere (the pose planner's projection, pplan.hip).  install_begin drops the result held, moves
    // to `dev`, makes room for nx x ny points and copies the geometry; the caller then fills d_cost, d_c and d_policy on a
    // stream it synchronises, and install_end records the counters and makes the result valid exactly as solve() does.
    int install_begin(int dev, int nx, int ny, const float* origin2, float lattice_step);
    void install_end(const PlanCounters& c) { cnt = c; valid = true; }

private:
    int ensure(long long np, long long tiles);
};

// GPIS_ERR_ARG on anything gpis_plan_solve documents as an argument error
int plan_check_opts(const PlanOpts& o);

}  // namespace gpis
