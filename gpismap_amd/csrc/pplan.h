// Routes for the robot's footprint (the contract: tests/pplan_ref.py): the path planner's solver (plan.h, §7h)
// on the lattice nx x ny x H of poses (x, y, heading), state s = (i, j, h) at index (h ny + j) nx + i.  A state is free iff the
// body rule (body.h, §7r) at its lattice point with the heading (c_h, s_h) gives (float)D >= clearance; its point cost is the
// planner's formula on that float.  Moves are directed: the 8 translations within a layer, each allowed per heading by a bit of
// the caller's table moves[H] and subject to the planner's subset rule in that layer, and the two turns h -> h +- 1 mod H.
// cost = the greatest solution of cost[s] = min over moves s -> s' of fl(cost[s'] + w), 0 at the goals; float32, no FMA; the
// fixed point does not depend on the relaxation order.  project() hands the 2-D summary (min over headings) to a Planner.
// The pose planner copies the lattice geometry and both tables and reads the field and the footprint only during solve().
#pragma once
#include <cstdint>
#include "dev_common.h"
#include "body.h"
#include "plan.h"

namespace gpis {

struct DistanceField;

struct PPlanOpts {
    float clearance = 0.f, margin = 0.f, gain = 4.f, turn = 0.f;
    int max_rounds = 0;
};

struct PosePlanner {
    static constexpr int kMaxStarts = 1 << 24;
    static constexpr long long kMaxStates = 1ll << 28;
    static constexpr float kMaxGain = 1e4f;
    static constexpr int kTile = 8;              // a tile: 8 x 8 lattice points x all H layers
    static constexpr int kMaxH = 64;
    static constexpr int kTurnUp = 27, kTurnDown = 28;

    int device = -1;
    hipStream_t own = nullptr;
    PlanSchedule sched;

    // grow-only device buffers, 9 B per state
    float* d_cost = nullptr;
    float* d_c = nullptr;                        // point cost; 0 = not free
    unsigned char* d_policy = nullptr;
    size_t cap_n = 0;
    int* d_flags = nullptr;   size_t cap_tiles = 0;   // [2][tiles]: active this round / next round
    unsigned long long* d_stat = nullptr;
    double* d_head = nullptr;                    // [kMaxH][2]
    unsigned short* d_moves = nullptr;           // [kMaxH]
    float* d_goals = nullptr; size_t cap_goals = 0;
    unsigned char* d_heading2 = nullptr; size_t cap_n2 = 0;   // the projection's heading per lattice point
    // paths
    float* d_starts = nullptr; size_t cap_starts = 0;    // [m][3]
    long long* d_off = nullptr;                          // [m + 1]; counts, then their exclusive scan
    float* d_scost = nullptr;
    unsigned char* d_status = nullptr;
    float* d_points = nullptr;                           // [total][2]
    int* d_pheading = nullptr;                           // [total]
    size_t cap_points = 0;

    // the last result
    int H = 0;
    int n[2] = {1, 1};
    float origin[2] = {0.f, 0.f};
    float step = 0.f;
    long long nstates = 0;
    double head[kMaxH][2];
    unsigned short moves[kMaxH];
    bool valid = false;
    PlanCounters cnt;
    double setup_ms = 0.0;
    bool paths_valid = false;
    long long npaths = 0, npoints = 0;

    PosePlanner();
    ~PosePlanner();
    void clear_result() { valid = paths_valid = false; H = 0; nstates = 0; npaths = npoints = 0; }
    int bind(int dev);
    // Arguments are checked by the caller (pplan_check_opts, the tables, the goals' headings).  goals: host [ngoals][3];
    // synchronises `s`.  GPIS_ERR_LIMIT: max_rounds exceeded.
    int solve(const DistanceField& df, const Footprint& body, const double* headings, const unsigned short* move_bits, int nh,
              const float* goals, int ngoals, const PPlanOpts& o, hipStream_t s);
    // pose paths from host starts [m][3]: count, scan, write; synchronises `s`
    int paths(const float* starts, int m, int max_points, hipStream_t s);
    // the 2-D summary into `plan`; heading2: host [nx ny] or nullptr.  Runs on this handle's own stream and synchronises it.
    int project(Planner& plan, unsigned char* heading2);
};

// GPIS_ERR_ARG on what gpis_pplan_solve documents as an argument error of the options for a lattice of step `step` (0: the
// lattice is not known, turn is only asked to be positive)
int pplan_check_opts(const PPlanOpts& o, float step);

}  // namespace gpis
