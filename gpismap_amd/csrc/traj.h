// Trajectory smoothing through a distance field on the device: a batch of m trajectories of N waypoints, either
// resampled by arc length from a planner's last paths or given by the caller, run through a fixed-order covariant gradient
// descent (smoothness + obstacle term from the field's sampler, the inverse of tridiag(-1, 2, -1) in closed form, a trust
// region) and an evaluation pass that doubles as a collision check.  float32, no FMA; every sum has one order, so the bits are
// those of tests/traj_ref.py.  One workgroup per trajectory, every iteration inside one launch.  The optimiser keeps its input and
// its result apart: a call always starts from the input, and a result outlives the field and the planner it came from.
// On top of a result: speeds and times under speed and acceleration limits, control sequences of the sampling
// controller's model through the timed positions, and one of them written into a controller's nominal sequence on the device;
// the bits are those of tests/timing_ref.py.
// With a footprint the obstacle term acts at the body's balls, the body facing along its chord, and the same
// launch keeps the body's clearance along the result; the bits are those of tests/traj_body_ref.py.
// On top of a timing: a schedule that plays the timed trajectory and pauses it until moving balls have passed,
// and the control sequences, the controller's seed and the check along it; the integers and bits are those of
// tests/retime_ref.py.
// With a footprint against moving balls: the timed check, the re-timing and the check along a schedule take the
// body at its timed pose -- the timed position and the chord rule's heading of the segment it lies on -- and every pair of a body
// ball and a moving ball; the integers and bits are those of tests/body_time_ref.py.
#pragma once
#include <cstdint>
#include <vector>
#include "dev_common.h"

namespace gpis {

struct DistanceField;
struct Planner;
struct PosePlanner;

struct TrajOpts {
    float clearance = 0.f, margin = 1.f, w_smooth = 1.f, w_obs = 0.f, rate = 0.f, max_move = 0.f, tol = 0.f;
    int iters = 0, sub = 0;
};

// the limits of the time parametrisation
struct TimingOpts {
    float v_max = 1.f, v_min = 1.f, a_max = 1.f, d_max = 1.f, a_lat = 0.f, w_max = 0.f, v_start = 0.f, v_end = 0.f, clearance = 0.f,
          slow_dist = 0.f;
};

// the options of a re-timing
struct RetimeOpts {
    double slot = 0.1;       // seconds of a slot, > 0
    int max_pause = 63;      // P: pause slots a schedule may hold, 0 .. 255
    double clearance = 0.0;  // a cell is free while no ball's separation is below it; >= 0
    int press_on = 0;        // 0: pauses as early as the optimum allows, 1: as late
};

struct Controller;
struct Obstacles;
struct BodyArgs;

struct Trajectories {
    static constexpr int kMinN = 3, kMaxN = 256;     // waypoints per trajectory (the reduction tree's width)
    static constexpr int kMaxT = 256;                // steps of a control sequence (the controller's horizon limit)
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

    // the timing of the last result (§7p), dropped wherever the result is
    float* d_tv = nullptr;                           // [m][N] speeds
    float* d_tt = nullptr;                           // [m][N] times
    unsigned char* d_lim = nullptr;                  // [m][N] limiter codes
    size_t cap_tn = 0;
    float* d_tsum = nullptr;                         // [m][3] duration, max speed, max curvature
    int* d_tint = nullptr;                           // [m][9] timing status, waypoints per limiter code
    size_t cap_tm = 0;
    std::vector<int> h_tint;                         // d_tint's host copy
    // the last control sequences
    double* d_cu = nullptr; size_t cap_cu = 0;       // [m][T][nu]
    double* d_chp = nullptr;                         // [m][5] heading0, p_0
    int* d_cclamp = nullptr;                         // [m] clamped steps
    size_t cap_cm = 0;
    double* d_follow = nullptr;                      // [8] heading0, p_0 and the clamped count of the last follow()
    // the last check against moving balls
    double* d_chkd = nullptr;                        // [m][2] min_sep, min_time
    int* d_chki = nullptr;                           // [m][3] min_obstacle, first_hit, collides
    size_t cap_chk = 0;
    // the last check of a footprint along the result
    double* d_bodyd = nullptr;                       // [m] D_min
    int* d_bodyi = nullptr;                          // [m][3] waypoint, ball, collides
    size_t cap_body = 0;
    // the body result of the last optimize() with a footprint
    double* d_bresd = nullptr;                       // [m] D_min
    int* d_bresi = nullptr;                          // [m][3] waypoint, ball, collides
    size_t cap_bres = 0;

    // the schedule of the last re-timing, dropped wherever the timing is; the layout follows the current m alone
    static constexpr int kMaxOwnSlots = 1024;        // own slots a trajectory may last (the position table's rows - 1)
    static constexpr int kMaxPause = 255;            // pause slots (the workgroup's lanes - 1)
    static constexpr int kOwnLen = kMaxOwnSlots + kMaxPause + 1;   // real slots of the longest schedule
    static constexpr int kSchedRes = 5;              // status, arrive, pauses, own_slots, first_pause
    int* d_rres = nullptr;                           // [m][kSchedRes]
    int* d_rown = nullptr;                           // [m][kOwnLen] the own slot of every real slot
    size_t cap_rt = 0;
    std::vector<int> h_rres;                         // d_rres' host copy
    RetimeOpts ropts;                                // the options and the start of the last re-timing
    double r_begin = 0.0;
    bool retimed = false;
    double retime_ms = 0.0;
    int r_body = 0;                                  // body balls of the last re-timing (0: the point's)
    // the last check of a footprint against moving balls, and the last timed poses
    double* d_btd = nullptr;                         // [m][2] min_sep, min_time
    int* d_bti = nullptr;                            // [m][4] min_obstacle, first_hit, collides, min_ball
    size_t cap_bt = 0;
    double* d_bst = nullptr; size_t cap_bst = 0;     // [m][steps + 1][dim + 2]

    int m = 0, N = 0, dim = 0;
    bool has_input = false, valid = false, timed = false;
    bool body_valid = false;                         // the last result came with a footprint: d_bresd, d_bresi hold its body result
    double opt_ms = 0.0, time_ms = 0.0, controls_ms = 0.0;

    Trajectories();
    ~Trajectories();
    int bind(int dev);                               // move to `dev`, the input carried along (the result is dropped)
    // the input from the planner's last paths, N waypoints each; moves to the planner's device; synchronises the own stream
    int from_paths(const Planner& p, int N);
    // the same from a pose planner's last paths (their points; the heading indices are not carried over): a segment of no
    // length -- a turn in place -- gives w = 0
    int from_pose_paths(const PosePlanner& p, int N);
    // the input from host waypoints [m][N][dim]
    int set(const float* x, int m, int N, int dim);
    // descent and evaluation from the input on df's dist; synchronises `s`.  bd: nullptr for the point, else a footprint of this
    // dim on df's device with m > 0 (checked by the caller): the obstacle term acts at its balls, the turn term has the weight
    // w_turn, and the body result is kept
    int optimize(const DistanceField& df, const TrajOpts& o, hipStream_t s, const BodyArgs* bd = nullptr, float w_turn = 0.f);
    // the body result of the last optimize() with a footprint; host outputs [m], any may be nullptr; synchronises the own stream
    int body_result(double* D_min, int* waypoint, int* ball, int* collides);
    // speeds, times and limiter codes of the last result; df: nullptr or a field on this device; s: nullptr for the field's
    // (the own) stream; synchronises it
    int time(const DistanceField* df, const TimingOpts& o, hipStream_t s);
    bool has_timing() const { return valid && timed; }
    // control sequences of T steps for every timed trajectory; host outputs, any may be nullptr; synchronises the own stream
    int controls(double dt, int T, double t0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped);
    // the sequence of trajectory `index` with the controller's T into the current half of its nominal sequence
    int follow(Controller& c, int index, double dt, double t0, double w_limit, double min_move, double* heading0, double* p0);
    // every timed trajectory, sampled at t0 + k dt (k = 0 .. steps) from the absolute time t_begin on, against the balls of
    // `ob` (on this device): the closest approach in continuous time under straight motion between samples; host outputs [m],
    // any may be nullptr.  Arguments are checked by the caller; synchronises the own stream
    int check_obst(const Obstacles& ob, double dt, int steps, double t0, double t_begin, double clearance, double* min_sep,
                   double* min_time, int* min_obstacle, int* first_hit, int* collides);
    // the last result's waypoints with the footprint `bd` (m > 0, on this device) on df's dist, the heading of a waypoint taken
    // from the horizontal chord: host outputs [m], any may be nullptr.  Arguments are checked by the caller; synchronises the
    // own stream
    int check_body(const DistanceField& df, const BodyArgs& bd, double clearance, double* D_min, int* waypoint, int* ball, int* collides);

    // Re-timing (the contract: tests/retime_ref.py).  Own time runs in slots: A = the least a with
    // (double)a * slot >= t_{N-1}, pos_a the timed position at (double)a * slot.  A schedule plays the timed trajectory and
    // pauses it: cell (a, p) -- own slot a after p pauses, real slot a + p -- is left by a play step if no ball's separation
    // from the interval (pos_a, pos_{a+1}) during real slot a + p is below the clearance, by a pause step if none from
    // (pos_a, pos_a) is; the separation is check_obst's expression.  The schedule that arrives first within max_pause pauses is
    // kept per trajectory: status (0 clear as timed, 1 with pauses, 2 no timing, 3 none within max_pause, 4 more than
    // kMaxOwnSlots own slots), arrive, pauses, own_slots, first_pause and own[real slot].  At worst A (P + 1) 2 n separations
    // per trajectory.  Arguments are checked by the caller; s: nullptr for the own stream; synchronises it
    int retime(const Obstacles& ob, const RetimeOpts& o, double t_begin, hipStream_t s);
    bool has_schedule() const { return has_timing() && retimed; }
    // controls() along the schedule from real slot k0 on, dt = the slot: a paused step has no displacement
    int retime_controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped);
    // follow() along the schedule of trajectory `index`
    int retime_follow(Controller& c, int index, int k0, double w_limit, double min_move, double* heading0, double* p0);
    // check_obst() along the schedule from real slot 0 on, the balls taken at the real slots from the schedule's t_begin
    int retime_check(const Obstacles& ob, int steps, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                     int* first_hit, int* collides);

    // The footprint against moving balls (the contract: tests/body_time_ref.py).  The timed pose at tau: the timed
    // position, and the chord rule's heading (check_body's) of the waypoint whose segment the position lies on (the last waypoint
    // from the duration on).  A body ball's centre moves in a straight line between two samples; its separation from a moving
    // ball is check_obst's expression at that centre, less the body ball's radius.  bd: a footprint of this dim on this device
    // with m > 0 (checked by the caller).
    // check_obst() over every (interval, moving ball, body ball); min_ball: the body ball of the least separation
    int check_body_obst(const Obstacles& ob, const BodyArgs& bd, double dt, int steps, double t0, double t_begin, double clearance,
                        double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides);
    // retime() with the cells' flags over every (moving ball, body ball): a pause holds the pose of its own slot, a play step
    // goes from the pose of own slot a to that of a + 1.  The schedule is kept where retime() keeps it
    int retime_body(const Obstacles& ob, const BodyArgs& bd, const RetimeOpts& o, double t_begin, hipStream_t s);
    // retime_check() with the footprint: the pose of own(k) at real slot k
    int retime_body_check(const Obstacles& ob, const BodyArgs& bd, int steps, double clearance, double* min_sep, double* min_time,
                          int* min_obstacle, int* min_ball, int* first_hit, int* collides);
    // the timed poses (p, c, s) [m][steps + 1][dim + 2] at t0 + k dt, or (sched) at own(k) of the schedule with dt its slot; NaN
    // for a trajectory without a timing or a schedule; a host output; synchronises the own stream
    int timed_states(double dt, int steps, double t0, bool sched, double* states);

private:
    int body_time_check(const Obstacles& ob, const BodyArgs& bd, bool sched, double dt, int steps, double t0, double TB, double clearance,
                        double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides);
    int ensure(int m, int N, int dim);
    int from_packed(int dev, long long npaths, long long npoints, int dim, const long long* off, const float* pts,
                    const unsigned char* pstat, int N, bool zero_w);
};

// GPIS_ERR_ARG on anything gpis_traj_optimize documents as an argument error of the options
int traj_check_opts(const TrajOpts& o);
// GPIS_ERR_ARG on anything gpis_timing_time documents as an argument error of the limits
int timing_check_opts(const TimingOpts& o);
// GPIS_ERR_ARG unless dt > 0, 1 <= T <= 256, t0 >= 0, w_limit >= 0, min_move >= 0, all finite
int timing_check_args(double dt, int T, double t0, double w_limit, double min_move);
// GPIS_ERR_ARG unless slot > 0 and clearance >= 0, both finite, 0 <= max_pause <= 255, press_on 0 or 1
int retime_check_opts(const RetimeOpts& o);

}  // namespace gpis
