// The host side of the layered planners, defined once for the time planner (tplan.h) and the time-pose planner (tpplan.h): the
// handle both derive from.  It owns the buffers the two have in common, the statistics words kStat* of d_stat and the fields of
// the last result, and provides the constructor and destructor, bind(), the reservations a solve opens with, the read-back of
// the statistics, and what check() and controls() do around their launches.  The kernels come in as callables or pointers; the
// lattices, the schedules, solve() and paths() are the planners' own.  A base for exactly these two handles.
#pragma once
#include <cstring>
#include <initializer_list>
#include <vector>
#include "dev_common.h"
#include "obst.h"

namespace gpis {

struct TimePlanCore {
    // words of d_stat
    enum { kStatKept = 0, kStatSkipped, kStatFree, kStatFinite, kStatMax, kStatWords };

    int device = -1;
    hipStream_t own = nullptr;
    int cull = 1;                            // the broad phase (test hook: the results do not depend on it)

    // grow-only device buffers; ns = the states of one layer
    unsigned char* d_policy = nullptr; size_t cap_policy = 0;     // [S + 1][ns]
    float* d_c = nullptr;                                          // [ns] point cost; 0 = not free
    float* d_cost0 = nullptr;                                      // [ns] the cost of slot 0
    float* d_lay = nullptr;      size_t cap_n = 0;                 // [2][ns] two cost layers in turn
    float* d_all = nullptr;      size_t cap_all = 0;               // [S + 1][ns] with keep_cost
    double* d_tab = nullptr;                                       // [Obstacles::kMax][kRow]: the solve's copy of the set
    unsigned long long* d_stat = nullptr;
    float* d_goals = nullptr;    size_t cap_goals = 0;
    // paths
    float* d_starts = nullptr;   size_t cap_starts = 0;            // [m][2 or 3]
    long long* d_off = nullptr;                                    // [m + 1]
    float* d_scost = nullptr;
    unsigned char* d_status = nullptr;
    float* d_points = nullptr;   size_t cap_points = 0;            // [total][2]
    // check and controls
    double* d_cd = nullptr;      size_t cap_cd = 0;                // [m][2]: min_sep, min_time
    int* d_ci = nullptr;         size_t cap_ci = 0;                // [m][4]: min_obstacle, first_hit, collides, min_ball
    double* d_u = nullptr;       size_t cap_u = 0;                 // [m][T][2]
    double* d_hp = nullptr;      size_t cap_hp = 0;                // [m][4]: heading0, p0
    int* d_cl = nullptr;         size_t cap_cl = 0;                // [m]

    // the last result
    bool valid = false, kept = false, paths_valid = false;
    int nx = 0, ny = 0, S = 0, n = 0;
    float origin[2] = {0.f, 0.f};
    float step = 0.f;
    long long ns = 0;
    double t_begin = 0.0;
    long long goals_given = 0, goals_kept = 0, nfree = 0, nfinite = 0, launches = 0, skipped = 0;
    double solve_ms = 0.0;
    float max_cost0 = 0.f;
    long long npaths = 0, npoints = 0;

    TimePlanCore() {
        (void)hipGetDevice(&device);
        if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
    }
    ~TimePlanCore() { (void)bind(-1); }

    void clear_result() { valid = kept = paths_valid = false; npaths = npoints = 0; }

    // Moves the handle to device `dev` (-1: to none): frees every buffer and the stream on the old device.  extra: the buffers a
    // derived handle adds, freed and cleared with the rest.
    int bind(int dev, std::initializer_list<void**> extra = {}) {
        if (dev == device && dev >= 0) return GPIS_OK;
        {
            DeviceScope ds(device);
            if (own) (void)hipStreamSynchronize(own);
            const std::initializer_list<void**> mine = {
                (void**)&d_policy, (void**)&d_c,     (void**)&d_cost0,  (void**)&d_lay,    (void**)&d_all, (void**)&d_tab,
                (void**)&d_stat,   (void**)&d_goals, (void**)&d_starts, (void**)&d_off,    (void**)&d_scost, (void**)&d_status,
                (void**)&d_points, (void**)&d_cd,    (void**)&d_ci,     (void**)&d_u,      (void**)&d_hp,  (void**)&d_cl};
            for (const auto& list : {mine, extra})
                for (void** p : list) { (void)hipFree(*p); *p = nullptr; }
            if (own) (void)hipStreamDestroy(own);
        }
        own = nullptr;
        cap_policy = cap_n = cap_all = cap_goals = cap_starts = cap_points = cap_cd = cap_ci = cap_u = cap_hp = cap_cl = 0;
        clear_result();
        device = dev;
        if (dev < 0) return GPIS_OK;
        DeviceScope ds(dev);
        GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        return GPIS_OK;
    }

    // what a solve opens with: room for `states` states per layer, Sn + 1 policy layers (and cost layers with keep_cost), the
    // ball table, the statistics and ngoals goals of `width` floats
    int reserve(long long states, int Sn, int keep_cost, int ngoals, int width) {
        if (!d_stat) GPIS_HIP(hipMalloc((void**)&d_stat, sizeof(unsigned long long) * kStatWords));
        if (!d_tab) GPIS_HIP(hipMalloc((void**)&d_tab, sizeof(double) * Obstacles::kMax * Obstacles::kRow));
        if ((size_t)states > cap_n) {
            for (void* p : {(void*)d_c, (void*)d_cost0, (void*)d_lay}) (void)hipFree(p);
            d_c = d_cost0 = d_lay = nullptr; cap_n = 0;
            GPIS_HIP(hipMalloc((void**)&d_c, sizeof(float) * states));
            GPIS_HIP(hipMalloc((void**)&d_cost0, sizeof(float) * states));
            GPIS_HIP(hipMalloc((void**)&d_lay, sizeof(float) * 2 * states));
            cap_n = (size_t)states;
        }
        if (int rc = grow(d_policy, cap_policy, (size_t)states * (Sn + 1))) return rc;
        if (keep_cost)
            if (int rc = grow(d_all, cap_all, (size_t)states * (Sn + 1))) return rc;
        return grow(d_goals, cap_goals, (size_t)ngoals * width);
    }

    // what a solve closes with, after its finish kernel: the statistics words into the result's fields; synchronises `s`
    int read_stats(hipStream_t s) {
        unsigned long long st[kStatWords];
        GPIS_HIP(hipMemcpyAsync(st, d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
        GPIS_HIP(hipStreamSynchronize(s));
        goals_kept = (long long)st[kStatKept]; skipped = (long long)st[kStatSkipped];
        nfree = (long long)st[kStatFree]; nfinite = (long long)st[kStatFinite];
        const unsigned mbits = (unsigned)st[kStatMax];
        std::memcpy(&max_cost0, &mbits, sizeof(float));
        return GPIS_OK;
    }

    // check(): launch() starts the planner's check kernel on `own`, writing d_cd and d_ci for the npaths last paths; the outputs
    // are host [npaths], any may be null
    template <class Launch>
    int run_check(Launch launch, double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides) {
        const size_t m = (size_t)npaths;
        if (int rc = grow(d_cd, cap_cd, m * 2)) return rc;
        if (int rc = grow(d_ci, cap_ci, m * 4)) return rc;
        launch();
        GPIS_HIP(hipGetLastError());
        std::vector<double> hd(m * 2);
        std::vector<int> hi(m * 4);
        GPIS_HIP(hipMemcpyAsync(hd.data(), d_cd, sizeof(double) * m * 2, hipMemcpyDeviceToHost, own));
        GPIS_HIP(hipMemcpyAsync(hi.data(), d_ci, sizeof(int) * m * 4, hipMemcpyDeviceToHost, own));
        GPIS_HIP(hipStreamSynchronize(own));
        for (size_t k = 0; k < m; ++k) {
            if (min_sep) min_sep[k] = hd[2 * k];
            if (min_time) min_time[k] = hd[2 * k + 1];
            if (min_obstacle) min_obstacle[k] = hi[4 * k];
            if (first_hit) first_hit[k] = hi[4 * k + 1];
            if (collides) collides[k] = hi[4 * k + 2];
            if (min_ball) min_ball[k] = hi[4 * k + 3];
        }
        return GPIS_OK;
    }

    // controls(): `kernel` is the including file's tplan_controls_kernel (tplan_dev.h), width the floats of a start.  U
    // [npaths][T][2], heading0 [npaths][2], p0 [npaths][2], clamped [npaths]: host, any may be null
    template <class Kernel>
    int run_controls(Kernel kernel, int width, double slot, int T, int k0, double w_limit, double min_move, double* U, double* heading0,
                     double* p0, int* clamped) {
        const size_t m = (size_t)npaths;
        if (int rc = grow(d_u, cap_u, m * T * 2)) return rc;
        if (int rc = grow(d_hp, cap_hp, m * 4)) return rc;
        if (int rc = grow(d_cl, cap_cl, m)) return rc;
        const int threads = 64 * ((T + 63) / 64);
        hipLaunchKernelGGL(kernel, dim3((unsigned)m), dim3(threads), 0, own, (const long long*)d_off, (const unsigned char*)d_status,
                           (const float*)d_points, (const float*)d_starts, width, T, k0, slot, w_limit, min_move, d_u, d_hp, d_cl);
        GPIS_HIP(hipGetLastError());
        std::vector<double> hp(m * 4);
        if (U) GPIS_HIP(hipMemcpyAsync(U, d_u, sizeof(double) * m * T * 2, hipMemcpyDeviceToHost, own));
        if (clamped) GPIS_HIP(hipMemcpyAsync(clamped, d_cl, sizeof(int) * m, hipMemcpyDeviceToHost, own));
        GPIS_HIP(hipMemcpyAsync(hp.data(), d_hp, sizeof(double) * m * 4, hipMemcpyDeviceToHost, own));
        GPIS_HIP(hipStreamSynchronize(own));
        for (size_t k = 0; k < m; ++k) {
            if (heading0) { heading0[2 * k] = hp[4 * k]; heading0[2 * k + 1] = hp[4 * k + 1]; }
            if (p0) { p0[2 * k] = hp[4 * k + 2]; p0[2 * k + 1] = hp[4 * k + 3]; }
        }
        return GPIS_OK;
    }
};

}  // namespace gpis
