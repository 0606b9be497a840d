// The host side of the solver's rule, defined once for the path planner (plan.hip) and the pose planner (pplan.hip): the outer
// rounds of a solve, the counters a solve leaves, and the count / scan / write sequence of paths().  The handles keep their own
// buffers and pass them by reference; the kernels come in as callables.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include "plan_dev.h"

namespace gpis {
namespace plan_host {

// Outer rounds until one raises no flag.  launch(cur, nxt, raised_word) starts one round's tile kernel on `s`; d_flags: [2][tiles],
// round r reads half r & 1 and raises in the other; d_raised: kMaxBatch words.  One read-back per sch.check_every rounds.
// Returns the number of rounds, GPIS_ERR_LIMIT after `cap` rounds, or GPIS_ERR_HIP.
template <class Launch>
long long run_rounds(hipStream_t s, int* d_flags, long long tiles, unsigned long long* d_raised, long long cap, const PlanSchedule& sch,
                     Launch launch) {
    unsigned long long raised[PlanSchedule::kMaxBatch];
    for (long long round = 0; round < cap;) {
        const int nb = (int)std::min((long long)sch.check_every, cap - round);
        GPIS_HIP(hipMemsetAsync(d_raised, 0, sizeof(unsigned long long) * nb, s));
        for (int b = 0; b < nb; ++b) {
            launch(d_flags + ((round + b) & 1) * tiles, d_flags + ((round + b + 1) & 1) * tiles, d_raised + b);
            GPIS_HIP(hipGetLastError());
        }
        GPIS_HIP(hipMemcpyAsync(raised, d_raised, sizeof(unsigned long long) * nb, hipMemcpyDeviceToHost, s));
        GPIS_HIP(hipStreamSynchronize(s));
        for (int b = 0; b < nb; ++b)
            if (raised[b] == 0) return round + b + 1;       // (the rounds after it found every flag down)
        round += nb;
    }
    return GPIS_ERR_LIMIT;
}

// The counters from the first kStatRaised words of d_stat, read back by the caller; free_word: kStatFree after a solve's policy
// kernel, kStatFree2 after the projection's
inline PlanCounters counters(const unsigned long long* st, int free_word, long long given, long long rounds, double ms) {
    PlanCounters c;
    c.goals_given = given; c.goals_kept = (long long)st[plan_dev::kStatKept];
    c.nfree = (long long)st[free_word]; c.nreach = (long long)st[free_word + 1];
    c.rounds = rounds; c.launches = (long long)st[plan_dev::kStatLaunch]; c.solve_ms = ms;
    const unsigned mb = (unsigned)st[free_word + 2];
    std::memcpy(&c.max_cost, &mb, sizeof(float));
    return c;
}

// paths(): the m starts (host, `width` floats each) go to the device, count_walk() leaves the path lengths in d_off, the scan
// turns them into offsets, grow_points(total) makes room (int: GPIS_OK or an error), write_walk() stores the points.  The start
// buffers grow exactly to the need and never shrink.  Synchronises `s`.
template <class Count, class Grow, class Write>
int run_paths(hipStream_t s, const float* starts, int m, int width, float*& d_starts, size_t& cap_starts, long long*& d_off, float*& d_scost,
              unsigned char*& d_status, long long& total, Count count_walk, Grow grow_points, Write write_walk) {
    if ((size_t)m > cap_starts) {
        for (void* p : {(void*)d_starts, (void*)d_off, (void*)d_scost, (void*)d_status}) (void)hipFree(p);
        d_starts = nullptr; d_off = nullptr; d_scost = nullptr; d_status = nullptr; cap_starts = 0;
        GPIS_HIP(hipMalloc((void**)&d_starts, sizeof(float) * 3 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_off, sizeof(long long) * ((size_t)m + 1)));
        GPIS_HIP(hipMalloc((void**)&d_scost, sizeof(float) * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_status, (size_t)m));
        cap_starts = (size_t)m;
    }
    GPIS_HIP(hipMemcpyAsync(d_starts, starts, sizeof(float) * (size_t)m * width, hipMemcpyHostToDevice, s));
    count_walk();
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(plan_dev::plan_scan_kernel, dim3(1), dim3(1024), 0, s, d_off, m);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(&total, d_off + m, sizeof(long long), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    if (int rc = grow_points((size_t)std::max(1ll, total))) return rc;
    write_walk();
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}

}  // namespace plan_host
}  // namespace gpis
