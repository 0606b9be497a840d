// The host side of the coverage mask (cover.h): the option checks, the diamond pseudo-angle and the sector table of
// a laser scan.  No HIP header, so it can be compiled and run on its own (tests/cpp/cover_host_check.cpp); the kernels include it
// for the pseudo-angle, which host and device must compute alike.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>
#include "../../include/gpismap_amd.h"

#ifdef __HIPCC__
#define GPIS_HD __host__ __device__
#else
#define GPIS_HD
#endif

namespace gpis {

struct CoverOpts {
    float back_off = 0.f, max_gap = 0.f, clearance = 0.f;
    int min_size = 8, max_rounds = 0;
};

inline int cover_default_opts(int dim, float step, CoverOpts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->back_off = step; o->max_gap = (float)(2.0 * (3.14159265358979323846 / 180.0)); o->clearance = 3.f * step;
    o->min_size = 8; o->max_rounds = 0;
    return GPIS_OK;
}

// GPIS_ERR_ARG: back_off negative or non-finite, max_gap outside (0, 90 degrees), clearance non-finite or <= back_off (below that
// every surface would raise a frontier), min_size < 1, max_rounds < 0
// the two options of the integration rule on their own (the view scorer applies the same rule: view_host.h)
inline int cover_check_rule(float back_off, float max_gap) {
    if (!(std::isfinite(back_off) && back_off >= 0.f)) return GPIS_ERR_ARG;
    if (!(std::isfinite(max_gap) && max_gap > 0.f && (double)max_gap < 3.14159265358979323846 / 2)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

inline int cover_check_opts(const CoverOpts& o) {
    if (int rc = cover_check_rule(o.back_off, o.max_gap)) return rc;
    if (!(std::isfinite(o.clearance) && o.clearance > o.back_off)) return GPIS_ERR_ARG;
    if (o.min_size < 1 || o.max_rounds < 0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

// The diamond angle of the direction (c, s): 0 at (1, 0), 1 at (0, 1), 2 at (-1, 0), 3 at (0, -1), monotone in atan2 in between;
// one division, no transcendental.  NaN for (0, 0).
GPIS_HD inline double pseudo_angle(double c, double s) {
    const double p = c / (fabs(c) + fabs(s));
    return s >= 0.0 ? 1.0 - p : 3.0 + p;
}

// Sector k runs from sorted valid beam k to beam k + 1 (the last wraps to the first).  lim_eff folds the three tests the device
// would make on a sector into one number: lim where the sector is narrow and lim > 0, else 0 (nothing is closer than 0).
struct SectorTable {
    std::vector<double> q, lim, lim_eff;
    std::vector<unsigned char> narrow;
    long long size() const { return (long long)q.size(); }
};

// cs: the frame's directions (SensorFrame::cs), ranges [n].  Valid beams: 0.2 < (double)r < 30 (the tracker's window).
inline void sector_table(const double* cs, const float* ranges, long long n, float back_off, float max_gap, SectorTable* t) {
    std::vector<double> q0, c0, s0, r0;
    for (long long k = 0; k < n; ++k) {
        const double r = (double)ranges[k];
        if (!(r > 0.2 && r < 30.0)) continue;
        c0.push_back(cs[2 * k]); s0.push_back(cs[2 * k + 1]); r0.push_back(r);
        q0.push_back(pseudo_angle(cs[2 * k], cs[2 * k + 1]));
    }
    const size_t m = q0.size();
    std::vector<size_t> ord(m);
    std::iota(ord.begin(), ord.end(), (size_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return q0[a] < q0[b]; });
    t->q.resize(m); t->lim.resize(m); t->lim_eff.resize(m); t->narrow.resize(m);
    const double cg = std::cos((double)max_gap), bo = (double)back_off;
    for (size_t k = 0; k < m; ++k) t->q[k] = q0[ord[k]];
    for (size_t k = 0; k < m; ++k) {
        const size_t a = ord[k], b = ord[k + 1 < m ? k + 1 : 0];
        const double dq = k + 1 < m ? t->q[k + 1] - t->q[k] : (t->q[0] + 4.0) - t->q[k];
        const double dot = c0[a] * c0[b] + s0[a] * s0[b];
        t->lim[k] = std::min(r0[a], r0[b]) - bo;
        t->narrow[k] = (dq < 2.0 && dot >= cg) ? 1 : 0;
        t->lim_eff[k] = (t->narrow[k] && t->lim[k] > 0.0) ? t->lim[k] : 0.0;
    }
}

// the sector of the pseudo-angle ql among the m >= 1 sorted q: the last k with q[k] <= ql, the wrapping one if there is none
GPIS_HD inline int sector_of(const double* q, int m, double ql) {
    int lo = 0, hi = m;                      // the first k with q[k] > ql
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] <= ql) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : m - 1;
}

}  // namespace gpis
