// The host side of the view scorer (view.h): the options past the march's, their checks, the limits of a batch and
// the order table of a scan's beams.  No HIP header, so it can be compiled and run on its own (tests/cpp/view_host_check.cpp).
// The pseudo-angle and the rule's option checks are cover_host.h's: a predicted scan is integrated by the coverage's rule.
#pragma once
#include <limits>
#include "cover_host.h"

namespace gpis {

constexpr long long kViewMaxPoses = 65536;         // poses of one call
constexpr long long kViewMaxRays = 1ll << 26;      // poses x rays of one call

// the options past opts->march (the caller fills that: gpis_render_field_default_opts): the coverage's back_off and max_gap, a
// miss measured one cell short of the march's far end, no distance gate
inline int view_default_tail(int dim, float step, gpis_view_opts* o) {
    CoverOpts c;
    if (!o) return GPIS_ERR_ARG;
    if (int rc = cover_default_opts(dim, step, &c)) return rc;
    o->back_off = c.back_off; o->max_gap = c.max_gap;
    o->miss = o->march.tfar - step;
    o->min_dist = -std::numeric_limits<float>::infinity();
    return GPIS_OK;
}

// GPIS_ERR_ARG: the coverage rule's refusals of back_off / max_gap, a NaN min_dist.  Any miss is legal: one outside the rule's
// window, 0 or NaN says "a ray without a predicted return reveals nothing".  (The march's own options: render_field_check_opts.)
inline int view_check_tail(const gpis_view_opts& o) {
    if (int rc = cover_check_rule(o.back_off, o.max_gap)) return rc;
    return std::isnan(o.min_dist) ? GPIS_ERR_ARG : GPIS_OK;
}

// GPIS_ERR_ARG: m < 1; GPIS_ERR_LIMIT: more than kViewMaxPoses poses or kViewMaxRays poses x rays
inline int view_check_batch(long long m, long long rays) {
    if (m < 1) return GPIS_ERR_ARG;
    if (m > kViewMaxPoses || rays < 0 || (rays > 0 && m > kViewMaxRays / rays)) return GPIS_ERR_LIMIT;
    return GPIS_OK;
}

// What a scan's sector tables need of its n beams and that depends on the angles alone: q[b] = the pseudo-angle of beam b's
// direction (cs[2 b], cs[2 b + 1]), and ord = the beams sorted stably by q.  A stable order of all beams restricted to a pose's
// valid beams is the stable order of those beams, cover_host.h's sector_table's.
inline void view_order_table(const double* cs, long long n, std::vector<double>* q, std::vector<int>* ord) {
    q->resize((size_t)n);
    ord->resize((size_t)n);
    for (long long b = 0; b < n; ++b) (*q)[(size_t)b] = pseudo_angle(cs[2 * b], cs[2 * b + 1]);
    std::iota(ord->begin(), ord->end(), 0);
    const double* t = q->data();
    std::stable_sort(ord->begin(), ord->end(), [t](int a, int b) { return t[a] < t[b]; });
}

}  // namespace gpis
