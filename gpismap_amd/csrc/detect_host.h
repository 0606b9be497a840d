// The host side of the moving-obstacle detector (detect.h): the options and their checks, the selection of the
// components that become balls, and the tracks that give the balls their velocities.  Plain C++ on arrays, all arithmetic double
// and written left to right as tests/detect_ref.py evaluates it.  No HIP header, so it can be compiled and run on its own
// (tests/cpp/detect_host_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/gpismap_amd.h"

namespace gpis {

constexpr int kDetectMaxBalls = 256;         // Obstacles::kMax (detect.hip asserts it)

struct DetectOpts {
    double min_dist = 0.0;       // a sample is foreign iff d is finite and (double)d >= min_dist
    double link = 0.0;           // neighbouring foreign samples are linked iff |x - y|^2 <= link * link
    double pad = 0.0;            // radius = sqrt(r2) + pad
    double max_radius = 0.0;     // components with sqrt(r2) > max_radius are no balls
    double gate = 0.0;           // association: |c_j - (c_i + v_i dt)| <= gate + max_speed * dt
    double max_speed = 0.0;
    double alpha = 1.0;          // v = alpha * v_raw + (1 - alpha) * v_i; in (0, 1]
    int min_points = 1;          // components of fewer samples are noise
    int max_missed = 0;          // a track coasts for at most this many calls without a match
    int stride = 1;              // 3-D: the tracker's pixel stride; ignored in 2-D
    int max_rounds = 0;          // labelling rounds, 0 = until converged
};

// Defaults (in lattice steps, stored in metres as (double)(k * step) with the product in float): min_dist 2, link 3, pad 1,
// gate 4 steps; max_radius 1 m, max_speed 2 m/s, alpha 0.5, min_points 3, max_missed 2, stride 1 (2-D) / 2 (3-D), max_rounds 0.
inline int detect_default_opts(int dim, float step, DetectOpts* o) {
    if (!o || (dim != 2 && dim != 3) || !(std::isfinite(step) && step > 0.f)) return GPIS_ERR_ARG;
    o->min_dist = (double)(2.f * step); o->link = (double)(3.f * step); o->pad = (double)(1.f * step); o->gate = (double)(4.f * step);
    o->max_radius = 1.0; o->max_speed = 2.0; o->alpha = 0.5;
    o->min_points = 3; o->max_missed = 2; o->stride = dim == 3 ? 2 : 1; o->max_rounds = 0;
    return GPIS_OK;
}

// GPIS_ERR_ARG: a non-finite or negative option, alpha outside (0, 1], stride < 1, min_points < 1
inline int detect_check_opts(const DetectOpts& o) {
    for (double v : {o.min_dist, o.link, o.pad, o.max_radius, o.gate, o.max_speed})
        if (!(std::isfinite(v) && v >= 0.0)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.alpha) && o.alpha > 0.0 && o.alpha <= 1.0)) return GPIS_ERR_ARG;
    if (o.stride < 1 || o.min_points < 1 || o.max_missed < 0 || o.max_rounds < 0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

// ---- selection ------------------------------------------------------------------------------------------------------------
enum { kDetBall = 0, kDetNoise = 1, kDetLarge = 2, kDetDropped = 3 };

// Components in label order (count, r2).  flag[c]: noise (count < min_points), too large (sqrt(r2) > max_radius), else a ball,
// or dropped for the cap: of the candidates the kDetectMaxBalls of the largest counts are kept, ties by the lower label (= the
// lower index).  sel: the indices of the balls, ascending.
inline void detect_select(int nc, const int* count, const double* r2, const DetectOpts& o, std::vector<int>* flag, std::vector<int>* sel) {
    flag->assign((size_t)nc, kDetBall);
    std::vector<int> cand;
    for (int c = 0; c < nc; ++c) {
        if (count[c] < o.min_points) (*flag)[c] = kDetNoise;
        else if (std::sqrt(r2[c]) > o.max_radius) (*flag)[c] = kDetLarge;
        else cand.push_back(c);
    }
    if ((int)cand.size() > kDetectMaxBalls) {
        std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return count[a] > count[b]; });
        for (size_t k = kDetectMaxBalls; k < cand.size(); ++k) (*flag)[cand[k]] = kDetDropped;
        cand.resize(kDetectMaxBalls);
        std::sort(cand.begin(), cand.end());
    }
    *sel = cand;
}

// ---- tracks ---------------------------------------------------------------------------------------------------------------
struct DetBall {
    double c[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, r = 0.0;
    int id = 0, age = 0, missed = 0;
    int comp = -1;               // index into the component table; -1: a coasting ball
};

struct DetTracks {
    std::vector<DetBall> balls;  // the balls of the previous call, detected ones first
    double t_prev = 0.0;
    bool held = false;           // a call has succeeded since the last reset
    int next_id = 0;
    void reset() { balls.clear(); held = false; t_prev = 0.0; }
};

// One call at time t > t_prev (checked by the caller): `det` holds the detected balls (c, r, comp set) in label order.  Returns
// the new ball list: the detected ones with velocity, id and age, then the unmatched old ones that still coast, in id order,
// while there is room below kDetectMaxBalls.  Updates tr.
inline std::vector<DetBall> detect_associate(int dim, std::vector<DetBall> det, double t, const DetectOpts& o, DetTracks* tr) {
    const std::vector<DetBall>& old = tr->balls;
    const int no = tr->held ? (int)old.size() : 0, nn = (int)det.size();
    const double dt = tr->held ? t - tr->t_prev : 0.0;
    struct Pair { double d; int i, j; };
    std::vector<Pair> pairs;
    const double lim = o.gate + o.max_speed * dt;
    for (int i = 0; i < no; ++i)
        for (int j = 0; j < nn; ++j) {
            double s = 0.0;
            for (int a = 0; a < dim; ++a) {
                const double e = det[j].c[a] - (old[i].c[a] + old[i].v[a] * dt);
                s = s + e * e;
            }
            const double d = std::sqrt(s);
            if (d <= lim) pairs.push_back(Pair{d, i, j});
        }
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) {
        if (a.d != b.d) return a.d < b.d;
        if (a.i != b.i) return a.i < b.i;
        return a.j < b.j;
    });
    std::vector<int> of_old((size_t)no, -1), of_new((size_t)nn, -1);
    for (const Pair& p : pairs)
        if (of_old[p.i] < 0 && of_new[p.j] < 0) { of_old[p.i] = p.j; of_new[p.j] = p.i; }
    for (int j = 0; j < nn; ++j) {
        DetBall& b = det[j];
        if (of_new[j] >= 0) {
            const DetBall& p = old[of_new[j]];
            for (int a = 0; a < dim; ++a) {
                const double vr = (b.c[a] - p.c[a]) / dt;
                b.v[a] = p.age == 0 ? vr : o.alpha * vr + (1.0 - o.alpha) * p.v[a];
            }
            b.id = p.id; b.age = p.age + 1;
        } else {
            for (int a = 0; a < dim; ++a) b.v[a] = 0.0;
            b.id = tr->next_id++; b.age = 0;
        }
        b.missed = 0;
    }
    std::vector<DetBall> coast;
    for (int i = 0; i < no; ++i) {
        if (of_old[i] >= 0 || old[i].missed + 1 > o.max_missed) continue;
        DetBall b = old[i];
        for (int a = 0; a < dim; ++a) b.c[a] = old[i].c[a] + old[i].v[a] * dt;
        b.missed = old[i].missed + 1; b.comp = -1;
        coast.push_back(b);
    }
    std::sort(coast.begin(), coast.end(), [](const DetBall& a, const DetBall& b) { return a.id < b.id; });
    for (const DetBall& b : coast)
        if ((int)det.size() < kDetectMaxBalls) det.push_back(b);
    tr->balls = det; tr->t_prev = t; tr->held = true;
    return det;
}

}  // namespace gpis
