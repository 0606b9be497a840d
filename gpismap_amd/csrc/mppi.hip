// The sampling controller on the device (mppi.h; the contract: tests/mppi_ref.py).  Per step, four launches:
// the rollouts (one thread per rollout, 64-thread workgroups: T serial steps of U Philox blocks, the unicycle / body-frame
// model, the Cayley heading, one field sample; J, the hit count and the block's minimum of J), the weights (every workgroup
// reduces the block minima itself, then q = floor(exp(-(J - Jmin) / lambda) 2^32) with the block's integer totals and best
// key), the update's terms (a workgroup per 256-rollout segment and 8 (t, u) columns: every thread regenerates its clamped
// perturbation from the counter and the old Ubar, then the tracker's segment tree), and one top workgroup (the integer totals,
// the tree over the segment partials, the new Ubar into the other half of the ping-pong buffer, the nominal rollout by one
// thread, the stats block).  No kernel waits on another workgroup; no atomics; every double expression is written left to right
// as the reference states it (-ffp-contract=off).
#include <chrono>
#include <cmath>
#include <cstring>
#include "dfield.h"
#include "plan.h"
#include "mppi.h"
#include "obst.h"
#include "body.h"
#include "block_ops.h"
#include "philox.h"

namespace gpis {

namespace {

typedef unsigned long long u64;
constexpr int kBlock = Controller::kBlock, kRollBlock = Controller::kRollBlock, kCols = Controller::kCols;
constexpr double kTwo32 = 4294967296.0;
constexpr uint32_t kTag = 2u;            // the counter's last word: 0 and 1 are the particle filter's
constexpr int kSums = 5;                 // block partials of the weigh kernel: q, q >> 16, (q >> 16)^2, hit > 0, the best key

struct MppiParams {
    double dt, half_dt, gamma, lambda;
    double sigma[4], umin[4], umax[4];
    double clearance, band, margin;      // band = clearance + margin
    double w_obs, w_col, w_off, w_goal;
    double start[5], goal[3];
    int K, T, use_plan;
    uint32_t tick, k0, k1;
};

// the clamped control and its perturbation of rollout k at column t * U + u
__device__ __forceinline__ double mppi_control(uint32_t k, uint32_t col, double ub, double sigma, double lo, double hi, const MppiParams& p,
                                               double* __restrict__ du) {
    const double z = k == 0u ? 0.0 : philox_deviate(k, p.tick, col, kTag, p.k0, p.k1);
    const double e = sigma * z;
    double v = ub + e;
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    *du = v - ub;
    return v;
}

// The least separation of a position from the moving balls (obst.h) at elapsed time e: the minimum over i
// ascending, from +inf.  Where the index and e are the same in every lane the table's rows come through scalar loads.
template <int D>
__device__ __forceinline__ double obst_least_sep(const ObstArgs* ob, const double* pos, double e) {
    const double* __restrict__ row = ob->tab;
    double Dm = INFINITY;
    for (int i = 0; i < ob->n; ++i, row += Obstacles::kRow) {
        const double q0 = pos[0] - (row[0] + row[3] * e);
        const double q1 = pos[1] - (row[1] + row[4] * e);
        double s2 = q0 * q0;
        s2 = s2 + q1 * q1;
        if constexpr (D == 3) {
            const double q2 = pos[2] - (row[2] + row[5] * e);
            s2 = s2 + q2 * q2;
        }
        const double sep = sqrt(s2) - row[6];
        Dm = sep < Dm ? sep : Dm;
    }
    return Dm;
}

// The least separation of a body (body.h) at position pos with the heading (c, s) from the moving balls at elapsed
// time e: sep_j = obst_least_sep(w_j, e) - rho_j per body ball j ascending, the minimum from +inf by the same strict comparison.
template <int D>
__device__ __forceinline__ double body_least_sep(const ObstArgs* ob, const BodyArgs* bd, const double* pos, double c, double s, double e) {
    const double* __restrict__ row = bd->tab;
    double Dm = INFINITY;
    for (int j = 0; j < bd->m; ++j, row += Footprint::kRow) {
        double w[3] = {0.0, 0.0, 0.0};
        body_ball_at<D>(row, pos, c, s, w);
        const double sep = obst_least_sep<D>(ob, w, e) - row[3];
        Dm = sep < Dm ? sep : Dm;
    }
    return Dm;
}

// One rollout: the T steps, the stage and control costs, the terminal term.  Ubar is read through a plain pointer: the top
// kernel rolls the sequence it has just written.  OBST = 1 adds the moving balls' term at every new position; OBST = 2 adds it
// with each step's least separation taken from sep_in[t] (the top kernel has them from a thread per step).  BODY = 1 puts the
// body rule's D (body.h) at the new position and the new heading in the place of the point's sampled distance, and takes the
// balls' separation from the body's balls; BODY = 2 takes each step's D from d_in[t] (the top kernel's thread per step).
// lim: nullptr, or the workgroup's LDS copy of the constants the loop reads -- [3][4] sigma, umin and umax, then clearance, band,
// margin, w_obs, w_col, w_off and the set's clearance, band, margin, w_obs, w_col: the body rollouts keep them out of the scalar
// registers, which the two tables' rows need.
template <int D, bool STATES, int OBST = 0, int BODY = 0>
__device__ __forceinline__ void mppi_roll(uint32_t k, const float* __restrict__ F, const DfLattice& L, const float* __restrict__ cost,
                                          const double* Ubar, const MppiParams& p, double* states, double* __restrict__ Jout,
                                          int* __restrict__ hout, const ObstArgs* ob = nullptr, int* __restrict__ dyn_out = nullptr,
                                          double* __restrict__ sep_out = nullptr, const double* sep_in = nullptr,
                                          const BodyArgs* bd = nullptr, const double* d_in = nullptr, const double* lim = nullptr) {
    constexpr int U = D == 3 ? 4 : 2, NS = D + 2;
    DfLattice Lc = L;
    Lc.dim = D;                                          // (a constant dim keeps the sampler's output in registers)
    double pos[3] = {p.start[0], p.start[1], D == 3 ? p.start[2] : 0.0};
    double c = p.start[D], s = p.start[D + 1];
    double J = 0.0;
    int hits = 0;
    int dyn = 0;
    double msep = INFINITY;
    if constexpr (STATES) {
#pragma unroll
        for (int a = 0; a < D; ++a) states[a] = pos[a];
        states[D] = c; states[D + 1] = s;
    }
    for (int t = 0; t < p.T; ++t) {
        double v[U], acc = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double ub = Ubar[t * U + u];
            double du;
            if constexpr (BODY == 1) {
                const double sg = lim[u];
                v[u] = mppi_control(k, (uint32_t)(t * U + u), ub, sg, lim[4 + u], lim[8 + u], p, &du);
                if (sg > 0.0) acc = acc + (ub * du) / (sg * sg);
            } else {
                v[u] = mppi_control(k, (uint32_t)(t * U + u), ub, p.sigma[u], p.umin[u], p.umax[u], p, &du);
                if (p.sigma[u] > 0.0) acc = acc + (ub * du) / (p.sigma[u] * p.sigma[u]);
            }
        }
        // translation with the heading from before the step
        const double bx = v[0] * p.dt;
        if constexpr (D == 2) {
            pos[0] = pos[0] + c * bx;
            pos[1] = pos[1] + s * bx;
        } else {
            const double by = v[1] * p.dt;
            pos[0] = pos[0] + (c * bx - s * by);
            pos[1] = pos[1] + (s * bx + c * by);
            pos[2] = pos[2] + v[2] * p.dt;
        }
        // heading: the Cayley map of half the turn
        const double a = p.half_dt * v[U - 1];
        const double den = 1.0 + a * a;
        const double cn = (1.0 - a * a) / den, sn = (a + a) / den;
        const double c1 = c * cn - s * sn, s1 = s * cn + c * sn;
        const double n = sqrt(c1 * c1 + s1 * s1);
        c = c1 / n; s = s1 / n;
        if constexpr (STATES) {
            double* S = states + (size_t)(t + 1) * NS;
#pragma unroll
            for (int q = 0; q < D; ++q) S[q] = pos[q];
            S[D] = c; S[D + 1] = s;
        }
        // stage cost
        double d;
        if constexpr (BODY == 2) d = d_in[t];
        else if constexpr (BODY == 1) {
            d = body_clearance_at<D>(F, Lc, bd->tab, bd->m, pos, c, s);
        } else {
            float o[1 + D];
            df_sample_at(F, Lc, (float)pos[0], (float)pos[1], D == 3 ? (float)pos[2] : 0.f, o);
            d = (double)o[0];
        }
        const double clr = BODY == 1 ? lim[12] : p.clearance, band = BODY == 1 ? lim[13] : p.band;
        const double margin = BODY == 1 ? lim[14] : p.margin, w_obs = BODY == 1 ? lim[15] : p.w_obs;
        const double w_col = BODY == 1 ? lim[16] : p.w_col, w_off = BODY == 1 ? lim[17] : p.w_off;
        double j = 0.0;
        if (d != d) j = w_off;
        else if (d < clr) { j = w_col; hits += 1; }
        else if (d < band) {
            const double r = (band - d) / margin;
            j = (w_obs * r) * r;
        }
        const double g = p.gamma * acc;
        if constexpr (OBST) {
            double Dm;
            if constexpr (OBST == 2) Dm = sep_in[t];
            else if constexpr (BODY) Dm = body_least_sep<D>(ob, bd, pos, c, s, ob->E0 + ((double)(t + 1) * p.dt));
            else Dm = obst_least_sep<D>(ob, pos, ob->E0 + ((double)(t + 1) * p.dt));
            const double oclr = BODY == 1 ? lim[18] : ob->clearance, oband = BODY == 1 ? lim[19] : ob->band;
            const double omargin = BODY == 1 ? lim[20] : ob->margin, ow_obs = BODY == 1 ? lim[21] : ob->w_obs;
            const double ow_col = BODY == 1 ? lim[22] : ob->w_col;
            double jd = 0.0;
            if (Dm < oclr) { jd = ow_col; dyn += 1; }
            else if (Dm < oband) {
                const double r = (oband - Dm) / omargin;
                jd = (ow_obs * r) * r;
            }
            msep = Dm < msep ? Dm : msep;
            J = ((J + j) + jd) + g;
        } else {
            J = (J + j) + g;
        }
    }
    // terminal term
    if (p.use_plan) {
        const float st = L.st;
        const float ux = ((float)pos[0] - L.ox) / st, uy = ((float)pos[1] - L.oy) / st, uz = D == 3 ? ((float)pos[2] - L.oz) / st : 0.f;
        const bool in = (ux >= 0.f && ux <= (float)(L.nx - 1)) && (uy >= 0.f && uy <= (float)(L.ny - 1)) &&
                        (D == 2 || (uz >= 0.f && uz <= (float)(L.nz - 1)));
        if (!in) J = J + p.w_off;
        else {
            const int ix = min((int)floorf(ux + 0.5f), L.nx - 1), iy = min((int)floorf(uy + 0.5f), L.ny - 1);
            const int iz = D == 3 ? min((int)floorf(uz + 0.5f), L.nz - 1) : 0;
            const float G = cost[((long long)iz * L.ny + iy) * L.nx + ix];
            if (isinf(G)) J = J + p.w_col;
            else J = J + p.w_goal * (double)G;
        }
    } else {
        double s2 = (pos[0] - p.goal[0]) * (pos[0] - p.goal[0]);
        s2 = s2 + (pos[1] - p.goal[1]) * (pos[1] - p.goal[1]);
        if constexpr (D == 3) s2 = s2 + (pos[2] - p.goal[2]) * (pos[2] - p.goal[2]);
        J = J + p.w_goal * sqrt(s2);
    }
    *Jout = J;
    *hout = hits;
    if constexpr (OBST) { *dyn_out = dyn; *sep_out = msep; }
}

template <int D>
__global__ void __launch_bounds__(kRollBlock) mppi_rollout_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                                  const double* __restrict__ Ubar, MppiParams p, double* __restrict__ J,
                                                                  int* __restrict__ hits, double* __restrict__ bmin) {
    __shared__ double sh[1];
    const int k = (int)(blockIdx.x * kRollBlock + threadIdx.x);
    double v = INFINITY;
    if (k < p.K) {
        int h;
        mppi_roll<D, false>((uint32_t)k, F, L, cost, Ubar, p, nullptr, &v, &h);
        J[k] = v;
        hits[k] = h;
    }
    v = block_reduce(v, OpMin(), sh, kRollBlock, (double)INFINITY);
    if (threadIdx.x == 0) bmin[blockIdx.x] = v;
}

// the same with the moving balls' term: also the rollout's count of steps nearer than the set's clearance, its least separation
// and the block's number of rollouts with such a step (an integer sum: order-free)
template <int D>
__global__ void __launch_bounds__(kRollBlock) mppi_obst_rollout_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                                       const double* __restrict__ Ubar, MppiParams p, ObstArgs ob,
                                                                       double* __restrict__ J, int* __restrict__ hits,
                                                                       double* __restrict__ bmin, int* __restrict__ dyn,
                                                                       double* __restrict__ msep, int* __restrict__ bdyn) {
    __shared__ double sh[1];
    __shared__ int shi[1];
    const int k = (int)(blockIdx.x * kRollBlock + threadIdx.x);
    double v = INFINITY;
    int any = 0;
    if (k < p.K) {
        int h, dh;
        double ms;
        mppi_roll<D, false, 1>((uint32_t)k, F, L, cost, Ubar, p, nullptr, &v, &h, &ob, &dh, &ms);
        J[k] = v;
        hits[k] = h;
        dyn[k] = dh;
        msep[k] = ms;
        any = dh > 0 ? 1 : 0;
    }
    v = block_reduce(v, OpMin(), sh, kRollBlock, (double)INFINITY);
    any = block_reduce(any, OpAdd(), shi, kRollBlock, 0);
    if (threadIdx.x == 0) { bmin[blockIdx.x] = v; bdyn[blockIdx.x] = any; }
}

// the rollouts of a robot with a footprint (body.h): the body rule at every new state; OBST: with the moving
// balls' term taken at the body's balls, and the outputs of mppi_obst_rollout_kernel (the pointers are not read without it)
template <int D, bool OBST>
__global__ void __launch_bounds__(kRollBlock) mppi_body_rollout_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                                       const double* __restrict__ Ubar, MppiParams p, BodyArgs bd, ObstArgs ob,
                                                                       double* __restrict__ J, int* __restrict__ hits,
                                                                       double* __restrict__ bmin, int* __restrict__ dyn,
                                                                       double* __restrict__ msep, int* __restrict__ bdyn) {
    __shared__ double sh[1];
    __shared__ int shi[1];
    __shared__ double lim[23];
    if (threadIdx.x == 0) {
        lim[12] = p.clearance; lim[13] = p.band; lim[14] = p.margin; lim[15] = p.w_obs; lim[16] = p.w_col; lim[17] = p.w_off;
        lim[18] = ob.clearance; lim[19] = ob.band; lim[20] = ob.margin; lim[21] = ob.w_obs; lim[22] = ob.w_col;
        lim[0] = p.sigma[0]; lim[1] = p.sigma[1]; lim[2] = p.sigma[2]; lim[3] = p.sigma[3];
        lim[4] = p.umin[0]; lim[5] = p.umin[1]; lim[6] = p.umin[2]; lim[7] = p.umin[3];
        lim[8] = p.umax[0]; lim[9] = p.umax[1]; lim[10] = p.umax[2]; lim[11] = p.umax[3];
    }
    __syncthreads();
    const int k = (int)(blockIdx.x * kRollBlock + threadIdx.x);
    double v = INFINITY;
    int any = 0;
    if (k < p.K) {
        int h;
        if constexpr (OBST) {
            int dh;
            double ms;
            mppi_roll<D, false, 1, 1>((uint32_t)k, F, L, cost, Ubar, p, nullptr, &v, &h, &ob, &dh, &ms, nullptr, &bd, nullptr, lim);
            dyn[k] = dh;
            msep[k] = ms;
            any = dh > 0 ? 1 : 0;
        } else {
            mppi_roll<D, false, 0, 1>((uint32_t)k, F, L, cost, Ubar, p, nullptr, &v, &h, nullptr, nullptr, nullptr, nullptr, &bd, nullptr, lim);
        }
        J[k] = v;
        hits[k] = h;
    }
    v = block_reduce(v, OpMin(), sh, kRollBlock, (double)INFINITY);
    if (threadIdx.x == 0) bmin[blockIdx.x] = v;
    if constexpr (OBST) {
        any = block_reduce(any, OpAdd(), shi, kRollBlock, 0);
        if (threadIdx.x == 0) bdyn[blockIdx.x] = any;
    }
}

// ---- block reductions (block_ops.h: block_reduce) of order-free operations only: min of doubles without NaN, integer sums and
// minima ------------------------------------------------------------------------------------------------------------------------
// Jmin from the block minima (every workgroup for itself), then q and the block's integer partials
__global__ void __launch_bounds__(kBlock) mppi_weigh_kernel(const double* __restrict__ J, const int* __restrict__ hits, int K, int nbr,
                                                            int nb, const double* __restrict__ bmin, double lambda,
                                                            u64* __restrict__ q, u64* __restrict__ bsum, MppiStats* __restrict__ st) {
    __shared__ double shd[kBlock / kWave];
    __shared__ u64 sh[kBlock / kWave];
    __shared__ double jmin_s;
    double m = INFINITY;
    for (int b = threadIdx.x; b < nbr; b += kBlock) m = OpMin()(m, bmin[b]);
    m = block_reduce(m, OpMin(), shd, kBlock, (double)INFINITY);
    if (threadIdx.x == 0) jmin_s = m;
    __syncthreads();
    const double jmin = jmin_s;
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    u64 v = 0, hit = 0, key = ~0ull;
    if (i < K) {
        const double Ji = J[i];
        const double w = exp(-((Ji - jmin) / lambda));
        v = (u64)floor(w * kTwo32);
        q[i] = v;
        hit = hits[i] > 0 ? 1ull : 0ull;
        if (Ji == jmin) key = (u64)i;
    }
    const u64 h = v >> 16;
    const u64 t = block_reduce(v, OpAdd(), sh, kBlock, 0ull);
    const u64 th = block_reduce(h, OpAdd(), sh, kBlock, 0ull);
    const u64 s2 = block_reduce(h * h, OpAdd(), sh, kBlock, 0ull);
    const u64 nh = block_reduce(hit, OpAdd(), sh, kBlock, 0ull);
    const u64 kb = block_reduce(key, OpMin(), sh, kBlock, ~0ull);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = t; bsum[(size_t)nb + blockIdx.x] = th; bsum[2 * (size_t)nb + blockIdx.x] = s2;
        bsum[3 * (size_t)nb + blockIdx.x] = nh; bsum[4 * (size_t)nb + blockIdx.x] = kb;
        if (blockIdx.x == 0) st->jmin = jmin;
    }
}

// ---- the update: the tracker's tree (block_ops.h: segment_reduce and tree_top state the order) -------------------------------
// the terms (double)q * d_u of kCols columns and their sums per segment; d_u regenerated from the counter and the old Ubar
template <int D>
__global__ void __launch_bounds__(kBlock) mppi_update_kernel(const double* __restrict__ Ubar, const u64* __restrict__ q, MppiParams p,
                                                             int nseg_pow2, double* __restrict__ part) {
    constexpr int U = D == 3 ? 4 : 2;
    static_assert(kCols % U == 0, "a chunk of columns starts at control 0");
    __shared__ double sh[kCols][kBlock / 2];
    const int tid = threadIdx.x, seg = blockIdx.x, col0 = (int)blockIdx.y * kCols, ncol = p.T * U;
    const int k = seg * kBlock + tid;
    double a[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) a[c] = 0.0;
    if (k < p.K) {
        const double w = (double)q[k];
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int col = col0 + c;
            if (col < ncol) {
                double du;
                (void)mppi_control((uint32_t)k, (uint32_t)col, Ubar[col], p.sigma[c % U], p.umin[c % U], p.umax[c % U], p, &du);
                a[c] = w * du;
            }
        }
    }
    segment_reduce<kCols, kBlock>(a, sh, tid, seg, nseg_pow2, part + (size_t)col0 * nseg_pow2);
}

// One workgroup: the integer totals, the tree over the segment partials (tree_top; P a power of two, in place), the new Ubar
// into the other half, then thread 0 rolls it (z = 0, the rollout's own code) and writes the stats block.  OBST: the nominal
// rollout charges the moving balls' term, and the block sums the rollout kernel's counts of rollouts that hit a ball (integers).
// BODY: the nominal rollout applies the body rule (body.h) at every state.
template <int D, bool OBST, bool BODY = false>
__device__ __forceinline__ void mppi_top(const float* __restrict__ F, const DfLattice L, const float* __restrict__ cost,
                                         const double* __restrict__ Uold, double* Unew, const MppiParams p, int nb, int P,
                                         const u64* __restrict__ bsum, double* __restrict__ part, double* __restrict__ nom,
                                         MppiStats* __restrict__ st, const ObstArgs* ob, int nbr, const int* __restrict__ bdyn,
                                         ObstStats* __restrict__ ost, const BodyArgs* bd = nullptr) {
    constexpr int U = D == 3 ? 4 : 2;
    __shared__ u64 sh[kBlock / kWave];
    __shared__ u64 tot_s;
    u64 t = 0, th = 0, s2 = 0, nh = 0, key = ~0ull;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        t += bsum[b]; th += bsum[(size_t)nb + b]; s2 += bsum[2 * (size_t)nb + b]; nh += bsum[3 * (size_t)nb + b];
        key = OpMin()(key, bsum[4 * (size_t)nb + b]);
    }
    t = block_reduce(t, OpAdd(), sh, kBlock, 0ull);
    th = block_reduce(th, OpAdd(), sh, kBlock, 0ull);
    s2 = block_reduce(s2, OpAdd(), sh, kBlock, 0ull);
    nh = block_reduce(nh, OpAdd(), sh, kBlock, 0ull);
    key = block_reduce(key, OpMin(), sh, kBlock, ~0ull);
    if (threadIdx.x == 0) {
        st->T = t; st->Th = th; st->S2 = s2; st->nhit = (int)nh; st->best = (int)key; st->pad = 0;
        tot_s = t;
    }
    const int ncol = p.T * U;
    tree_top(ncol, P, part);
    __syncthreads();                                     // (P = 1: the tree has no level and no barrier)
    const double Tq = (double)tot_s;
    for (int e = threadIdx.x; e < ncol; e += kBlock) {
        const int u = e % U;
        const double lo = u == 0 ? p.umin[0] : u == 1 ? p.umin[1] : u == 2 ? p.umin[2] : p.umin[3];
        const double hi = u == 0 ? p.umax[0] : u == 1 ? p.umax[1] : u == 2 ? p.umax[2] : p.umax[3];
        double v = Uold[e] + part[(size_t)e * P] / Tq;
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
        Unew[e] = v;
    }
    __threadfence();
    __syncthreads();
    if constexpr (OBST) {
        u64 nd = 0;
        for (int b = threadIdx.x; b < nbr; b += kBlock) nd += (u64)bdyn[b];
        nd = block_reduce(nd, OpAdd(), sh, kBlock, 0ull);
        if (threadIdx.x == 0) ost->ndyn = (int)nd;
    }
    if constexpr (BODY) {
        // As below, for a body: one lane rolls the states out, a thread per step applies the body rule at that step's state (m field
        // samples, and with moving balls m walks of their table), and the lane rolls again with the steps' D (and least separations)
        // at hand.  The same expressions on the same doubles: the bits are those of the rollout kernel's loop.
        __shared__ double sd[Controller::kMaxSteps];
        __shared__ double ssep[OBST ? Controller::kMaxSteps : 1];
        constexpr int NS = D + 2;
        if (threadIdx.x == 0) {
            double J0;
            int h0;
            mppi_roll<D, true>(0u, F, L, cost, Unew, p, nom, &J0, &h0);
        }
        __threadfence();
        __syncthreads();
        DfLattice Lc = L;
        Lc.dim = D;
        for (int t = threadIdx.x; t < p.T; t += kBlock) {
            const double* S = nom + (size_t)(t + 1) * NS;
            double pos[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int a = 0; a < D; ++a) pos[a] = S[a];
            sd[t] = body_clearance_at<D>(F, Lc, bd->tab, bd->m, pos, S[D], S[D + 1]);
            if constexpr (OBST) ssep[t] = body_least_sep<D>(ob, bd, pos, S[D], S[D + 1], ob->E0 + ((double)(t + 1) * p.dt));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double Jn, sn = INFINITY;
            int hn, dn = 0;
            if constexpr (OBST) {
                mppi_roll<D, true, 2, 2>(0u, F, L, cost, Unew, p, nom, &Jn, &hn, ob, &dn, &sn, ssep, bd, sd);
                ost->nominal_dyn_hits = dn; ost->nominal_min_sep = sn;
            } else {
                mppi_roll<D, true, 0, 2>(0u, F, L, cost, Unew, p, nom, &Jn, &hn, nullptr, nullptr, nullptr, nullptr, bd, sd);
            }
            st->nominal_cost = Jn; st->nominal_hits = hn;
#pragma unroll
            for (int u = 0; u < 4; ++u) st->u0[u] = u < U ? Unew[u] : 0.0;
        }
    } else if constexpr (OBST) {
        // The nominal rollout's states do not depend on its costs: one lane rolls them out (the plain rollout, its cost dropped),
        // a thread per step then walks the table at that step's position -- T chains of n separations side by side instead of
        // one of T n -- and the lane rolls again with the steps' least separations at hand.  The same expressions on the same
        // doubles: the bits are those of the rollout kernel's loop.
        __shared__ double ssep[Controller::kMaxSteps];
        constexpr int NS = D + 2;
        if (threadIdx.x == 0) {
            double J0;
            int h0;
            mppi_roll<D, true>(0u, F, L, cost, Unew, p, nom, &J0, &h0);
        }
        __threadfence();
        __syncthreads();
        for (int t = threadIdx.x; t < p.T; t += kBlock) {
            double pos[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int a = 0; a < D; ++a) pos[a] = nom[(size_t)(t + 1) * NS + a];
            ssep[t] = obst_least_sep<D>(ob, pos, ob->E0 + ((double)(t + 1) * p.dt));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double Jn, sn;
            int hn, dn;
            mppi_roll<D, true, 2>(0u, F, L, cost, Unew, p, nom, &Jn, &hn, ob, &dn, &sn, ssep);
            ost->nominal_dyn_hits = dn; ost->nominal_min_sep = sn;
            st->nominal_cost = Jn; st->nominal_hits = hn;
#pragma unroll
            for (int u = 0; u < 4; ++u) st->u0[u] = u < U ? Unew[u] : 0.0;
        }
    } else {
        if (threadIdx.x == 0) {
            double Jn;
            int hn;
            mppi_roll<D, true>(0u, F, L, cost, Unew, p, nom, &Jn, &hn);
            st->nominal_cost = Jn; st->nominal_hits = hn;
#pragma unroll
            for (int u = 0; u < 4; ++u) st->u0[u] = u < U ? Unew[u] : 0.0;
        }
    }
}

template <int D>
__global__ void __launch_bounds__(kBlock) mppi_top_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                          const double* __restrict__ Uold, double* Unew, MppiParams p, int nb, int P,
                                                          const u64* __restrict__ bsum, double* __restrict__ part,
                                                          double* __restrict__ nom, MppiStats* __restrict__ st) {
    mppi_top<D, false>(F, L, cost, Uold, Unew, p, nb, P, bsum, part, nom, st, nullptr, 0, nullptr, nullptr);
}

template <int D>
__global__ void __launch_bounds__(kBlock) mppi_obst_top_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                               const double* __restrict__ Uold, double* Unew, MppiParams p, int nb,
                                                               int P, const u64* __restrict__ bsum, double* __restrict__ part,
                                                               double* __restrict__ nom, MppiStats* __restrict__ st, ObstArgs ob,
                                                               int nbr, const int* __restrict__ bdyn, ObstStats* __restrict__ ost) {
    mppi_top<D, true>(F, L, cost, Uold, Unew, p, nb, P, bsum, part, nom, st, &ob, nbr, bdyn, ost);
}

template <int D, bool OBST>
__global__ void __launch_bounds__(kBlock) mppi_body_top_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ cost,
                                                               const double* __restrict__ Uold, double* Unew, MppiParams p, int nb,
                                                               int P, const u64* __restrict__ bsum, double* __restrict__ part,
                                                               double* __restrict__ nom, MppiStats* __restrict__ st, BodyArgs bd,
                                                               ObstArgs ob, int nbr, const int* __restrict__ bdyn,
                                                               ObstStats* __restrict__ ost) {
    mppi_top<D, OBST, true>(F, L, cost, Uold, Unew, p, nb, P, bsum, part, nom, st, &ob, nbr, bdyn, ost, &bd);
}

// the four launches of a step with a footprint (OB: and with moving balls), from the controller's current half into the other
template <int D, bool OB>
void body_launches(Controller& c, hipStream_t s, const float* F, const DfLattice& L, const float* cost, const MppiParams& p,
                   const BodyArgs& bd, const ObstArgs& oa, double lambda) {
    const int K = c.K, nbr = (K + kRollBlock - 1) / kRollBlock, nb = (K + kBlock - 1) / kBlock, P = (int)pow2_at_least(nb);
    const int nchunk = (c.T * c.nu() + kCols - 1) / kCols;
    const double* Uc = c.d_U[c.cur];
    hipLaunchKernelGGL((mppi_body_rollout_kernel<D, OB>), dim3(nbr), dim3(kRollBlock), 0, s, F, L, cost, Uc, p, bd, oa, c.d_J, c.d_hits,
                       c.d_bmin, c.d_dyn, c.d_msep, c.d_bdyn);
    hipLaunchKernelGGL(mppi_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)c.d_J, (const int*)c.d_hits, K, nbr, nb,
                       (const double*)c.d_bmin, lambda, c.d_q, c.d_bsum, c.d_stats);
    hipLaunchKernelGGL(mppi_update_kernel<D>, dim3(P, nchunk), dim3(kBlock), 0, s, Uc, (const u64*)c.d_q, p, P, c.d_part);
    hipLaunchKernelGGL((mppi_body_top_kernel<D, OB>), dim3(1), dim3(kBlock), 0, s, F, L, cost, Uc, c.d_U[c.cur ^ 1], p, nb, P,
                       (const u64*)c.d_bsum, c.d_part, c.d_nom, c.d_stats, bd, oa, nbr, (const int*)c.d_bdyn, c.d_ostats);
}

}  // namespace

// ---- host -------------------------------------------------------------------------------------------------------------------
void mppi_default_opts(int dim, float step, MppiOpts* o) {
    const double st = (double)step;
    o->dt = 0.1; o->lambda = 1.0; o->gamma = 0.1;
    o->clearance = st; o->margin = 2.0 * st;
    o->w_obs = 1.0; o->w_col = 100.0; o->w_off = 100.0; o->w_goal = 1.0;
    for (int u = 0; u < 4; ++u) { o->sigma[u] = 0.0; o->umin[u] = 0.0; o->umax[u] = 0.0; }
    if (dim == 3) {
        for (int u = 0; u < 4; ++u) { o->sigma[u] = 0.25; o->umin[u] = -1.0; o->umax[u] = 1.0; }
        o->sigma[3] = 0.5;
    } else {
        o->sigma[0] = 0.25; o->sigma[1] = 0.5;
        o->umin[0] = 0.0; o->umax[0] = 1.0; o->umin[1] = -1.0; o->umax[1] = 1.0;
    }
}

int mppi_check_opts(const MppiOpts& o) {
    const double* all = &o.dt;
    for (size_t i = 0; i < sizeof(MppiOpts) / sizeof(double); ++i) if (!std::isfinite(all[i])) return GPIS_ERR_ARG;
    if (o.dt <= 0.0 || o.lambda <= 0.0 || o.margin < 0.0 || o.w_obs < 0.0 || o.w_col < 0.0 || o.w_off < 0.0 || o.w_goal < 0.0)
        return GPIS_ERR_ARG;
    for (int u = 0; u < 4; ++u) if (o.sigma[u] < 0.0 || o.umin[u] > o.umax[u]) return GPIS_ERR_ARG;
    return GPIS_OK;
}

Controller::Controller() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Controller::~Controller() { (void)bind(-1); }

int Controller::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_U[0], (void*)d_U[1], (void*)d_J, (void*)d_q, (void*)d_hits, (void*)d_bmin, (void*)d_bsum, (void*)d_part,
                        (void*)d_nom, (void*)d_stats, (void*)d_dyn, (void*)d_msep, (void*)d_bdyn, (void*)d_ostats})
            (void)hipFree(p);
        if (h_stats) (void)hipHostFree(h_stats);
        if (h_ostats) (void)hipHostFree(h_ostats);
        if (own) (void)hipStreamDestroy(own);
    }
    d_U[0] = d_U[1] = nullptr; d_J = nullptr; d_q = nullptr; d_hits = nullptr; d_bmin = nullptr; d_bsum = nullptr; d_part = nullptr;
    d_nom = nullptr; d_stats = nullptr; h_stats = nullptr; own = nullptr;
    d_dyn = nullptr; d_msep = nullptr; d_bdyn = nullptr; d_ostats = nullptr; h_ostats = nullptr; cap_dyn = 0; obst_n = 0;
    cap_u = cap_k = cap_part = cap_nom = 0;
    inited = have_step = false; dim = K = T = 0;
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int Controller::ensure(int dm, int k, int t) {
    if (!d_stats) GPIS_HIP(hipMalloc((void**)&d_stats, sizeof(MppiStats)));
    if (!h_stats) GPIS_HIP(hipHostMalloc((void**)&h_stats, sizeof(MppiStats)));
    const size_t nu_ = dm == 3 ? 4 : 2, ncol = (size_t)t * nu_, colp = (ncol + kCols - 1) / kCols * kCols;
    const size_t nseg = ((size_t)k + kBlock - 1) / kBlock, P = (size_t)pow2_at_least((long long)nseg);
    if (ncol > cap_u) {
        for (int h = 0; h < 2; ++h) { (void)hipFree(d_U[h]); d_U[h] = nullptr; }
        cap_u = 0;
        for (int h = 0; h < 2; ++h) GPIS_HIP(hipMalloc((void**)&d_U[h], sizeof(double) * ncol));     // (halves apart: no shared line)
        cap_u = ncol;
    }
    if ((size_t)k > cap_k) {
        for (void* p : {(void*)d_J, (void*)d_q, (void*)d_hits, (void*)d_bmin, (void*)d_bsum}) (void)hipFree(p);
        d_J = nullptr; d_q = nullptr; d_hits = nullptr; d_bmin = nullptr; d_bsum = nullptr; cap_k = 0;
        GPIS_HIP(hipMalloc((void**)&d_J, sizeof(double) * k));
        GPIS_HIP(hipMalloc((void**)&d_q, sizeof(u64) * k));
        GPIS_HIP(hipMalloc((void**)&d_hits, sizeof(int) * k));
        GPIS_HIP(hipMalloc((void**)&d_bmin, sizeof(double) * (((size_t)k + kRollBlock - 1) / kRollBlock)));
        GPIS_HIP(hipMalloc((void**)&d_bsum, sizeof(u64) * kSums * nseg));
        cap_k = (size_t)k;
    }
    if (colp * P > cap_part) {
        (void)hipFree(d_part); d_part = nullptr; cap_part = 0;
        GPIS_HIP(hipMalloc((void**)&d_part, sizeof(double) * colp * P));
        cap_part = colp * P;
    }
    const size_t nn = (size_t)(t + 1) * (size_t)(dm + 2);
    if (nn > cap_nom) {
        (void)hipFree(d_nom); d_nom = nullptr; cap_nom = 0;
        GPIS_HIP(hipMalloc((void**)&d_nom, sizeof(double) * nn));
        cap_nom = nn;
    }
    return GPIS_OK;
}

int Controller::init(int dm, int k, int t, uint64_t sd) {
    int dev = -1;
    GPIS_HIP(hipGetDevice(&dev));
    if (int rc = bind(dev)) return rc;
    if (!own) return GPIS_ERR_HIP;
    inited = have_step = false;
    if (int rc = ensure(dm, k, t)) return rc;
    const size_t ncol = (size_t)t * (dm == 3 ? 4 : 2);
    GPIS_HIP(hipMemsetAsync(d_U[0], 0, sizeof(double) * ncol, own));
    GPIS_HIP(hipMemsetAsync(d_U[1], 0, sizeof(double) * ncol, own));
    GPIS_HIP(hipMemsetAsync(d_J, 0, sizeof(double) * k, own));
    GPIS_HIP(hipMemsetAsync(d_q, 0, sizeof(u64) * k, own));
    GPIS_HIP(hipMemsetAsync(d_hits, 0, sizeof(int) * k, own));
    GPIS_HIP(hipMemsetAsync(d_nom, 0, sizeof(double) * (size_t)(t + 1) * (size_t)(dm + 2), own));
    GPIS_HIP(hipStreamSynchronize(own));
    dim = dm; K = k; T = t; cur = 0; tick = 0; seed = sd; steps = 0; neff = 0.0; ms = 0.0;
    stats = MppiStats{};
    obst_n = 0; ostats = ObstStats{};
    inited = true;
    return GPIS_OK;
}

int Controller::set_nominal(const double* U) {
    GPIS_HIP(hipMemcpyAsync(d_U[cur], U, sizeof(double) * (size_t)T * nu(), hipMemcpyHostToDevice, own));
    GPIS_HIP(hipStreamSynchronize(own));
    return GPIS_OK;
}

int Controller::shift() {
    // rows 1 .. T - 1 into rows 0 .. T - 2 of the other half, the last row twice
    const size_t row = sizeof(double) * (size_t)nu();
    const int to = cur ^ 1;
    if (T > 1) GPIS_HIP(hipMemcpyAsync(d_U[to], d_U[cur] + nu(), row * (size_t)(T - 1), hipMemcpyDeviceToDevice, own));
    GPIS_HIP(hipMemcpyAsync(d_U[to] + (size_t)(T - 1) * nu(), d_U[cur] + (size_t)(T - 1) * nu(), row, hipMemcpyDeviceToDevice, own));
    GPIS_HIP(hipStreamSynchronize(own));
    cur = to;
    return GPIS_OK;
}

int Controller::step(const DistanceField& df, const Planner* pl, const double* start, const double* goal, const MppiOpts& o,
                     hipStream_t s, const ObstArgs* ob, const BodyArgs* bd) {
    const auto t0 = std::chrono::steady_clock::now();
    if (ob) {
        if (!d_ostats) GPIS_HIP(hipMalloc((void**)&d_ostats, sizeof(ObstStats)));
        if (!h_ostats) GPIS_HIP(hipHostMalloc((void**)&h_ostats, sizeof(ObstStats)));
        if ((size_t)K > cap_dyn) {
            for (void* q : {(void*)d_dyn, (void*)d_msep, (void*)d_bdyn}) (void)hipFree(q);
            d_dyn = nullptr; d_msep = nullptr; d_bdyn = nullptr; cap_dyn = 0;
            GPIS_HIP(hipMalloc((void**)&d_dyn, sizeof(int) * (size_t)K));
            GPIS_HIP(hipMalloc((void**)&d_msep, sizeof(double) * (size_t)K));
            GPIS_HIP(hipMalloc((void**)&d_bdyn, sizeof(int) * (((size_t)K + kRollBlock - 1) / kRollBlock)));
            cap_dyn = (size_t)K;
        }
    }
    MppiParams p{};
    p.dt = o.dt; p.half_dt = 0.5 * o.dt; p.gamma = o.gamma; p.lambda = o.lambda;
    for (int u = 0; u < 4; ++u) { p.sigma[u] = o.sigma[u]; p.umin[u] = o.umin[u]; p.umax[u] = o.umax[u]; }
    p.clearance = o.clearance; p.band = o.clearance + o.margin; p.margin = o.margin;
    p.w_obs = o.w_obs; p.w_col = o.w_col; p.w_off = o.w_off; p.w_goal = o.w_goal;
    for (int a = 0; a < dim + 2; ++a) p.start[a] = start[a];
    if (goal) for (int a = 0; a < dim; ++a) p.goal[a] = goal[a];
    p.K = K; p.T = T; p.use_plan = pl ? 1 : 0;
    p.tick = tick + 1; p.k0 = (uint32_t)(seed & 0xffffffffull); p.k1 = (uint32_t)(seed >> 32);
    const DfLattice L = df.lattice();
    const float* cost = pl ? pl->d_cost : nullptr;
    const int nbr = (K + kRollBlock - 1) / kRollBlock, nb = (K + kBlock - 1) / kBlock, P = (int)pow2_at_least(nb);
    const int ncol = T * nu(), nchunk = (ncol + kCols - 1) / kCols, to = cur ^ 1;
    const double* Uc = d_U[cur];
    if (bd) {
        const float* F = (const float*)df.d_dist;
        const ObstArgs oa = ob ? *ob : ObstArgs{};
        if (dim == 3) {
            if (ob) body_launches<3, true>(*this, s, F, L, cost, p, *bd, oa, o.lambda);
            else body_launches<3, false>(*this, s, F, L, cost, p, *bd, oa, o.lambda);
        } else {
            if (ob) body_launches<2, true>(*this, s, F, L, cost, p, *bd, oa, o.lambda);
            else body_launches<2, false>(*this, s, F, L, cost, p, *bd, oa, o.lambda);
        }
        if (ob) {
            GPIS_HIP(hipGetLastError());
            GPIS_HIP(hipMemcpyAsync(h_ostats, d_ostats, sizeof(ObstStats), hipMemcpyDeviceToHost, s));
        }
    } else if (ob) {
        const float* F = (const float*)df.d_dist;
        if (dim == 3) {
            hipLaunchKernelGGL(mppi_obst_rollout_kernel<3>, dim3(nbr), dim3(kRollBlock), 0, s, F, L, cost, Uc, p, *ob, d_J, d_hits, d_bmin,
                               d_dyn, d_msep, d_bdyn);
            hipLaunchKernelGGL(mppi_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)d_J, (const int*)d_hits, K, nbr, nb,
                               (const double*)d_bmin, o.lambda, d_q, d_bsum, d_stats);
            hipLaunchKernelGGL(mppi_update_kernel<3>, dim3(P, nchunk), dim3(kBlock), 0, s, Uc, (const u64*)d_q, p, P, d_part);
            hipLaunchKernelGGL(mppi_obst_top_kernel<3>, dim3(1), dim3(kBlock), 0, s, F, L, cost, Uc, d_U[to], p, nb, P, (const u64*)d_bsum,
                               d_part, d_nom, d_stats, *ob, nbr, (const int*)d_bdyn, d_ostats);
        } else {
            hipLaunchKernelGGL(mppi_obst_rollout_kernel<2>, dim3(nbr), dim3(kRollBlock), 0, s, F, L, cost, Uc, p, *ob, d_J, d_hits, d_bmin,
                               d_dyn, d_msep, d_bdyn);
            hipLaunchKernelGGL(mppi_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)d_J, (const int*)d_hits, K, nbr, nb,
                               (const double*)d_bmin, o.lambda, d_q, d_bsum, d_stats);
            hipLaunchKernelGGL(mppi_update_kernel<2>, dim3(P, nchunk), dim3(kBlock), 0, s, Uc, (const u64*)d_q, p, P, d_part);
            hipLaunchKernelGGL(mppi_obst_top_kernel<2>, dim3(1), dim3(kBlock), 0, s, F, L, cost, Uc, d_U[to], p, nb, P, (const u64*)d_bsum,
                               d_part, d_nom, d_stats, *ob, nbr, (const int*)d_bdyn, d_ostats);
        }
        GPIS_HIP(hipGetLastError());
        GPIS_HIP(hipMemcpyAsync(h_ostats, d_ostats, sizeof(ObstStats), hipMemcpyDeviceToHost, s));
    } else if (dim == 3) {
        hipLaunchKernelGGL(mppi_rollout_kernel<3>, dim3(nbr), dim3(kRollBlock), 0, s, (const float*)df.d_dist, L, cost, Uc, p, d_J, d_hits, d_bmin);
        hipLaunchKernelGGL(mppi_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)d_J, (const int*)d_hits, K, nbr, nb,
                           (const double*)d_bmin, o.lambda, d_q, d_bsum, d_stats);
        hipLaunchKernelGGL(mppi_update_kernel<3>, dim3(P, nchunk), dim3(kBlock), 0, s, Uc, (const u64*)d_q, p, P, d_part);
        hipLaunchKernelGGL(mppi_top_kernel<3>, dim3(1), dim3(kBlock), 0, s, (const float*)df.d_dist, L, cost, Uc, d_U[to], p, nb, P,
                           (const u64*)d_bsum, d_part, d_nom, d_stats);
    } else {
        hipLaunchKernelGGL(mppi_rollout_kernel<2>, dim3(nbr), dim3(kRollBlock), 0, s, (const float*)df.d_dist, L, cost, Uc, p, d_J, d_hits, d_bmin);
        hipLaunchKernelGGL(mppi_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)d_J, (const int*)d_hits, K, nbr, nb,
                           (const double*)d_bmin, o.lambda, d_q, d_bsum, d_stats);
        hipLaunchKernelGGL(mppi_update_kernel<2>, dim3(P, nchunk), dim3(kBlock), 0, s, Uc, (const u64*)d_q, p, P, d_part);
        hipLaunchKernelGGL(mppi_top_kernel<2>, dim3(1), dim3(kBlock), 0, s, (const float*)df.d_dist, L, cost, Uc, d_U[to], p, nb, P,
                           (const u64*)d_bsum, d_part, d_nom, d_stats);
    }
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof(MppiStats), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    stats = *h_stats;
    obst_n = ob ? ob->n : 0;
    if (ob) ostats = *h_ostats;
    neff = (double)stats.Th * (double)stats.Th / (double)stats.S2;
    tick += 1; cur = to; steps += 1; have_step = true;
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GPIS_OK;
}

}  // namespace gpis
