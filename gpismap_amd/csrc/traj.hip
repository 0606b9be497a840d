// Trajectory smoothing through a distance field (traj.h).
//
// Waypoint i of trajectory t: x[(t N + i) dim + a].  x_0 and x_{N-1} never move; n = N - 2 interior points.  One workgroup of
// 64 ceil(N / 64) threads owns a trajectory, lane i its waypoint i (in the evaluation also the segment i -> i + 1).  x and the
// gradient g live in LDS; an iteration is: sample the field at the own waypoint (4 / 8 corners through L2), g to LDS, the own row
// of inverse(tridiag(-1, 2, -1)) times g accumulated in registers over ascending j with g_j a broadcast LDS read, the largest
// step by a wavefront reduction (a max is exact in any order), the trust region, the update.  Sums of the evaluation use one
// fixed tree over 256 slots.  No floating-point atomics; -ffp-contract=off keeps every product and sum apart.
//
// Time parametrisation of the last result and the control sequences it gives follow below: the same layout (a
// workgroup per trajectory, a lane per waypoint or per step), prefixes summed ascending by each lane, the speed profile as a
// minimum over cones.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>
#include "traj.h"
#include "block_ops.h"
#include "mppi.h"
#include "obst.h"
#include "body.h"
#include "dfield.h"
#include "plan.h"
#include "pplan.h"

namespace gpis {

namespace {

constexpr int kBlock = 256;
constexpr int kTree = Trajectories::kMaxN;

constexpr long long kGridCapTraj = 65535ll * 16;

// s[off[p] + k] = length of path p up to its point k: a serial ascending sum of sqrtf(squares summed left to right)
__global__ void __launch_bounds__(kBlock) traj_arc_kernel(const long long* __restrict__ off, const float* __restrict__ pts,
                                                          const unsigned char* __restrict__ pstat, int m, int dim,
                                                          float* __restrict__ arc) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        if (pstat[p] != 0) continue;
        const long long b = off[p], len = off[p + 1] - b;
        float s = 0.f;
        for (long long k = 0; k < len; ++k) {
            if (k > 0) {
                const float* q = pts + (size_t)(b + k) * dim;
                float sq = 0.f;
                for (int a = 0; a < dim; ++a) {
                    const float d = q[a] - q[a - dim];
                    sq = a ? sq + d * d : d * d;
                }
                s = s + sqrtf(sq);
            }
            arc[b + k] = s;
        }
    }
}

// one thread per waypoint: t_i = (float)i * (s_{L-1} / (float)(N - 1)), the last segment k <= L - 2 with s_k <= t_i by bisection,
// x_i = Q_k + w (Q_{k+1} - Q_k); the two ends are copies.  A path of another status than 0: NaN and input status 2.
// ZERO_W (pose paths, DESIGN.md §7t: a turn in place repeats a point): w = 0 on a segment of no length.
template <bool ZERO_W>
__global__ void __launch_bounds__(kBlock) traj_resample_kernel(const long long* __restrict__ off, const float* __restrict__ pts,
                                                               const unsigned char* __restrict__ pstat,
                                                               const float* __restrict__ arc, int m, int N, int dim,
                                                               float* __restrict__ x, unsigned char* __restrict__ instat) {
    const long long total = (long long)m * N;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(id / N), i = (int)(id % N);
        float* out = x + (size_t)id * dim;
        const long long b = off[p], len = off[p + 1] - b;
        const bool ok = pstat[p] == 0 && len >= 1;
        if (i == 0) instat[p] = ok ? 0 : 2;
        if (!ok) {
            for (int a = 0; a < dim; ++a) out[a] = __int_as_float(0x7fc00000);
            continue;
        }
        const float* q = pts + (size_t)b * dim;
        if (len == 1 || i == 0 || i == N - 1) {
            const float* s = i == N - 1 ? q + (size_t)(len - 1) * dim : q;
            for (int a = 0; a < dim; ++a) out[a] = s[a];
            continue;
        }
        const float* s = arc + b;
        const float t = (float)i * (s[len - 1] / (float)(N - 1));
        long long lo = 0, hi = len - 2;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if (s[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const float w = ZERO_W && s[lo + 1] == s[lo] ? 0.f : (t - s[lo]) / (s[lo + 1] - s[lo]);
        const float* q0 = q + (size_t)lo * dim;
        for (int a = 0; a < dim; ++a) out[a] = q0[a] + w * (q0[dim + a] - q0[a]);
    }
}

// max that keeps a NaN, as numpy's does: a step that overflowed must not pass for a small one
__device__ __forceinline__ float traj_max(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : fmaxf(a, b); }

struct TrajSample {
    float d, g[3];
    bool fin;            // d and every gradient component finite
};

template <int DIM>
__device__ __forceinline__ TrajSample traj_sample(const float* __restrict__ F, const DfLattice& L, const float* x) {
    float o[4];
    DfLattice K = L;
    K.dim = DIM;                                         // (a constant dim keeps o in registers)
    df_sample_at(F, K, x[0], x[1], DIM == 3 ? x[2] : 0.f, o);
    TrajSample s;
    s.d = o[0];
    s.fin = isfinite(o[0]);
#pragma unroll
    for (int a = 0; a < DIM; ++a) { s.g[a] = o[1 + a]; s.fin = s.fin && isfinite(o[1 + a]); }
    return s;
}

// The heading a waypoint takes from the horizontal chords of its trajectory (the chord rule of DESIGN.md §7r, the one statement
// of it): waypoint k's first two components are x0[k st], x1[k st].  The first chord k >= min(i, N - 2) with a horizontal length
// > 0, else the last one before, else (1, 0); double from the float32 waypoints.  own: the chord min(i, N - 2) itself has a
// length (then nn is that length).
struct TrajChord {
    double c, s, nn;
    bool own;
};

__device__ __forceinline__ TrajChord traj_chord_heading(const float* x0, const float* x1, int st, int i, int N) {
    const int k0 = min(i, N - 2);
    TrajChord h{1.0, 0.0, 1.0, false};
    bool found = false;
    for (int pass = 0; pass < 2 && !found; ++pass) {
        // pass 0: k = k0 .. N - 2 ascending; pass 1: k = k0 - 1 .. 0 descending
        for (int k = pass == 0 ? k0 : k0 - 1; pass == 0 ? k <= N - 2 : k >= 0; k += pass == 0 ? 1 : -1) {
            const double e0 = (double)x0[(k + 1) * st] - (double)x0[k * st], e1 = (double)x1[(k + 1) * st] - (double)x1[k * st];
            const double n2 = e0 * e0 + e1 * e1;
            if (n2 > 0.0) {
                const double nn = sqrt(n2);
                h.c = e0 / nn; h.s = e1 / nn; h.nn = nn;
                h.own = k == k0;
                found = true;
                break;
            }
        }
    }
    return h;
}

// One workgroup per trajectory, blockDim.x = 64 ceil(N / 64).  fres[t] = length, smoothness, obstacle cost, min_dist;
// ires[t] = status, iterations, non-finite samples, collides.
// BODY (the contract: tests/traj_body_ref.py): the obstacle term acts at the balls of the footprint bd.  Every lane
// of a waypoint (the ends too) takes its chord's heading from x in LDS, walks the table by a pointer whose index is the same in
// every lane, and sums the force and the torque over ascending j; the torque over the chord's length along the chord's normal
// is t_i, kept in LDS, and an interior lane gathers T_{i-1} - T_i after one barrier.  The evaluation walks the table once more:
// the obstacle cost at the balls and the body rule of every waypoint, reduced as traj_body_check_kernel does.
// bres_d[t] = D_min; bres_i[t][3] = waypoint, ball, collides.  Without BODY the last four arguments are not read.
template <int DIM, bool BODY>
__global__ void __launch_bounds__(kBlock) traj_opt_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ xin,
                                                          const unsigned char* __restrict__ instat, int N, TrajOpts o,
                                                          float* __restrict__ xout, float* __restrict__ fres,
                                                          int* __restrict__ ires, BodyArgs bd, float w_turn,
                                                          double* __restrict__ bres_d, int* __restrict__ bres_i) {
    __shared__ float sx[DIM][kTree];
    __shared__ float sg[DIM][kTree];
    __shared__ float ssum[3][kTree];
    __shared__ float smin[kTree];
    __shared__ int scnt[kTree];
    __shared__ float swave[kBlock / 64];
    __shared__ float sT[2][kTree];                       // (BODY only, as the two below)
    __shared__ double shd[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, t = threadIdx.x, n = N - 2, nthr = blockDim.x;
    const size_t base = (size_t)tr * N * DIM;
    const float nan = __int_as_float(0x7fc00000);

    if (instat[tr] != 0) {                               // no input: the waypoints pass through untouched
        if (t < N) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) xout[base + (size_t)t * DIM + a] = xin[base + (size_t)t * DIM + a];
        }
        if (t == 0) {
            for (int k = 0; k < 4; ++k) fres[(size_t)tr * 4 + k] = nan;
            ires[(size_t)tr * 4 + 0] = 2; ires[(size_t)tr * 4 + 1] = 0; ires[(size_t)tr * 4 + 2] = 0; ires[(size_t)tr * 4 + 3] = 0;
            if constexpr (BODY) {
                bres_d[tr] = (double)NAN;
                bres_i[(size_t)tr * 3] = -1; bres_i[(size_t)tr * 3 + 1] = -1; bres_i[(size_t)tr * 3 + 2] = 0;
            }
        }
        return;
    }

    if (t < N) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) sx[a][t] = xin[base + (size_t)t * DIM + a];
    }
    __syncthreads();

    const bool interior = t >= 1 && t <= n;
    const float fn1 = (float)(n + 1);
    int status = 1, used = 0;
    for (int it = 0; it < o.iters; ++it) {
        float xi[DIM], g[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) { xi[a] = 0.f; g[a] = 0.f; }
        if constexpr (BODY) {
            float f[DIM], t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int a = 0; a < DIM; ++a) f[a] = 0.f;
            if (t < N) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) xi[a] = sx[a][t];
                const TrajChord h = traj_chord_heading(sx[0], sx[1], 1, t, N);
                const double p[3] = {(double)xi[0], (double)xi[1], DIM == 3 ? (double)xi[DIM - 1] : 0.0};
                const double* __restrict__ row = bd.tab;
                float tau = 0.f;
                for (int j = 0; j < bd.m; ++j, row += 4) {
                    double w[3] = {0.0, 0.0, 0.0};
                    body_ball_at<DIM>(row, p, h.c, h.s, w);
                    const float pw[3] = {(float)w[0], (float)w[1], (float)w[2]};
                    const TrajSample s = traj_sample<DIM>(F, L, pw);
                    const float d = (float)((double)s.d - row[3]);
                    float q = 0.f;
                    if (s.fin) {
                        const float e = d - o.clearance;
                        if (e >= o.margin) q = 0.f;
                        else if (e >= 0.f) q = (e - o.margin) / o.margin;
                        else q = -1.f;
                    }
                    const float r0 = (float)((-h.s) * row[0] - h.c * row[1]), r1 = (float)(h.c * row[0] - h.s * row[1]);
                    float gr[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        gr[a] = s.fin ? s.g[a] : 0.f;
                        const float fj = q * gr[a];
                        f[a] = j ? f[a] + fj : fj;
                    }
                    const float tj = q * (gr[0] * r0 + gr[1] * r1);
                    tau = j ? tau + tj : tj;
                }
                if (h.own) {
                    const float u = tau / (float)h.nn;
                    t0 = u * (-(float)h.s);
                    t1 = u * (float)h.c;
                }
            }
            sT[0][t] = t0; sT[1][t] = t1;
            __syncthreads();
            if (interior) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const float aa = (xi[a] - sx[a][t - 1]) + (xi[a] - sx[a][t + 1]);
                    if (a < 2) {
                        const float Ti = t == N - 2 ? sT[a][t] + sT[a][t + 1] : sT[a][t];
                        g[a] = o.w_smooth * aa + o.w_obs * (f[a] + w_turn * (sT[a][t - 1] - Ti));
                    } else {
                        g[a] = o.w_smooth * aa + o.w_obs * f[a];
                    }
                }
            }
        } else if (interior) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) xi[a] = sx[a][t];
            const TrajSample s = traj_sample<DIM>(F, L, xi);
            float q = 0.f;
            if (s.fin) {
                const float e = s.d - o.clearance;
                if (e >= o.margin) q = 0.f;
                else if (e >= 0.f) q = (e - o.margin) / o.margin;
                else q = -1.f;
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const float gr = s.fin ? s.g[a] : 0.f;
                const float aa = (xi[a] - sx[a][t - 1]) + (xi[a] - sx[a][t + 1]);
                g[a] = o.w_smooth * aa + o.w_obs * (q * gr);
            }
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) sg[a][t] = g[a];
        __syncthreads();

        // the own row of inverse(tridiag(-1, 2, -1)): (min(i, j) (n + 1 - max(i, j))) / (n + 1), ascending j from 0.f
        float acc[DIM], del[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) acc[a] = 0.f;
        if (interior) {
            for (int j = 1; j <= n; ++j) {
                const float cf = (float)(min(t, j) * (n + 1 - max(t, j)));
#pragma unroll
                for (int a = 0; a < DIM; ++a) acc[a] = acc[a] + cf * sg[a][j];
            }
        }
        float sq = 0.f;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            del[a] = acc[a] / fn1;
            sq = a ? sq + del[a] * del[a] : del[a] * del[a];
        }
        float R = interior ? sqrtf(sq) : 0.f;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) R = traj_max(R, __shfl_xor(R, sh));
        if (nthr > 64) {
            if ((t & 63) == 0) swave[t >> 6] = R;
            __syncthreads();
            R = swave[0];
            for (int w = 1; w < (nthr >> 6); ++w) R = traj_max(R, swave[w]);
        }
        const float kappa = o.rate * R <= o.max_move ? o.rate : o.max_move / R;
        if (interior) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) sx[a][t] = xi[a] - kappa * del[a];
        }
        used = it + 1;
        if (kappa * R < o.tol) { status = 0; break; }    // (uniform: every lane holds the same kappa and R)
        __syncthreads();
    }
    __syncthreads();

    // evaluation: lane i samples waypoint i and the `sub` points inside segment i -> i + 1
    for (int k = t; k < kTree; k += nthr) { ssum[0][k] = 0.f; ssum[1][k] = 0.f; ssum[2][k] = 0.f; smin[k] = INFINITY; scnt[k] = 0; }
    float len = 0.f, sm = 0.f, oc = 0.f, md = INFINITY;
    int nf = 0;
    [[maybe_unused]] double bbest = INFINITY;
    [[maybe_unused]] int bwp = -1, bjm = -1, bbad = 0, boff = 0;
    if (t < N) {
        float xi[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) { xi[a] = sx[a][t]; xout[base + (size_t)t * DIM + a] = xi[a]; }
        const TrajSample s = traj_sample<DIM>(F, L, xi);
        if (isfinite(s.d)) md = s.d; else ++nf;
        if constexpr (BODY) {
            // the body at the result's heading: the obstacle cost at the balls (interior waypoints) and the body rule
            const TrajChord h = traj_chord_heading(sx[0], sx[1], 1, t, N);
            const double p[3] = {(double)xi[0], (double)xi[1], DIM == 3 ? (double)xi[DIM - 1] : 0.0};
            const double* __restrict__ row = bd.tab;
            double D = INFINITY;
            int jm = 0;
            bool off = false;
            for (int j = 0; j < bd.m; ++j, row += 4) {
                double w[3] = {0.0, 0.0, 0.0};
                body_ball_at<DIM>(row, p, h.c, h.s, w);
                const float pw[3] = {(float)w[0], (float)w[1], (float)w[2]};
                const TrajSample u = traj_sample<DIM>(F, L, pw);
                const double d = (double)u.d - row[3];
                off = off || d != d;
                if (d < D) { D = d; jm = j; }
                float cj = 0.f;
                if (interior && u.fin) {
                    const float e = (float)d - o.clearance;
                    if (e >= o.margin) cj = 0.f;
                    else if (e >= 0.f) { const float v = e - o.margin; cj = (v * v) / (2.f * o.margin); }
                    else cj = 0.5f * o.margin - e;
                }
                oc = j ? oc + cj : cj;
            }
            if (off) { boff = 1; bbad = 1; }
            else {
                bbad = D < (double)o.clearance ? 1 : 0;
                if (D < bbest) { bbest = D; bwp = t; bjm = jm; }
            }
        } else if (interior && s.fin) {
            const float e = s.d - o.clearance;
            if (e >= o.margin) oc = 0.f;
            else if (e >= 0.f) { const float u = e - o.margin; oc = (u * u) / (2.f * o.margin); }
            else oc = 0.5f * o.margin - e;
        }
        if (t <= N - 2) {
            float v[DIM], sq = 0.f;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                v[a] = sx[a][t + 1] - xi[a];
                sq = a ? sq + v[a] * v[a] : v[a] * v[a];
            }
            sm = sq;
            len = sqrtf(sq);
            for (int k = 1; k <= o.sub; ++k) {
                const float w = (float)k / (float)(o.sub + 1);
                float p[DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) p[a] = xi[a] + w * v[a];
                const TrajSample u = traj_sample<DIM>(F, L, p);
                if (isfinite(u.d)) md = fminf(md, u.d); else ++nf;
            }
        }
    }
    ssum[0][t] = len; ssum[1][t] = sm; ssum[2][t] = oc; smin[t] = md; scnt[t] = nf;
    // the tree over 256 slots; a slot past the workgroup holds 0 (+inf) and takes part through the lanes below it
    for (int h = kTree / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (t < h) {
            ssum[0][t] = ssum[0][t] + ssum[0][t + h];
            ssum[1][t] = ssum[1][t] + ssum[1][t + h];
            ssum[2][t] = ssum[2][t] + ssum[2][t + h];
            smin[t] = fminf(smin[t], smin[t + h]);
            scnt[t] = scnt[t] + scnt[t + h];
        }
    }
    if (t == 0) {
        fres[(size_t)tr * 4 + 0] = ssum[0][0]; fres[(size_t)tr * 4 + 1] = ssum[1][0]; fres[(size_t)tr * 4 + 2] = ssum[2][0];
        fres[(size_t)tr * 4 + 3] = smin[0];
        ires[(size_t)tr * 4 + 0] = status; ires[(size_t)tr * 4 + 1] = used; ires[(size_t)tr * 4 + 2] = scnt[0];
        ires[(size_t)tr * 4 + 3] = smin[0] < o.clearance ? 1 : 0;
    }
    if constexpr (BODY) {
        // the least D (a min of doubles that are never NaN where they were taken: order-free), then the least waypoint among the
        // lanes that hold it, and that lane writes
        const double bmin = block_reduce(bbest, OpMin(), shd, nthr, (double)INFINITY);
        if (t == 0) shd[0] = bmin;
        __syncthreads();
        const double least = shd[0];
        const int key = bwp >= 0 && bbest == least ? bwp : 0x7fffffff;
        const int kmin = block_reduce(key, OpMin(), shi, nthr, 0x7fffffff);
        if (t == 0) shi[0] = kmin;
        __syncthreads();
        const int win = shi[0];
        __syncthreads();
        const int nbad = block_reduce(bbad, OpAdd(), shi, nthr, 0);
        const int noff = block_reduce(boff, OpAdd(), shi, nthr, 0);
        if (t == 0) {
            bres_i[(size_t)tr * 3 + 2] = nbad > 0 ? 1 : 0;
            if (win == 0x7fffffff) {                     // no waypoint gave a D below +inf
                bres_d[tr] = noff == N ? (double)NAN : (double)INFINITY;
                bres_i[(size_t)tr * 3] = -1; bres_i[(size_t)tr * 3 + 1] = -1;
            }
        }
        if (bwp >= 0 && bwp == win) {
            bres_d[tr] = bbest;
            bres_i[(size_t)tr * 3] = bwp; bres_i[(size_t)tr * 3 + 1] = bjm;
        }
    }
}

// ---- time parametrisation --------------------------------------------------------------------------------------
struct OpMaxNan { __device__ float operator()(float a, float b) const { return traj_max(a, b); } };

// One workgroup per trajectory, blockDim.x = 64 ceil(N / 64), lane i = waypoint i (and segment i -> i + 1).  ds, S, L, the
// speeds and dt live in LDS; a lane sums its own prefix over ascending j and takes its own row of the envelope, every operand
// a broadcast LDS read.  tsum[t] = duration, max speed, max curvature; tint[t] = status, waypoints per limiter code.
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_time_kernel(const float* __restrict__ F, DfLattice L, int use_field,
                                                           const float* __restrict__ x, const int* __restrict__ ires, int N,
                                                           TimingOpts o, float* __restrict__ vout, float* __restrict__ tout,
                                                           unsigned char* __restrict__ lim, float* __restrict__ tsum,
                                                           int* __restrict__ tint) {
    __shared__ float sx[DIM][kTree];
    __shared__ float sds[kTree], sS[kTree], sL[kTree], sv[kTree], sdt[kTree];
    __shared__ unsigned char scode[kTree];
    __shared__ float swf[kBlock / 64];
    __shared__ int swi[kBlock / 64];
    const int tr = blockIdx.x, t = threadIdx.x, nthr = blockDim.x;
    const size_t base = (size_t)tr * N;
    const float nan = __int_as_float(0x7fc00000);

    if (ires[(size_t)tr * 4] == 2) {                     // no input
        if (t < N) { vout[base + t] = nan; tout[base + t] = nan; lim[base + t] = 0; }
        if (t < 3) tsum[(size_t)tr * 3 + t] = nan;
        if (t < 9) tint[(size_t)tr * 9 + t] = t == 0 ? 2 : 0;
        return;
    }

    if (t < N) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) sx[a][t] = x[(base + t) * DIM + a];
    }
    __syncthreads();
    float ds = 0.f;
    if (t <= N - 2) {
        float sq = 0.f;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const float d = sx[a][t + 1] - sx[a][t];
            sq = a ? sq + d * d : d * d;
        }
        ds = sqrtf(sq);
    }
    sds[t] = ds;
    __syncthreads();

    const bool interior = t >= 1 && t <= N - 2;
    float S = 0.f, kappa = 0.f;
    if (t < N)
        for (int j = 0; j < t; ++j) S = S + sds[j];
    sS[t] = S;
    if (interior) {
        float a[DIM], b[DIM], sq = 0.f;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            a[k] = sx[k][t] - sx[k][t - 1];
            b[k] = sx[k][t + 1] - sx[k][t];
            const float c = sx[k][t + 1] - sx[k][t - 1];
            sq = k ? sq + c * c : c * c;
        }
        float cr;
        if (DIM == 2) cr = fabsf(a[0] * b[1] - a[1] * b[0]);
        else {
            const float cx = a[1] * b[DIM - 1] - a[DIM - 1] * b[1], cy = a[DIM - 1] * b[0] - a[0] * b[DIM - 1],
                        cz = a[0] * b[1] - a[1] * b[0];
            cr = sqrtf((cx * cx + cy * cy) + cz * cz);
        }
        const float num = 2.f * cr, den = (sds[t - 1] * ds) * sqrtf(sq);
        kappa = den == 0.f ? 0.f : num / den;
    }
    float Li = o.v_max * o.v_max;
    int code = 0;
    if (t < N) {
        if (kappa != 0.f) {
            if (o.a_lat > 0.f) { const float c = o.a_lat / kappa; if (c < Li) { Li = c; code = 1; } }
            if (o.w_max > 0.f) { const float q = o.w_max / kappa, c = q * q; if (c < Li) { Li = c; code = 2; } }
        }
        if (use_field && o.slow_dist > 0.f) {
            float xi[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) xi[a] = sx[a][t];
            const float d = traj_sample<DIM>(F, L, xi).d;
            if (isfinite(d)) {
                const float e = d - o.clearance;
                const float vs = e <= 0.f ? o.v_min : o.v_min + (o.v_max - o.v_min) * fminf(e / o.slow_dist, 1.f);
                const float c = vs * vs;
                if (c < Li) { Li = c; code = 3; }
            }
        }
        if (interior && Li < o.v_min * o.v_min) { Li = o.v_min * o.v_min; code = 4; }
        if (t == 0) { const float c = o.v_start * o.v_start; if (c < Li) { Li = c; code = 5; } }
        if (t == N - 1) { const float c = o.v_end * o.v_end; if (c < Li) { Li = c; code = 5; } }
    }
    sL[t] = Li;
    __syncthreads();

    // the own row of the lower envelope: a minimum, so the order of j is free; the code is the own limit's unless a cone is
    // strictly below it, the acceleration cones (j < i) before the braking cones
    const float ta = 2.f * o.a_max, td = 2.f * o.d_max;
    float u = Li;
    if (t < N) {
        for (int j = 0; j < N; ++j) {
            const float c = j < t ? sL[j] + ta * (S - sS[j]) : sL[j] + td * (sS[j] - S);
            if (j != t && c < u) { u = c; code = j < t ? 6 : 7; }
        }
    }
    const float v = t < N ? sqrtf(u) : 0.f;
    sv[t] = v;
    scode[t] = (unsigned char)code;
    __syncthreads();
    float dt = 0.f;
    if (t <= N - 2 && ds != 0.f) dt = (2.f * ds) / (v + sv[t + 1]);
    sdt[t] = dt;
    __syncthreads();
    float tm = 0.f;
    if (t < N) {
        for (int j = 0; j < t; ++j) tm = tm + sdt[j];
        vout[base + t] = v; tout[base + t] = tm; lim[base + t] = (unsigned char)code;
    }
    const float vmax = block_reduce(v, OpMaxNan(), swf, nthr, 0.f);
    const float kmax = block_reduce(kappa, OpMaxNan(), swf, nthr, 0.f);
    const int bad = block_reduce(isfinite(dt) ? 0 : 1, OpMax(), swi, nthr, 0);
    if (t == 0) {
        tsum[(size_t)tr * 3 + 1] = vmax; tsum[(size_t)tr * 3 + 2] = kmax;
        tint[(size_t)tr * 9] = bad ? 3 : 0;
    }
    if (t == N - 1) tsum[(size_t)tr * 3] = tm;
    if (t < 8) {
        int cnt = 0;
        for (int j = 0; j < N; ++j) cnt += scode[j] == t ? 1 : 0;
        tint[(size_t)tr * 9 + 1 + t] = cnt;
    }
}

// The timed position at tau: the last waypoint from the duration on, else the segment by bisection (the largest i <= N - 2 with
// t_i <= tau) and the distance along it under constant acceleration.  USER: 0 for the timing's and the check's kernels, 1 for
// those that read or make a schedule -- the same statements, instantiated apart: a function of this file has
// internal linkage, so what the compiler learns from one kernel's arguments would else reach the code of the others.
template <int DIM, int USER = 0>
__device__ __forceinline__ void traj_position(const float* __restrict__ x, const float* __restrict__ v, const float* st, int N,
                                              double tau, double* p) {
    if (tau >= (double)st[N - 1]) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) p[a] = (double)x[(size_t)(N - 1) * DIM + a];
        return;
    }
    int lo = 0, hi = N - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((double)st[mid] <= tau) lo = mid; else hi = mid - 1;
    }
    const double ti = (double)st[lo], h = (double)st[lo + 1] - ti, e = tau - ti, vi = (double)v[lo];
    const double acc = ((double)v[lo + 1] - vi) / h;
    const double s = vi * e + ((0.5 * acc) * e) * e;
    double d[DIM], x0[DIM], sq = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        x0[a] = (double)x[(size_t)lo * DIM + a];
        d[a] = (double)x[(size_t)(lo + 1) * DIM + a] - x0[a];
        sq = a ? sq + d[a] * d[a] : d[a] * d[a];
    }
    double w = s / sqrt(sq);
    w = w > 0.0 ? w : 0.0;
    w = w < 1.0 ? w : 1.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = x0[a] + w * d[a];
}

// A schedule of gpis_retime_solve as its readers see it: res[tr][kSchedRes] = status, arrive, pauses, own_slots,
// first_pause; own[tr][kOwnLen] the own slot of every real slot (own_slots from arrive on); k0: the real slot a sequence starts at.
constexpr int kSchedRes = Trajectories::kSchedRes, kOwnLen = Trajectories::kOwnLen, kMaxOwnSlots = Trajectories::kMaxOwnSlots;

struct TrajSched {
    const int* res;
    const int* own;
    int k0;
};

__device__ __forceinline__ int sched_own(const TrajSched& sc, int tr, int k) {
    return k < kOwnLen ? sc.own[(size_t)tr * kOwnLen + k] : sc.res[(size_t)tr * kSchedRes + 3];
}

// One workgroup per trajectory (first + blockIdx.x), blockDim.x = 64 ceil(T / 64), thread k = step k: its two timed positions,
// the displacement, the heading of the latest moving step by an integer max-scan, the controls.  U[blockIdx.x][T][nu],
// hp[blockIdx.x][5] = heading0, p_0, clamped[blockIdx.x].  Double, nothing contracted.
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_controls_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                               const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                               int T, int first, double dt, double t0, double w_limit,
                                                               double min_move, double* __restrict__ U, double* __restrict__ hp,
                                                               int* __restrict__ clamped) {
#define TRAJ_SCHED 0
#include "traj_controls_body.inc"
#undef TRAJ_SCHED
}

// the same along a schedule (the contract: tests/retime_ref.py): dt is the schedule's slot
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_retime_controls_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                      const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                      int T, int first, double dt, double w_limit, double min_move,
                                                                      double* __restrict__ U, double* __restrict__ hp,
                                                                      int* __restrict__ clamped, TrajSched sc) {
#define TRAJ_SCHED 1
#include "traj_controls_body.inc"
#undef TRAJ_SCHED
}

// A timed trajectory against a set of moving balls (obst.h; the contract: tests/obst_ref.py).  One workgroup of
// kBlock threads per trajectory.  The intervals are taken in chunks of kChunk: the timed positions p_k of a chunk (and the one
// that ends it) go to LDS once, by traj_position; then a thread per interval loops over the table (its index is the same in every
// lane: scalar loads) and keeps its own least (sep, k, i) -- it meets its intervals and the balls in ascending order, so a
// strict comparison keeps the smallest (k, i) -- and the first interval with a sep below the clearance.  The block's result:
// the least sep (a min of doubles that are never NaN where they were taken: order-free), then the least key (k << 8 | i) among
// the threads that hold it, and the thread that owns that key writes.  Double, nothing contracted.  out_d[tr][2] = min_sep,
// min_time; out_i[tr][3] = min_obstacle, first_hit, collides.
constexpr int kChunk = 1024;

template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_obst_check_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                 const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                 int steps, double dt, double t0, double TB, double clearance,
                                                                 const double* __restrict__ tab, int n, double* __restrict__ out_d,
                                                                 int* __restrict__ out_i) {
#define TRAJ_SCHED 0
#include "traj_check_body.inc"
#undef TRAJ_SCHED
}

// the same along a schedule: dt is the schedule's slot, min_time is in real time
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_retime_check_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                   const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                   int steps, double dt, double TB, double clearance,
                                                                   const double* __restrict__ tab, int n, double* __restrict__ out_d,
                                                                   int* __restrict__ out_i, TrajSched sc) {
    constexpr double t0 = 0.0;
#define TRAJ_SCHED 1
#include "traj_check_body.inc"
#undef TRAJ_SCHED
}

// ---- re-timing: when to move along a timed trajectory so that moving balls pass ----------------------------------
// The contract: tests/retime_ref.py.  One workgroup of kBlock threads per trajectory; lane = pause count p, rows = own slots a
// taken in order, the real slot of cell (a, p) is a + p.  pos_a = traj_position((double)a * slot), a = 0 .. A, go to LDS once
// (<= 1025 x DIM doubles).  A row: the lanes whose cell can still be reached evaluate its pause flag (no ball's separation of
// (pos_a, 0) at slot a + p below the clearance; the table's index is the same in every lane: scalar loads); the wavefronts'
// ballots of the seeds (reached from row a - 1 by a free play cell) and of the pause flags meet in LDS, and after one barrier
// every lane floods the seeds along the open pause links, a wavefront's 64 cells by shifts of one word, the carry into the next
// wavefront a bit; then only the reached lanes evaluate the play flag that seeds row a + 1.  Reach bits live in registers from
// row to row; what the walk back needs goes to LDS, one bit per cell (1025 x 256 bits = 32.8 KB): with press_on 0 "reached by a
// play step", with press_on 1 "reached by a pause step".  The walk back is lane 0's.  Integers and flags: nothing depends on an
// order.  At worst A (P + 1) 2 n separations per trajectory.
// res[tr][kSchedRes] = status, arrive, pauses, own_slots, first_pause; own[tr][kOwnLen].

// The separation of one interval from one ball for gpis_retime_solve's cells: the expression of the check's inner loop
// (traj_check_body.inc), operation for operation (that loop keeps its own text, so that the plain check kernels compile to what they were; the
// certificate of tests/test_gpu_retime.py holds the two together).  The robot goes from p0 by dp while the ball of `row` goes
// from its place at the elapsed time e0 to that at e1; *s_out = where in the interval the two are closest.
template <int DIM>
__device__ __forceinline__ double traj_ball_sep(const double* p0, const double* dp, double e0, double e1,
                                                const double* __restrict__ row, double* s_out) {
    double A[DIM], B[DIM], bb = 0.0, ab = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double o0 = row[a] + row[3 + a] * e0, o1 = row[a] + row[3 + a] * e1;
        A[a] = p0[a] - o0;
        B[a] = dp[a] - (o1 - o0);
        bb = a ? bb + B[a] * B[a] : B[a] * B[a];
        ab = a ? ab + A[a] * B[a] : A[a] * B[a];
    }
    double s = 0.0;
    if (bb > 0.0) {
        s = (-ab) / bb;
        s = s > 0.0 ? s : 0.0;
        s = s < 1.0 ? s : 1.0;
    }
    double s2 = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double q = A[a] + s * B[a];
        s2 = a ? s2 + q * q : q * q;
    }
    *s_out = s;
    return sqrt(s2) - row[6];
}

template <int DIM>
__device__ __forceinline__ bool retime_cell_free(const double* p0, const double* dp, double e0, double e1,
                                                 const double* __restrict__ tab, int n, double clearance) {
    bool ok = true;
    const double* __restrict__ row = tab;
    for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
        double s;
        const double sep = traj_ball_sep<DIM>(p0, dp, e0, e1, row, &s);
        ok = ok && !(sep < clearance);                   // (a NaN separation is not below the clearance, as in the check)
    }
    return ok;
}

template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_retime_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                             const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                             double slot, int P, double clearance, int press_on, double TB,
                                                             const double* __restrict__ tab, int n, int* __restrict__ res,
                                                             int* __restrict__ own) {
    typedef unsigned long long u64;
    __shared__ float st[kTree];
    __shared__ double sp[kMaxOwnSlots + 1][DIM];
    __shared__ u64 spred[kMaxOwnSlots + 1][kBlock / 64];
    __shared__ u64 smask[2][2][kBlock / 64];             // [row parity][seeds, pause flags][wavefront]
    const int tr = blockIdx.x, p = threadIdx.x, lane = p & 63, w = p >> 6;
    const size_t base = (size_t)tr * N;
    int* ro = res + (size_t)tr * kSchedRes;
    int* oo = own + (size_t)tr * kOwnLen;

    int A = -1, status = 2;
    if (tint[(size_t)tr * 9] == 0) {                     // (uniform: one trajectory per workgroup)
        for (int i = p; i < N; i += kBlock) st[i] = tt[base + i];
        const double dur = (double)tt[base + N - 1];
        status = 4;
        if (dur / slot <= (double)(kMaxOwnSlots + 2)) {
            int a = (int)(dur / slot);
            while (a > 0 && (double)(a - 1) * slot >= dur) --a;
            while ((double)a * slot < dur) ++a;
            if (a <= kMaxOwnSlots) { A = a; status = 0; }
        }
    }
    if (status != 0) {                                   // no timing, or too long for this slot
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = -1;
        if (p == 0) { ro[0] = status; ro[1] = -1; ro[2] = -1; ro[3] = -1; ro[4] = -1; }
        return;
    }
    if (n == 0) {                                        // nothing to wait for: the identity
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = min(k, A);
        if (p == 0) { ro[0] = 0; ro[1] = A; ro[2] = 0; ro[3] = A; ro[4] = -1; }
        return;
    }
    __syncthreads();                                     // (st is written)
    for (int j = p; j <= A; j += kBlock) {
        double q[DIM];
        traj_position<DIM, 1>(x + base * DIM, v + base, st, N, (double)j * slot, q);
#pragma unroll
        for (int a = 0; a < DIM; ++a) sp[j][a] = q[a];
    }
    __syncthreads();

    bool seed = p == 0;
    int lo = 0, pstar = -1;                              // lo: the least reached p of the row before
    for (int a = 0; a <= A; ++a) {
        double pa[DIM], dp[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) { pa[c] = sp[a][c]; dp[c] = 0.0; }
        const double e0 = TB + (double)(a + p) * slot, e1 = TB + (double)(a + p + 1) * slot;
        bool f = false;
        // (row A needs no pause: a cell reached there by one has a reached cell of a smaller p before it)
        if (a < A && p < P && p >= lo) f = retime_cell_free<DIM>(pa, dp, e0, e1, tab, n, clearance);
        const u64 S = __ballot(seed), F = __ballot(f);
        if (lane == 0) { smask[a & 1][0][w] = S; smask[a & 1][1][w] = F; }
        __syncthreads();                                 // (the other parity is free: every lane has passed the barrier after its reads)
        u64 cin = 0, mine = 0, any = 0;
        int first = -1;
#pragma unroll
        for (int q = 0; q < kBlock / 64; ++q) {
            const u64 sq = smask[a & 1][0][q], fq = smask[a & 1][1][q];
            u64 r = sq | cin, open = fq;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {           // cells reached within 2 d - 1 pauses; open: d links in a row from here
                r |= (r & open) << d;
                open &= open >> d;
            }
            const u64 by_pause = ((r & fq) << 1) | cin;
            if (q == w) {
                mine = r;
                if (lane == 0) spred[a][w] = press_on ? by_pause : sq;
            }
            if (first < 0 && r) first = q * 64 + (__ffsll(r) - 1);
            any |= r;
            cin = (r & fq) >> 63;
        }
        if (!any) break;                                 // (uniform) no cell of this row is reached: none of a later one
        lo = first;
        if (a == A) { pstar = first; break; }
#pragma unroll
        for (int c = 0; c < DIM; ++c) dp[c] = sp[a + 1][c] - pa[c];
        seed = ((mine >> lane) & 1) ? retime_cell_free<DIM>(pa, dp, e0, e1, tab, n, clearance) : false;
    }
    if (pstar < 0) {                                     // no schedule within P pauses
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = -1;
        if (p == 0) { ro[0] = 3; ro[1] = -1; ro[2] = -1; ro[3] = A; ro[4] = -1; }
        return;
    }
    const int arrive = A + pstar;
    for (int k = arrive + 1 + p; k < kOwnLen; k += kBlock) oo[k] = A;
    __syncthreads();                                     // (spred is written)
    if (p == 0) {
        int a = A, pp = pstar, fp = -1;
        oo[arrive] = A;
        while (a > 0 || pp > 0) {
            const bool bit = (spred[a][pp >> 6] >> (pp & 63)) & 1;
            bool play = press_on ? !bit : bit;
            if (a == 0) play = false;                    // (what the bits say there anyway; the walk ends whatever they hold)
            else if (pp == 0) play = true;
            if (play) --a;
            else { --pp; fp = a + pp; }
            oo[a + pp] = a;
        }
        ro[0] = pstar > 0 ? 1 : 0; ro[1] = arrive; ro[2] = pstar; ro[3] = A; ro[4] = fp;
    }
}

// A footprint (body.h; the contract: tests/body_ref.py) along a smoothed trajectory.  One workgroup of kBlock
// threads per trajectory, a thread per waypoint.  The waypoints go to LDS once; a thread finds the chord that gives its waypoint
// a heading -- the first chord k >= min(i, N - 2) with a horizontal length > 0, else the last one before, else (1, 0); double from
// the float32 waypoints -- and applies the body rule there.  The block's result: the least D (a min of doubles that are never NaN
// where they were taken: order-free), then the least waypoint among the threads that hold it, and that thread writes.
// out_d[tr] = D_min; out_i[tr][3] = waypoint, ball, collides.  A trajectory without a result (status 2): NaN, -1, -1, 0.
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_body_check_kernel(const float* __restrict__ F, DfLattice L, BodyArgs bd,
                                                                 const float* __restrict__ x, const int* __restrict__ ires, int N,
                                                                 double clearance, double* __restrict__ out_d, int* __restrict__ out_i) {
    __shared__ float sx[kTree][2];
    __shared__ double shd[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, i = threadIdx.x;
    const float* __restrict__ xt = x + (size_t)tr * N * DIM;
    if (ires[(size_t)tr * 4] == 2) {
        if (i == 0) {
            out_d[tr] = (double)NAN;
            out_i[(size_t)tr * 3] = -1; out_i[(size_t)tr * 3 + 1] = -1; out_i[(size_t)tr * 3 + 2] = 0;
        }
        return;
    }
    if (i < N) { sx[i][0] = xt[(size_t)i * DIM]; sx[i][1] = xt[(size_t)i * DIM + 1]; }
    __syncthreads();
    DfLattice Lc = L;
    Lc.dim = DIM;
    double best = INFINITY;
    int wp = -1, jm = -1, bad = 0, off = 0;
    if (i < N) {
        const TrajChord h = traj_chord_heading(&sx[0][0], &sx[0][1], 2, i, N);
        double p[3] = {(double)sx[i][0], (double)sx[i][1], DIM == 3 ? (double)xt[(size_t)i * DIM + 2] : 0.0};
        const double d = body_clearance_at<DIM>(F, Lc, bd.tab, bd.m, p, h.c, h.s, &jm);
        if (d != d) { off = 1; bad = 1; }
        else {
            bad = d < clearance ? 1 : 0;
            if (d < best) { best = d; wp = i; }
        }
    }
    const double bmin = block_reduce(best, OpMin(), shd, kBlock, (double)INFINITY);
    if (i == 0) shd[0] = bmin;
    __syncthreads();
    const double least = shd[0];
    const int key = wp >= 0 && best == least ? wp : 0x7fffffff;
    const int kmin = block_reduce(key, OpMin(), shi, kBlock, 0x7fffffff);
    if (i == 0) shi[0] = kmin;
    __syncthreads();
    const int win = shi[0];
    __syncthreads();
    const int nbad = block_reduce(bad, OpAdd(), shi, kBlock, 0);
    const int noff = block_reduce(off, OpAdd(), shi, kBlock, 0);
    if (i == 0) {
        out_i[(size_t)tr * 3 + 2] = nbad > 0 ? 1 : 0;
        if (win == 0x7fffffff) {                         // no waypoint gave a D below +inf
            out_d[tr] = noff == N ? (double)NAN : (double)INFINITY;
            out_i[(size_t)tr * 3] = -1; out_i[(size_t)tr * 3 + 1] = -1;
        }
    }
    if (wp >= 0 && wp == win) {
        out_d[tr] = best;
        out_i[(size_t)tr * 3] = wp; out_i[(size_t)tr * 3 + 1] = jm;
    }
}

// ---- the footprint against moving balls along a timed trajectory and in its re-timing --------------------------
// The contract: tests/body_time_ref.py.  The timed pose at tau is (p, c, s): p is traj_position's timed position, i(tau) the
// segment its bisection ends on (N - 1 from the duration on), (c, s) the chord rule's heading of waypoint i(tau).  The two
// functions below restate traj_position and traj_chord_heading statement for statement and are called by the kernels of this
// section alone: a function of this file has internal linkage, and a new caller of the old ones would reach the code of the
// kernels that call them (§7w).  For the same reason this section writes its minima of two integers as conditionals: the
// header's min(int, int) is such a shared function too, and new calls of it changed the bisection of the plain check kernels.

// traj_position's statements; returns the segment index
template <int DIM>
__device__ __forceinline__ int traj_pose_position(const float* __restrict__ x, const float* __restrict__ v, const float* st, int N,
                                                  double tau, double* p) {
    if (tau >= (double)st[N - 1]) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) p[a] = (double)x[(size_t)(N - 1) * DIM + a];
        return N - 1;
    }
    int lo = 0, hi = N - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((double)st[mid] <= tau) lo = mid; else hi = mid - 1;
    }
    const double ti = (double)st[lo], h = (double)st[lo + 1] - ti, e = tau - ti, vi = (double)v[lo];
    const double acc = ((double)v[lo + 1] - vi) / h;
    const double s = vi * e + ((0.5 * acc) * e) * e;
    double d[DIM], x0[DIM], sq = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        x0[a] = (double)x[(size_t)lo * DIM + a];
        d[a] = (double)x[(size_t)(lo + 1) * DIM + a] - x0[a];
        sq = a ? sq + d[a] * d[a] : d[a] * d[a];
    }
    double w = s / sqrt(sq);
    w = w > 0.0 ? w : 0.0;
    w = w < 1.0 ? w : 1.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = x0[a] + w * d[a];
    return lo;
}

// traj_chord_heading's rule on the waypoints x[k * DIM + {0, 1}]: (c, s) of waypoint i
template <int DIM>
__device__ __forceinline__ void traj_pose_heading(const float* __restrict__ x, int i, int N, double* c, double* s) {
    const int k0 = i < N - 2 ? i : N - 2;
    *c = 1.0; *s = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = pass == 0 ? k0 : k0 - 1; pass == 0 ? k <= N - 2 : k >= 0; k += pass == 0 ? 1 : -1) {
            const double e0 = (double)x[(size_t)(k + 1) * DIM] - (double)x[(size_t)k * DIM];
            const double e1 = (double)x[(size_t)(k + 1) * DIM + 1] - (double)x[(size_t)k * DIM + 1];
            const double n2 = e0 * e0 + e1 * e1;
            if (n2 > 0.0) {
                const double nn = sqrt(n2);
                *c = e0 / nn; *s = e1 / nn;
                return;
            }
        }
    }
}

// the pose q[DIM + 2] = (p, c, s) at tau
template <int DIM>
__device__ __forceinline__ void traj_pose_at(const float* __restrict__ x, const float* __restrict__ v, const float* st, int N, double tau,
                                             double* q) {
    const int i = traj_pose_position<DIM>(x, v, st, N, tau, q);
    traj_pose_heading<DIM>(x, i, N, &q[DIM], &q[DIM + 1]);
}

// where ball `row` of the body sits at the pose q (the body rule's position, §7r: body_ball_at's statements)
template <int DIM>
__device__ __forceinline__ void traj_pose_ball(const double* __restrict__ row, const double* q, double* w) {
    const double b0 = row[0], b1 = row[1], c = q[DIM], s = q[DIM + 1];
    w[0] = q[0] + (c * b0 - s * b1);
    w[1] = q[1] + (s * b0 + c * b1);
    if constexpr (DIM == 3) w[2] = q[2] + row[2];
}

// the separation of one interval of one body ball's centre (from w0 by dw) from the moving ball of `row`, less the body ball's
// radius: the expression of the check's inner loop, operation for operation
template <int DIM>
__device__ __forceinline__ double traj_body_ball_sep(const double* w0, const double* dw, double e0, double e1,
                                                     const double* __restrict__ row, double rho, double* s_out) {
    double A[DIM], B[DIM], bb = 0.0, ab = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double o0 = row[a] + row[3 + a] * e0, o1 = row[a] + row[3 + a] * e1;
        A[a] = w0[a] - o0;
        B[a] = dw[a] - (o1 - o0);
        bb = a ? bb + B[a] * B[a] : B[a] * B[a];
        ab = a ? ab + A[a] * B[a] : A[a] * B[a];
    }
    double s = 0.0;
    if (bb > 0.0) {
        s = (-ab) / bb;
        s = s > 0.0 ? s : 0.0;
        s = s < 1.0 ? s : 1.0;
    }
    double s2 = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double q = A[a] + s * B[a];
        s2 = a ? s2 + q * q : q * q;
    }
    *s_out = s;
    return (sqrt(s2) - row[6]) - rho;
}

// The timed poses of every trajectory: out[tr][steps + 1][DIM + 2].  SCHED 0: at t0 + k dt; SCHED 1: at the own slot own(k) of
// the schedule `sc`, dt its slot.  A trajectory without a timing (SCHED 1: or without a schedule): NaN.
template <int DIM, int SCHED>
__global__ void __launch_bounds__(kBlock) traj_body_states_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                  const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                  int steps, double dt, double t0, double* __restrict__ out,
                                                                  TrajSched sc) {
    __shared__ float st[kTree];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)tr * N;
    double* o = out + (size_t)tr * (steps + 1) * (DIM + 2);
    bool timed = tint[(size_t)tr * 9] == 0;
    if constexpr (SCHED) timed = timed && sc.res[(size_t)tr * kSchedRes] < 2;
    if (!timed) {                                        // (uniform: one trajectory per workgroup)
        for (int j = tid; j < (steps + 1) * (DIM + 2); j += kBlock) o[j] = (double)NAN;
        return;
    }
    for (int i = tid; i < N; i += kBlock) st[i] = tt[base + i];
    __syncthreads();
    for (int j = tid; j <= steps; j += kBlock) {
        double q[DIM + 2];
        const double tau = SCHED ? (double)sched_own(sc, tr, j) * dt : t0 + (double)j * dt;
        traj_pose_at<DIM>(x + base * DIM, v + base, st, N, tau, q);
#pragma unroll
        for (int a = 0; a < DIM + 2; ++a) o[(size_t)j * (DIM + 2) + a] = q[a];
    }
}

// traj_obst_check_kernel / traj_retime_check_kernel (SCHED 1) with the footprint bd.  The chunk's poses go to LDS once; a thread
// per interval takes the body balls j (the footprint's rows: the same index in every lane, scalar loads) and inside them the
// moving balls i (the same), and keeps its own least (sep, k, i, j): it meets k ascending, and within an interval a later pair
// replaces the kept one if its sep is smaller, or equal with a smaller i (its j is the larger one).  The block's result: the
// least sep, then the least key (k << 12 | i << 4 | j) among the threads that hold it.  out_d[tr][2] = min_sep, min_time;
// out_i[tr][4] = min_obstacle, first_hit, collides, min_ball.
template <int DIM, int SCHED>
__global__ void __launch_bounds__(kBlock) traj_body_time_check_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                      const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                      int steps, double dt, double t0, double TB, double clearance,
                                                                      const double* __restrict__ tab, int n, BodyArgs bd,
                                                                      double* __restrict__ out_d, int* __restrict__ out_i, TrajSched sc) {
    typedef unsigned long long u64;
    __shared__ float st[kTree];
    __shared__ double sq[kChunk + 1][DIM + 2];
    __shared__ double shd[kBlock / 64];
    __shared__ u64 shk[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)tr * N;
    bool timed = tint[(size_t)tr * 9] == 0;
    if constexpr (SCHED) timed = timed && sc.res[(size_t)tr * kSchedRes] < 2;
    if (!timed || n == 0) {
        if (tid == 0) {
            out_d[(size_t)tr * 2] = timed ? (double)INFINITY : (double)NAN; out_d[(size_t)tr * 2 + 1] = (double)NAN;
            out_i[(size_t)tr * 4] = -1; out_i[(size_t)tr * 4 + 1] = -1; out_i[(size_t)tr * 4 + 2] = 0; out_i[(size_t)tr * 4 + 3] = -1;
        }
        return;
    }
    for (int i = tid; i < N; i += kBlock) st[i] = tt[base + i];
    double best = INFINITY, best_s = 0.0;
    int best_k = -1, best_i = -1, best_j = -1, hit = 0x7fffffff;
    for (int k0 = 0; k0 < steps; k0 += kChunk) {
        const int cnt = steps - k0 < kChunk ? steps - k0 : kChunk;
        __syncthreads();                                 // (st is written; sq of the previous chunk is read)
        for (int j = tid; j <= cnt; j += kBlock) {
            double q[DIM + 2];
            const double tau = SCHED ? (double)sched_own(sc, tr, k0 + j) * dt : t0 + (double)(k0 + j) * dt;
            traj_pose_at<DIM>(x + base * DIM, v + base, st, N, tau, q);
#pragma unroll
            for (int a = 0; a < DIM + 2; ++a) sq[j][a] = q[a];
        }
        __syncthreads();
        for (int jj = tid; jj < cnt; jj += kBlock) {
            const int k = k0 + jj;
            const double e0 = TB + (t0 + (double)k * dt), e1 = TB + (t0 + (double)(k + 1) * dt);
            double q0[DIM + 2], q1[DIM + 2];
#pragma unroll
            for (int a = 0; a < DIM + 2; ++a) { q0[a] = sq[jj][a]; q1[a] = sq[jj + 1][a]; }
            const double* __restrict__ brow = bd.tab;
            for (int j = 0; j < bd.m; ++j, brow += 4) {
                double w0[DIM], w1[DIM], dw[DIM];
                traj_pose_ball<DIM>(brow, q0, w0);
                traj_pose_ball<DIM>(brow, q1, w1);
#pragma unroll
                for (int a = 0; a < DIM; ++a) dw[a] = w1[a] - w0[a];
                const double rho = brow[3];
                const double* __restrict__ row = tab;
                for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
                    double s;
                    const double sep = traj_body_ball_sep<DIM>(w0, dw, e0, e1, row, rho, &s);
                    if (sep < best || (sep == best && k == best_k && i < best_i)) { best = sep; best_s = s; best_k = k; best_i = i; best_j = j; }
                    if (sep < clearance && k < hit) hit = k;
                }
            }
        }
    }
    const double bmin = block_reduce(best, OpMin(), shd, kBlock, (double)INFINITY);
    if (tid == 0) shd[0] = bmin;
    __syncthreads();
    const double least = shd[0];
    const u64 key = best_k >= 0 && best == least ? ((u64)best_k << 12) | ((u64)best_i << 4) | (u64)best_j : ~0ull;
    const u64 kmin = block_reduce(key, OpMin(), shk, kBlock, ~0ull);
    if (tid == 0) shk[0] = kmin;
    __syncthreads();
    const u64 win = shk[0];
    const int fh = block_reduce(hit, OpMin(), shi, kBlock, 0x7fffffff);
    if (tid == 0) {
        out_i[(size_t)tr * 4 + 1] = fh == 0x7fffffff ? -1 : fh;
        out_i[(size_t)tr * 4 + 2] = fh == 0x7fffffff ? 0 : 1;
        if (win == ~0ull) {                              // no separation was a number
            out_d[(size_t)tr * 2] = (double)INFINITY; out_d[(size_t)tr * 2 + 1] = (double)NAN;
            out_i[(size_t)tr * 4] = -1; out_i[(size_t)tr * 4 + 3] = -1;
        }
    }
    if (key == win && win != ~0ull) {
        out_d[(size_t)tr * 2] = best;
        out_d[(size_t)tr * 2 + 1] = (t0 + (double)best_k * dt) + best_s * dt;
        out_i[(size_t)tr * 4] = best_i; out_i[(size_t)tr * 4 + 3] = best_j;
    }
}

// a cell of the body's re-timing: no (body ball, moving ball) pair's separation is below the clearance while the body goes from
// the pose q0 to q1 (a pause: q1 = q0 and every ball's displacement is 0) during the real slot [e0, e1]
template <int DIM, bool PAUSE>
__device__ __forceinline__ bool retime_body_cell_free(const double* q0, const double* q1, double e0, double e1,
                                                      const double* __restrict__ tab, int n, BodyArgs bd, double clearance) {
    bool ok = true;
    const double* __restrict__ brow = bd.tab;
    for (int j = 0; j < bd.m; ++j, brow += 4) {
        double w0[DIM], dw[DIM];
        traj_pose_ball<DIM>(brow, q0, w0);
        if constexpr (PAUSE) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) dw[a] = 0.0;
        } else {
            double w1[DIM];
            traj_pose_ball<DIM>(brow, q1, w1);
#pragma unroll
            for (int a = 0; a < DIM; ++a) dw[a] = w1[a] - w0[a];
        }
        const double rho = brow[3];
        const double* __restrict__ row = tab;
        for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
            double s;
            const double sep = traj_body_ball_sep<DIM>(w0, dw, e0, e1, row, rho, &s);
            ok = ok && !(sep < clearance);               // (a NaN separation is not below the clearance, as in the check)
        }
    }
    return ok;
}

// traj_retime_kernel with the footprint bd: the same rows, ballots, flood and walk; a cell's flags range over the pairs (body
// ball, moving ball).  The table in LDS is the timed position and the segment index of every own slot (a byte: N <= 256) and the
// chord rule's heading of every waypoint, which is the pose of every own slot -- the body holds its segment's heading -- in
// (1025 DIM + 512) doubles and 1025 bytes: one chord search per waypoint, and the kernel's LDS stays below 64 KB with the walk's bits
// as the point kernel's does.
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_body_retime_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                                  const float* __restrict__ tt, const int* __restrict__ tint, int N,
                                                                  double slot, int P, double clearance, int press_on, double TB,
                                                                  const double* __restrict__ tab, int n, BodyArgs bd,
                                                                  int* __restrict__ res, int* __restrict__ own) {
    typedef unsigned long long u64;
    __shared__ float st[kTree];
    __shared__ double sp[kMaxOwnSlots + 1][DIM];
    __shared__ double shead[kTree][2];
    __shared__ unsigned char sseg[kMaxOwnSlots + 4];
    __shared__ u64 spred[kMaxOwnSlots + 1][kBlock / 64];
    __shared__ u64 smask[2][2][kBlock / 64];             // [row parity][seeds, pause flags][wavefront]
    const int tr = blockIdx.x, p = threadIdx.x, lane = p & 63, w = p >> 6;
    const size_t base = (size_t)tr * N;
    int* ro = res + (size_t)tr * kSchedRes;
    int* oo = own + (size_t)tr * kOwnLen;

    int A = -1, status = 2;
    if (tint[(size_t)tr * 9] == 0) {                     // (uniform: one trajectory per workgroup)
        for (int i = p; i < N; i += kBlock) st[i] = tt[base + i];
        const double dur = (double)tt[base + N - 1];
        status = 4;
        if (dur / slot <= (double)(kMaxOwnSlots + 2)) {
            int a = (int)(dur / slot);
            while (a > 0 && (double)(a - 1) * slot >= dur) --a;
            while ((double)a * slot < dur) ++a;
            if (a <= kMaxOwnSlots) { A = a; status = 0; }
        }
    }
    if (status != 0) {                                   // no timing, or too long for this slot
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = -1;
        if (p == 0) { ro[0] = status; ro[1] = -1; ro[2] = -1; ro[3] = -1; ro[4] = -1; }
        return;
    }
    if (n == 0) {                                        // nothing to wait for: the identity
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = k < A ? k : A;
        if (p == 0) { ro[0] = 0; ro[1] = A; ro[2] = 0; ro[3] = A; ro[4] = -1; }
        return;
    }
    __syncthreads();                                     // (st is written)
    for (int j = p; j <= A; j += kBlock) {
        double q[DIM];
        const int i = traj_pose_position<DIM>(x + base * DIM, v + base, st, N, (double)j * slot, q);
#pragma unroll
        for (int a = 0; a < DIM; ++a) sp[j][a] = q[a];
        sseg[j] = (unsigned char)i;
    }
    for (int i = p; i < N; i += kBlock) {
        double c, s;
        traj_pose_heading<DIM>(x + base * DIM, i, N, &c, &s);
        shead[i][0] = c; shead[i][1] = s;
    }
    __syncthreads();

    bool seed = p == 0;
    int lo = 0, pstar = -1;                              // lo: the least reached p of the row before
    for (int a = 0; a <= A; ++a) {
        double qa[DIM + 2], qb[DIM + 2];
        const int ia = sseg[a];
#pragma unroll
        for (int c = 0; c < DIM; ++c) qa[c] = sp[a][c];
        qa[DIM] = shead[ia][0]; qa[DIM + 1] = shead[ia][1];
        const double e0 = TB + (double)(a + p) * slot, e1 = TB + (double)(a + p + 1) * slot;
        bool f = false;
        // (row A needs no pause: a cell reached there by one has a reached cell of a smaller p before it)
        if (a < A && p < P && p >= lo) f = retime_body_cell_free<DIM, true>(qa, qa, e0, e1, tab, n, bd, clearance);
        const u64 S = __ballot(seed), F = __ballot(f);
        if (lane == 0) { smask[a & 1][0][w] = S; smask[a & 1][1][w] = F; }
        __syncthreads();                                 // (the other parity is free: every lane has passed the barrier after its reads)
        u64 cin = 0, mine = 0, any = 0;
        int first = -1;
#pragma unroll
        for (int q = 0; q < kBlock / 64; ++q) {
            const u64 sq = smask[a & 1][0][q], fq = smask[a & 1][1][q];
            u64 r = sq | cin, open = fq;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {           // cells reached within 2 d - 1 pauses; open: d links in a row from here
                r |= (r & open) << d;
                open &= open >> d;
            }
            const u64 by_pause = ((r & fq) << 1) | cin;
            if (q == w) {
                mine = r;
                if (lane == 0) spred[a][w] = press_on ? by_pause : sq;
            }
            if (first < 0 && r) first = q * 64 + (__ffsll(r) - 1);
            any |= r;
            cin = (r & fq) >> 63;
        }
        if (!any) break;                                 // (uniform) no cell of this row is reached: none of a later one
        lo = first;
        if (a == A) { pstar = first; break; }
        const int ib = sseg[a + 1];
#pragma unroll
        for (int c = 0; c < DIM; ++c) qb[c] = sp[a + 1][c];
        qb[DIM] = shead[ib][0]; qb[DIM + 1] = shead[ib][1];
        seed = ((mine >> lane) & 1) ? retime_body_cell_free<DIM, false>(qa, qb, e0, e1, tab, n, bd, clearance) : false;
    }
    if (pstar < 0) {                                     // no schedule within P pauses
        for (int k = p; k < kOwnLen; k += kBlock) oo[k] = -1;
        if (p == 0) { ro[0] = 3; ro[1] = -1; ro[2] = -1; ro[3] = A; ro[4] = -1; }
        return;
    }
    const int arrive = A + pstar;
    for (int k = arrive + 1 + p; k < kOwnLen; k += kBlock) oo[k] = A;
    __syncthreads();                                     // (spred is written)
    if (p == 0) {
        int a = A, pp = pstar, fp = -1;
        oo[arrive] = A;
        while (a > 0 || pp > 0) {
            const bool bit = (spred[a][pp >> 6] >> (pp & 63)) & 1;
            bool play = press_on ? !bit : bit;
            if (a == 0) play = false;                    // (what the bits say there anyway; the walk ends whatever they hold)
            else if (pp == 0) play = true;
            if (play) --a;
            else { --pp; fp = a + pp; }
            oo[a + pp] = a;
        }
        ro[0] = pstar > 0 ? 1 : 0; ro[1] = arrive; ro[2] = pstar; ro[3] = A; ro[4] = fp;
    }
}

}  // namespace

int traj_check_opts(const TrajOpts& o) {
    auto nonneg = [](float v) { return std::isfinite(v) && v >= 0.f; };
    if (!std::isfinite(o.clearance) || !(std::isfinite(o.margin) && o.margin > 0.f)) return GPIS_ERR_ARG;
    if (!nonneg(o.w_smooth) || !nonneg(o.w_obs) || !nonneg(o.rate) || !nonneg(o.max_move) || !nonneg(o.tol)) return GPIS_ERR_ARG;
    if (o.iters < 0 || o.sub < 0 || o.sub > Trajectories::kMaxSub) return GPIS_ERR_ARG;
    return GPIS_OK;
}

Trajectories::Trajectories() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Trajectories::~Trajectories() {
    has_input = false;
    (void)bind(-1);
}

int Trajectories::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    std::vector<float> hx;
    std::vector<unsigned char> hs;
    const bool carry = has_input && dev >= 0;
    const int cm = m, cN = N, cdim = dim;
    int rc = GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        if (carry) {
            hx.resize((size_t)cm * cN * cdim);
            hs.resize((size_t)cm);
            if (hipMemcpy(hx.data(), d_in, sizeof(float) * hx.size(), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(hs.data(), d_instat, hs.size(), hipMemcpyDeviceToHost) != hipSuccess)
                rc = GPIS_ERR_HIP;
        }
        for (void* p : {(void*)d_in, (void*)d_x, (void*)d_instat, (void*)d_fres, (void*)d_ires, (void*)d_arc, (void*)d_tv, (void*)d_tt,
                        (void*)d_lim, (void*)d_tsum, (void*)d_tint, (void*)d_cu, (void*)d_chp, (void*)d_cclamp, (void*)d_follow,
                        (void*)d_chkd, (void*)d_chki, (void*)d_bodyd, (void*)d_bodyi, (void*)d_bresd,
                        (void*)d_bresi, (void*)d_rres, (void*)d_rown, (void*)d_btd, (void*)d_bti, (void*)d_bst})
            (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_in = d_x = d_fres = d_arc = nullptr; d_instat = nullptr; d_ires = nullptr; own = nullptr;
    d_tv = d_tt = d_tsum = nullptr; d_lim = nullptr; d_tint = nullptr; d_cu = d_chp = d_follow = nullptr; d_cclamp = nullptr;
    d_chkd = nullptr; d_chki = nullptr; cap_chk = 0;
    d_bodyd = nullptr; d_bodyi = nullptr; cap_body = 0;
    d_bresd = nullptr; d_bresi = nullptr; cap_bres = 0;
    d_rres = nullptr; d_rown = nullptr; cap_rt = 0;
    d_btd = nullptr; d_bti = nullptr; cap_bt = 0; d_bst = nullptr; cap_bst = 0;
    cap_x = cap_m = cap_arc = cap_tn = cap_tm = cap_cu = cap_cm = 0;
    has_input = valid = timed = body_valid = retimed = false;
    m = N = dim = 0;
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    if (rc != GPIS_OK) return rc;
    if (carry) {
        if (int e = ensure(cm, cN, cdim)) return e;
        GPIS_HIP(hipMemcpy(d_in, hx.data(), sizeof(float) * hx.size(), hipMemcpyHostToDevice));
        GPIS_HIP(hipMemcpy(d_instat, hs.data(), hs.size(), hipMemcpyHostToDevice));
        m = cm; N = cN; dim = cdim;
        has_input = true;
    }
    return GPIS_OK;
}

int Trajectories::ensure(int mm, int NN, int dd) {
    const size_t nx = (size_t)mm * NN * dd;
    if (nx > cap_x) {
        (void)hipFree(d_in); (void)hipFree(d_x);
        d_in = d_x = nullptr; cap_x = 0;
        GPIS_HIP(hipMalloc((void**)&d_in, sizeof(float) * nx));
        GPIS_HIP(hipMalloc((void**)&d_x, sizeof(float) * nx));
        cap_x = nx;
    }
    if ((size_t)mm > cap_m) {
        for (void* p : {(void*)d_instat, (void*)d_fres, (void*)d_ires}) (void)hipFree(p);
        d_instat = nullptr; d_fres = nullptr; d_ires = nullptr; cap_m = 0;
        GPIS_HIP(hipMalloc((void**)&d_instat, (size_t)mm));
        GPIS_HIP(hipMalloc((void**)&d_fres, sizeof(float) * 4 * (size_t)mm));
        GPIS_HIP(hipMalloc((void**)&d_ires, sizeof(int) * 4 * (size_t)mm));
        cap_m = (size_t)mm;
    }
    return GPIS_OK;
}

int Trajectories::from_packed(int dev, long long npaths, long long npoints, int dd, const long long* off, const float* pts,
                              const unsigned char* pstat, int NN, bool zero_w) {
    has_input = valid = timed = body_valid = retimed = false;
    if (int rc = bind(dev)) return rc;
    const int mm = (int)npaths;
    if (int rc = ensure(mm, NN, dd)) return rc;
    if (int rc = grow(d_arc, cap_arc, (size_t)std::max(1ll, npoints))) return rc;
    hipLaunchKernelGGL(traj_arc_kernel, dim3(grid_for(mm, kBlock, kGridCapTraj)), dim3(kBlock), 0, own, off, pts, pstat, mm, dd, d_arc);
    GPIS_HIP(hipGetLastError());
    const dim3 grid(grid_for((long long)mm * NN, kBlock, kGridCapTraj));
    if (zero_w)
        hipLaunchKernelGGL(traj_resample_kernel<true>, grid, dim3(kBlock), 0, own, off, pts, pstat, d_arc, mm, NN, dd, d_in, d_instat);
    else
        hipLaunchKernelGGL(traj_resample_kernel<false>, grid, dim3(kBlock), 0, own, off, pts, pstat, d_arc, mm, NN, dd, d_in, d_instat);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(own));
    m = mm; N = NN; dim = dd;
    has_input = true;
    return GPIS_OK;
}

int Trajectories::from_paths(const Planner& p, int NN) {
    if (NN < kMinN || NN > kMaxN) return GPIS_ERR_ARG;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (p.npaths > kMaxTraj) return GPIS_ERR_LIMIT;
    return from_packed(p.device, p.npaths, p.npoints, p.dim, p.d_off, p.d_points, p.d_status, NN, false);
}

int Trajectories::from_pose_paths(const PosePlanner& p, int NN) {
    if (NN < kMinN || NN > kMaxN) return GPIS_ERR_ARG;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (p.npaths > kMaxTraj) return GPIS_ERR_LIMIT;
    return from_packed(p.device, p.npaths, p.npoints, 2, p.d_off, p.d_points, p.d_status, NN, true);
}

int Trajectories::set(const float* x, int mm, int NN, int dd) {
    if (!x || mm < 1 || NN < kMinN || NN > kMaxN || (dd != 2 && dd != 3)) return GPIS_ERR_ARG;
    if (mm > kMaxTraj) return GPIS_ERR_LIMIT;
    has_input = valid = timed = body_valid = retimed = false;
    if (int rc = ensure(mm, NN, dd)) return rc;
    const size_t per = (size_t)NN * dd;
    std::vector<unsigned char> st((size_t)mm, 0);
    for (int t = 0; t < mm; ++t)
        for (size_t k = 0; k < per; ++k)
            if (!std::isfinite(x[(size_t)t * per + k])) { st[t] = 2; break; }
    GPIS_HIP(hipMemcpyAsync(d_in, x, sizeof(float) * per * mm, hipMemcpyHostToDevice, own));
    GPIS_HIP(hipMemcpyAsync(d_instat, st.data(), (size_t)mm, hipMemcpyHostToDevice, own));
    GPIS_HIP(hipStreamSynchronize(own));
    m = mm; N = NN; dim = dd;
    has_input = true;
    return GPIS_OK;
}

int Trajectories::optimize(const DistanceField& df, const TrajOpts& o, hipStream_t s, const BodyArgs* bd, float w_turn) {
    if (int rc = traj_check_opts(o)) return rc;
    if (!df.valid || !has_input) return GPIS_ERR_STATE;
    if (df.dim != dim) return GPIS_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    valid = timed = body_valid = retimed = false;
    if (int rc = bind(df.device)) return rc;
    if (bd && (size_t)m > cap_bres) {
        (void)hipFree(d_bresd); (void)hipFree(d_bresi);
        d_bresd = nullptr; d_bresi = nullptr; cap_bres = 0;
        GPIS_HIP(hipMalloc((void**)&d_bresd, sizeof(double) * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_bresi, sizeof(int) * 3 * (size_t)m));
        cap_bres = (size_t)m;
    }
    const DfLattice L = df.lattice();
    const int threads = 64 * ((N + 63) / 64);
    const BodyArgs none{nullptr, 0};
#define GPIS_TRAJ_OPT(D, B, ARGS, WT, RD, RI)                                                                                        \
    hipLaunchKernelGGL((traj_opt_kernel<D, B>), dim3((unsigned)m), dim3(threads), 0, s, df.d_dist, L, d_in, d_instat, N, o, d_x, d_fres, \
                       d_ires, ARGS, WT, RD, RI)
    if (bd) {
        if (dim == 2) GPIS_TRAJ_OPT(2, true, *bd, w_turn, d_bresd, d_bresi);
        else GPIS_TRAJ_OPT(3, true, *bd, w_turn, d_bresd, d_bresi);
    } else {
        if (dim == 2) GPIS_TRAJ_OPT(2, false, none, 0.f, (double*)nullptr, (int*)nullptr);
        else GPIS_TRAJ_OPT(3, false, none, 0.f, (double*)nullptr, (int*)nullptr);
    }
#undef GPIS_TRAJ_OPT
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    opt_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    valid = true;
    body_valid = bd != nullptr;
    return GPIS_OK;
}

int Trajectories::body_result(double* D_min, int* waypoint, int* ball, int* collides) {
    if (!valid || !body_valid) return GPIS_ERR_STATE;
    std::vector<double> hd((size_t)m);
    std::vector<int> hi(3 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_bresd, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_bresi, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m; ++r) {
        if (D_min) D_min[r] = hd[r];
        if (waypoint) waypoint[r] = hi[3 * r];
        if (ball) ball[r] = hi[3 * r + 1];
        if (collides) collides[r] = hi[3 * r + 2];
    }
    return GPIS_OK;
}

// ---- time parametrisation and control sequences ---------------------------------------------------------------
int timing_check_opts(const TimingOpts& o) {
    for (float v : {o.v_max, o.v_min, o.a_max, o.d_max, o.a_lat, o.w_max, o.v_start, o.v_end, o.clearance, o.slow_dist})
        if (!std::isfinite(v)) return GPIS_ERR_ARG;
    if (!(o.v_max > 0.f) || !(o.v_min > 0.f && o.v_min <= o.v_max) || !(o.a_max > 0.f) || !(o.d_max > 0.f)) return GPIS_ERR_ARG;
    if (o.a_lat < 0.f || o.w_max < 0.f || o.v_start < 0.f || o.v_end < 0.f || o.slow_dist < 0.f) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int timing_check_args(double dt, int T, double t0, double w_limit, double min_move) {
    if (!std::isfinite(dt) || !std::isfinite(t0) || !std::isfinite(w_limit) || !std::isfinite(min_move)) return GPIS_ERR_ARG;
    if (!(dt > 0.0) || T < 1 || T > Trajectories::kMaxT || t0 < 0.0 || w_limit < 0.0 || min_move < 0.0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int Trajectories::time(const DistanceField* df, const TimingOpts& o, hipStream_t s) {
    if (int rc = timing_check_opts(o)) return rc;
    if (!valid) return GPIS_ERR_STATE;
    if (df) {
        if (!df->valid) return GPIS_ERR_STATE;
        if (df->dim != dim || df->device != device) return GPIS_ERR_ARG;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!s) s = df ? df->own : own;
    timed = retimed = false;
    // (the layout follows the current m and N; the capacities only ever say how much is allocated)
    const size_t mn = (size_t)m * N;
    if (mn > cap_tn) {
        for (void* p : {(void*)d_tv, (void*)d_tt, (void*)d_lim}) (void)hipFree(p);
        d_tv = d_tt = nullptr; d_lim = nullptr; cap_tn = 0;
        GPIS_HIP(hipMalloc((void**)&d_tv, sizeof(float) * mn));
        GPIS_HIP(hipMalloc((void**)&d_tt, sizeof(float) * mn));
        GPIS_HIP(hipMalloc((void**)&d_lim, mn));
        cap_tn = mn;
    }
    if ((size_t)m > cap_tm) {
        (void)hipFree(d_tsum); (void)hipFree(d_tint);
        d_tsum = nullptr; d_tint = nullptr; cap_tm = 0;
        GPIS_HIP(hipMalloc((void**)&d_tsum, sizeof(float) * 3 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_tint, sizeof(int) * 9 * (size_t)m));
        cap_tm = (size_t)m;
    }
    DfLattice L{};
    if (df) L = df->lattice();
    const float* F = df ? df->d_dist : nullptr;
    const int threads = 64 * ((N + 63) / 64);
    if (dim == 2)
        hipLaunchKernelGGL(traj_time_kernel<2>, dim3((unsigned)m), dim3(threads), 0, s, F, L, df ? 1 : 0, d_x, d_ires, N, o, d_tv, d_tt,
                           d_lim, d_tsum, d_tint);
    else
        hipLaunchKernelGGL(traj_time_kernel<3>, dim3((unsigned)m), dim3(threads), 0, s, F, L, df ? 1 : 0, d_x, d_ires, N, o, d_tv, d_tt,
                           d_lim, d_tsum, d_tint);
    GPIS_HIP(hipGetLastError());
    h_tint.resize(9 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(h_tint.data(), d_tint, sizeof(int) * 9 * (size_t)m, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    time_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    timed = true;
    return GPIS_OK;
}

int Trajectories::controls(double dt, int T, double t0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                           int* clamped) {
    if (int rc = timing_check_args(dt, T, t0, w_limit, min_move)) return rc;
    if (!has_timing()) return GPIS_ERR_STATE;
    const auto c0 = std::chrono::steady_clock::now();
    const int nu = dim == 3 ? 4 : 2;
    if (int rc = grow(d_cu, cap_cu, (size_t)m * T * nu)) return rc;
    if ((size_t)m > cap_cm) {
        (void)hipFree(d_chp); (void)hipFree(d_cclamp);
        d_chp = nullptr; d_cclamp = nullptr; cap_cm = 0;
        GPIS_HIP(hipMalloc((void**)&d_chp, sizeof(double) * 5 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_cclamp, sizeof(int) * (size_t)m));
        cap_cm = (size_t)m;
    }
    const int threads = 64 * ((T + 63) / 64);
    if (dim == 2)
        hipLaunchKernelGGL(traj_controls_kernel<2>, dim3((unsigned)m), dim3(threads), 0, own, d_x, d_tv, d_tt, d_tint, N, T, 0, dt, t0,
                           w_limit, min_move, d_cu, d_chp, d_cclamp);
    else
        hipLaunchKernelGGL(traj_controls_kernel<3>, dim3((unsigned)m), dim3(threads), 0, own, d_x, d_tv, d_tt, d_tint, N, T, 0, dt, t0,
                           w_limit, min_move, d_cu, d_chp, d_cclamp);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hp;
    if (U) GPIS_HIP(hipMemcpyAsync(U, d_cu, sizeof(double) * (size_t)m * T * nu, hipMemcpyDeviceToHost, own));
    if (heading0 || p0) {
        hp.resize(5 * (size_t)m);
        GPIS_HIP(hipMemcpyAsync(hp.data(), d_chp, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, own));
    }
    if (clamped) GPIS_HIP(hipMemcpyAsync(clamped, d_cclamp, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m && !hp.empty(); ++r) {
        if (heading0) { heading0[2 * r] = hp[5 * r]; heading0[2 * r + 1] = hp[5 * r + 1]; }
        if (p0) for (int a = 0; a < dim; ++a) p0[r * dim + a] = hp[5 * r + 2 + a];
    }
    controls_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    return GPIS_OK;
}

int Trajectories::follow(Controller& c, int index, double dt, double t0, double w_limit, double min_move, double* heading0,
                         double* p0) {
    if (!c.inited || !has_timing()) return GPIS_ERR_STATE;
    if (int rc = timing_check_args(dt, c.T, t0, w_limit, min_move)) return rc;
    if (c.dim != dim || c.device != device || index < 0 || index >= m) return GPIS_ERR_ARG;
    if (h_tint[9 * (size_t)index] != 0) return GPIS_ERR_STATE;
    if (!d_follow) GPIS_HIP(hipMalloc((void**)&d_follow, sizeof(double) * 8));
    // (the own stream's work is finished: time() synchronised; the controller's stream orders the write with its steps)
    const int threads = 64 * ((c.T + 63) / 64);
    int* d_cl = (int*)(d_follow + 6);
    if (dim == 2)
        hipLaunchKernelGGL(traj_controls_kernel<2>, dim3(1), dim3(threads), 0, c.own, d_x, d_tv, d_tt, d_tint, N, c.T, index, dt, t0,
                           w_limit, min_move, c.d_U[c.cur], d_follow, d_cl);
    else
        hipLaunchKernelGGL(traj_controls_kernel<3>, dim3(1), dim3(threads), 0, c.own, d_x, d_tv, d_tt, d_tint, N, c.T, index, dt, t0,
                           w_limit, min_move, c.d_U[c.cur], d_follow, d_cl);
    GPIS_HIP(hipGetLastError());
    double hp[5];
    GPIS_HIP(hipMemcpyAsync(hp, d_follow, sizeof(hp), hipMemcpyDeviceToHost, c.own));
    GPIS_HIP(hipStreamSynchronize(c.own));
    if (heading0) { heading0[0] = hp[0]; heading0[1] = hp[1]; }
    if (p0) for (int a = 0; a < dim; ++a) p0[a] = hp[2 + a];
    return GPIS_OK;
}

int Trajectories::check_obst(const Obstacles& ob, double dt, int steps, double t0, double t_begin, double clearance, double* min_sep,
                             double* min_time, int* min_obstacle, int* first_hit, int* collides) {
    if (!has_timing()) return GPIS_ERR_STATE;
    if ((size_t)m > cap_chk) {
        (void)hipFree(d_chkd); (void)hipFree(d_chki);
        d_chkd = nullptr; d_chki = nullptr; cap_chk = 0;
        GPIS_HIP(hipMalloc((void**)&d_chkd, sizeof(double) * 2 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_chki, sizeof(int) * 3 * (size_t)m));
        cap_chk = (size_t)m;
    }
    const double TB = t_begin - ob.epoch;
    if (dim == 2)
        hipLaunchKernelGGL(traj_obst_check_kernel<2>, dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, dt, t0, TB,
                           clearance, (const double*)ob.d_tab, ob.n, d_chkd, d_chki);
    else
        hipLaunchKernelGGL(traj_obst_check_kernel<3>, dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, dt, t0, TB,
                           clearance, (const double*)ob.d_tab, ob.n, d_chkd, d_chki);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hd(2 * (size_t)m);
    std::vector<int> hi(3 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_chkd, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_chki, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m; ++r) {
        if (min_sep) min_sep[r] = hd[2 * r];
        if (min_time) min_time[r] = hd[2 * r + 1];
        if (min_obstacle) min_obstacle[r] = hi[3 * r];
        if (first_hit) first_hit[r] = hi[3 * r + 1];
        if (collides) collides[r] = hi[3 * r + 2];
    }
    return GPIS_OK;
}

int Trajectories::check_body(const DistanceField& df, const BodyArgs& bd, double clearance, double* D_min, int* waypoint, int* ball,
                             int* collides) {
    if (!valid) return GPIS_ERR_STATE;
    if ((size_t)m > cap_body) {
        (void)hipFree(d_bodyd); (void)hipFree(d_bodyi);
        d_bodyd = nullptr; d_bodyi = nullptr; cap_body = 0;
        GPIS_HIP(hipMalloc((void**)&d_bodyd, sizeof(double) * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_bodyi, sizeof(int) * 3 * (size_t)m));
        cap_body = (size_t)m;
    }
    const DfLattice L = df.lattice();
    if (dim == 2)
        hipLaunchKernelGGL(traj_body_check_kernel<2>, dim3((unsigned)m), dim3(kBlock), 0, own, (const float*)df.d_dist, L, bd, (const float*)d_x,
                           (const int*)d_ires, N, clearance, d_bodyd, d_bodyi);
    else
        hipLaunchKernelGGL(traj_body_check_kernel<3>, dim3((unsigned)m), dim3(kBlock), 0, own, (const float*)df.d_dist, L, bd, (const float*)d_x,
                           (const int*)d_ires, N, clearance, d_bodyd, d_bodyi);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hd((size_t)m);
    std::vector<int> hi(3 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_bodyd, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_bodyi, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m; ++r) {
        if (D_min) D_min[r] = hd[r];
        if (waypoint) waypoint[r] = hi[3 * r];
        if (ball) ball[r] = hi[3 * r + 1];
        if (collides) collides[r] = hi[3 * r + 2];
    }
    return GPIS_OK;
}

// ---- re-timing ---------------------------------------------------------------------------------------------------
int retime_check_opts(const RetimeOpts& o) {
    if (!std::isfinite(o.slot) || !(o.slot > 0.0) || !std::isfinite(o.clearance) || o.clearance < 0.0) return GPIS_ERR_ARG;
    if (o.max_pause < 0 || o.max_pause > Trajectories::kMaxPause || (o.press_on != 0 && o.press_on != 1)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int Trajectories::retime(const Obstacles& ob, const RetimeOpts& o, double t_begin, hipStream_t s) {
    if (!has_timing()) return GPIS_ERR_STATE;
    const auto c0 = std::chrono::steady_clock::now();
    if (!s) s = own;
    retimed = false;
    if ((size_t)m > cap_rt) {
        (void)hipFree(d_rres); (void)hipFree(d_rown);
        d_rres = nullptr; d_rown = nullptr; cap_rt = 0;
        GPIS_HIP(hipMalloc((void**)&d_rres, sizeof(int) * kSchedRes * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_rown, sizeof(int) * kOwnLen * (size_t)m));
        cap_rt = (size_t)m;
    }
    const double TB = t_begin - ob.epoch;
    if (dim == 2)
        hipLaunchKernelGGL(traj_retime_kernel<2>, dim3((unsigned)m), dim3(kBlock), 0, s, d_x, d_tv, d_tt, d_tint, N, o.slot, o.max_pause,
                           o.clearance, o.press_on, TB, (const double*)ob.d_tab, ob.n, d_rres, d_rown);
    else
        hipLaunchKernelGGL(traj_retime_kernel<3>, dim3((unsigned)m), dim3(kBlock), 0, s, d_x, d_tv, d_tt, d_tint, N, o.slot, o.max_pause,
                           o.clearance, o.press_on, TB, (const double*)ob.d_tab, ob.n, d_rres, d_rown);
    GPIS_HIP(hipGetLastError());
    h_rres.resize(kSchedRes * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(h_rres.data(), d_rres, sizeof(int) * h_rres.size(), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    ropts = o;
    r_begin = t_begin;
    r_body = 0;
    retime_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    retimed = true;
    return GPIS_OK;
}

int Trajectories::retime_controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    if (!has_schedule()) return GPIS_ERR_STATE;
    const int nu = dim == 3 ? 4 : 2;
    if (int rc = grow(d_cu, cap_cu, (size_t)m * T * nu)) return rc;
    if ((size_t)m > cap_cm) {
        (void)hipFree(d_chp); (void)hipFree(d_cclamp);
        d_chp = nullptr; d_cclamp = nullptr; cap_cm = 0;
        GPIS_HIP(hipMalloc((void**)&d_chp, sizeof(double) * 5 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_cclamp, sizeof(int) * (size_t)m));
        cap_cm = (size_t)m;
    }
    const int threads = 64 * ((T + 63) / 64);
    const TrajSched sc{d_rres, d_rown, k0};
    if (dim == 2)
        hipLaunchKernelGGL(traj_retime_controls_kernel<2>, dim3((unsigned)m), dim3(threads), 0, own, d_x, d_tv, d_tt, d_tint, N, T, 0,
                           ropts.slot, w_limit, min_move, d_cu, d_chp, d_cclamp, sc);
    else
        hipLaunchKernelGGL(traj_retime_controls_kernel<3>, dim3((unsigned)m), dim3(threads), 0, own, d_x, d_tv, d_tt, d_tint, N, T, 0,
                           ropts.slot, w_limit, min_move, d_cu, d_chp, d_cclamp, sc);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hp;
    if (U) GPIS_HIP(hipMemcpyAsync(U, d_cu, sizeof(double) * (size_t)m * T * nu, hipMemcpyDeviceToHost, own));
    if (heading0 || p0) {
        hp.resize(5 * (size_t)m);
        GPIS_HIP(hipMemcpyAsync(hp.data(), d_chp, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, own));
    }
    if (clamped) GPIS_HIP(hipMemcpyAsync(clamped, d_cclamp, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m && !hp.empty(); ++r) {
        if (heading0) { heading0[2 * r] = hp[5 * r]; heading0[2 * r + 1] = hp[5 * r + 1]; }
        if (p0) for (int a = 0; a < dim; ++a) p0[r * dim + a] = hp[5 * r + 2 + a];
    }
    return GPIS_OK;
}

int Trajectories::retime_follow(Controller& c, int index, int k0, double w_limit, double min_move, double* heading0, double* p0) {
    if (!c.inited || !has_schedule()) return GPIS_ERR_STATE;
    if (int rc = timing_check_args(ropts.slot, c.T, 0.0, w_limit, min_move)) return rc;
    if (c.dim != dim || c.device != device || index < 0 || index >= m) return GPIS_ERR_ARG;
    if (h_tint[9 * (size_t)index] != 0 || h_rres[kSchedRes * (size_t)index] >= 2) return GPIS_ERR_STATE;
    if (!d_follow) GPIS_HIP(hipMalloc((void**)&d_follow, sizeof(double) * 8));
    // (the own stream's work is finished: retime() synchronised; the controller's stream orders the write with its steps)
    const int threads = 64 * ((c.T + 63) / 64);
    int* d_cl = (int*)(d_follow + 6);
    const TrajSched sc{d_rres, d_rown, k0};
    if (dim == 2)
        hipLaunchKernelGGL(traj_retime_controls_kernel<2>, dim3(1), dim3(threads), 0, c.own, d_x, d_tv, d_tt, d_tint, N, c.T, index,
                           ropts.slot, w_limit, min_move, c.d_U[c.cur], d_follow, d_cl, sc);
    else
        hipLaunchKernelGGL(traj_retime_controls_kernel<3>, dim3(1), dim3(threads), 0, c.own, d_x, d_tv, d_tt, d_tint, N, c.T, index,
                           ropts.slot, w_limit, min_move, c.d_U[c.cur], d_follow, d_cl, sc);
    GPIS_HIP(hipGetLastError());
    double hp[5];
    GPIS_HIP(hipMemcpyAsync(hp, d_follow, sizeof(hp), hipMemcpyDeviceToHost, c.own));
    GPIS_HIP(hipStreamSynchronize(c.own));
    if (heading0) { heading0[0] = hp[0]; heading0[1] = hp[1]; }
    if (p0) for (int a = 0; a < dim; ++a) p0[a] = hp[2 + a];
    return GPIS_OK;
}

int Trajectories::retime_check(const Obstacles& ob, int steps, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                               int* first_hit, int* collides) {
    if (!has_schedule()) return GPIS_ERR_STATE;
    if ((size_t)m > cap_chk) {
        (void)hipFree(d_chkd); (void)hipFree(d_chki);
        d_chkd = nullptr; d_chki = nullptr; cap_chk = 0;
        GPIS_HIP(hipMalloc((void**)&d_chkd, sizeof(double) * 2 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_chki, sizeof(int) * 3 * (size_t)m));
        cap_chk = (size_t)m;
    }
    const double TB = r_begin - ob.epoch;
    const TrajSched sc{d_rres, d_rown, 0};
    if (dim == 2)
        hipLaunchKernelGGL(traj_retime_check_kernel<2>, dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, ropts.slot,
                           TB, clearance, (const double*)ob.d_tab, ob.n, d_chkd, d_chki, sc);
    else
        hipLaunchKernelGGL(traj_retime_check_kernel<3>, dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, ropts.slot,
                           TB, clearance, (const double*)ob.d_tab, ob.n, d_chkd, d_chki, sc);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hd(2 * (size_t)m);
    std::vector<int> hi(3 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_chkd, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_chki, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m; ++r) {
        if (min_sep) min_sep[r] = hd[2 * r];
        if (min_time) min_time[r] = hd[2 * r + 1];
        if (min_obstacle) min_obstacle[r] = hi[3 * r];
        if (first_hit) first_hit[r] = hi[3 * r + 1];
        if (collides) collides[r] = hi[3 * r + 2];
    }
    return GPIS_OK;
}

// ---- the footprint against moving balls ---------------------------------------------------------------------------
int Trajectories::body_time_check(const Obstacles& ob, const BodyArgs& bd, bool sched, double dt, int steps, double t0, double TB,
                                  double clearance, double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit,
                                  int* collides) {
    if ((size_t)m > cap_bt) {
        (void)hipFree(d_btd); (void)hipFree(d_bti);
        d_btd = nullptr; d_bti = nullptr; cap_bt = 0;
        GPIS_HIP(hipMalloc((void**)&d_btd, sizeof(double) * 2 * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_bti, sizeof(int) * 4 * (size_t)m));
        cap_bt = (size_t)m;
    }
    const TrajSched sc{d_rres, d_rown, 0};
#define GPIS_BODY_CHECK(D, S)                                                                                                          \
    hipLaunchKernelGGL((traj_body_time_check_kernel<D, S>), dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, dt, \
                       t0, TB, clearance, (const double*)ob.d_tab, ob.n, bd, d_btd, d_bti, sc)
    if (dim == 2) { if (sched) GPIS_BODY_CHECK(2, 1); else GPIS_BODY_CHECK(2, 0); }
    else { if (sched) GPIS_BODY_CHECK(3, 1); else GPIS_BODY_CHECK(3, 0); }
#undef GPIS_BODY_CHECK
    GPIS_HIP(hipGetLastError());
    std::vector<double> hd(2 * (size_t)m);
    std::vector<int> hi(4 * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_btd, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_bti, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t r = 0; r < (size_t)m; ++r) {
        if (min_sep) min_sep[r] = hd[2 * r];
        if (min_time) min_time[r] = hd[2 * r + 1];
        if (min_obstacle) min_obstacle[r] = hi[4 * r];
        if (first_hit) first_hit[r] = hi[4 * r + 1];
        if (collides) collides[r] = hi[4 * r + 2];
        if (min_ball) min_ball[r] = hi[4 * r + 3];
    }
    return GPIS_OK;
}

int Trajectories::check_body_obst(const Obstacles& ob, const BodyArgs& bd, double dt, int steps, double t0, double t_begin,
                                  double clearance, double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit,
                                  int* collides) {
    if (!has_timing()) return GPIS_ERR_STATE;
    return body_time_check(ob, bd, false, dt, steps, t0, t_begin - ob.epoch, clearance, min_sep, min_time, min_obstacle, min_ball,
                           first_hit, collides);
}

int Trajectories::retime_body_check(const Obstacles& ob, const BodyArgs& bd, int steps, double clearance, double* min_sep,
                                    double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides) {
    if (!has_schedule()) return GPIS_ERR_STATE;
    return body_time_check(ob, bd, true, ropts.slot, steps, 0.0, r_begin - ob.epoch, clearance, min_sep, min_time, min_obstacle,
                           min_ball, first_hit, collides);
}

int Trajectories::retime_body(const Obstacles& ob, const BodyArgs& bd, const RetimeOpts& o, double t_begin, hipStream_t s) {
    if (!has_timing()) return GPIS_ERR_STATE;
    const auto c0 = std::chrono::steady_clock::now();
    if (!s) s = own;
    retimed = false;
    if ((size_t)m > cap_rt) {
        (void)hipFree(d_rres); (void)hipFree(d_rown);
        d_rres = nullptr; d_rown = nullptr; cap_rt = 0;
        GPIS_HIP(hipMalloc((void**)&d_rres, sizeof(int) * kSchedRes * (size_t)m));
        GPIS_HIP(hipMalloc((void**)&d_rown, sizeof(int) * kOwnLen * (size_t)m));
        cap_rt = (size_t)m;
    }
    const double TB = t_begin - ob.epoch;
    if (dim == 2)
        hipLaunchKernelGGL(traj_body_retime_kernel<2>, dim3((unsigned)m), dim3(kBlock), 0, s, d_x, d_tv, d_tt, d_tint, N, o.slot,
                           o.max_pause, o.clearance, o.press_on, TB, (const double*)ob.d_tab, ob.n, bd, d_rres, d_rown);
    else
        hipLaunchKernelGGL(traj_body_retime_kernel<3>, dim3((unsigned)m), dim3(kBlock), 0, s, d_x, d_tv, d_tt, d_tint, N, o.slot,
                           o.max_pause, o.clearance, o.press_on, TB, (const double*)ob.d_tab, ob.n, bd, d_rres, d_rown);
    GPIS_HIP(hipGetLastError());
    h_rres.resize(kSchedRes * (size_t)m);
    GPIS_HIP(hipMemcpyAsync(h_rres.data(), d_rres, sizeof(int) * h_rres.size(), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    ropts = o;
    r_begin = t_begin;
    r_body = bd.m;
    retime_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    retimed = true;
    return GPIS_OK;
}

int Trajectories::timed_states(double dt, int steps, double t0, bool sched, double* states) {
    if (sched ? !has_schedule() : !has_timing()) return GPIS_ERR_STATE;
    const size_t cnt = (size_t)m * (steps + 1) * (dim + 2);
    if (int rc = grow(d_bst, cap_bst, cnt)) return rc;
    const TrajSched sc{d_rres, d_rown, 0};
    if (sched) dt = ropts.slot;
#define GPIS_BODY_STATES(D, S)                                                                                                         \
    hipLaunchKernelGGL((traj_body_states_kernel<D, S>), dim3((unsigned)m), dim3(kBlock), 0, own, d_x, d_tv, d_tt, d_tint, N, steps, dt, t0, \
                       d_bst, sc)
    if (dim == 2) { if (sched) GPIS_BODY_STATES(2, 1); else GPIS_BODY_STATES(2, 0); }
    else { if (sched) GPIS_BODY_STATES(3, 1); else GPIS_BODY_STATES(3, 0); }
#undef GPIS_BODY_STATES
    GPIS_HIP(hipGetLastError());
    if (states) GPIS_HIP(hipMemcpyAsync(states, d_bst, sizeof(double) * cnt, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    return GPIS_OK;
}

}  // namespace gpis
