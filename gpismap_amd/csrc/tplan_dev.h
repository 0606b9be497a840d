// The device side of the layered planners, defined once for the time planner (tplan.hip) and the time-pose planner (tpplan.hip):
// world(), a lattice index as a world coordinate; broad_phase(), the cull of the moving balls against a workgroup's region and
// the mask of the kept ones; closest_approach() of two points that each move on a chord over one slot; check_begin() /
// check_finish(), the empty result and the block's winner rule of a check kernel; tplan_finish_kernel, the counts of slot 0; and
// tplan_controls_kernel, the control sequences along the paths (each including file gets its own copy of the two kernels).  The
// statistics words are TimePlanCore::kStat* (tplan_host.h).  The tiles, the move sets, the candidate logic, the radii a
// separation subtracts and the keys a check packs are the planners' own.  Double, left to right, nothing contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "tplan_host.h"
#include "plan_dev.h"
#include "block_ops.h"

namespace gpis {
namespace tplan_dev {

using namespace plan_dev;

constexpr int kBlock = 256;              // the block of every kernel but the time planner's layer kernel

__device__ __forceinline__ double world(float o, int i, float step) { return (double)(o + (float)i * step); }

// The broad phase of a layer kernel: thread i decides whether ball i < n can come within reach of the region [rx0, rx1] x [ry0,
// ry1] of world points between the elapsed times e_lo and e_hi: the region's box against the box of the ball's centre at the two
// ends.  reach(row) is the caller's threshold for the ball of that row (read only where the ball exists; a lambda that captures
// by value: a reference to a kernel's by-value argument changed the tile load before it, profiles/tplan_shared_core.md); a ball
// whose ends are not finite is kept.  The kept balls' bits go to s_keep[Obstacles::kMax / 32]; after the barrier (which also publishes what the
// caller stored to LDS before) thread 0 adds the skipped balls to stat[kStatSkipped].  For blocks of at least Obstacles::kMax
// threads.
template <class Reach>
__device__ __forceinline__ void broad_phase(const double* __restrict__ tab, int n, int cull, double e_lo, double e_hi, double rx0, double rx1,
                                            double ry0, double ry1, Reach reach, unsigned* s_keep, unsigned long long* __restrict__ stat) {
    const int tid = threadIdx.x;
    bool keep = tid < n;
    if (keep && cull) {
        const double* row = tab + (size_t)tid * Obstacles::kRow;
        const double ax = row[0] + row[3] * e_lo, bx = row[0] + row[3] * e_hi;
        const double ay = row[1] + row[4] * e_lo, by = row[1] + row[4] * e_hi;
        if (isfinite(ax) && isfinite(bx) && isfinite(ay) && isfinite(by)) {
            const double gx = fmax(0.0, fmax(rx0 - fmax(ax, bx), fmin(ax, bx) - rx1));
            const double gy = fmax(0.0, fmax(ry0 - fmax(ay, by), fmin(ay, by) - ry1));
            if (sqrt(gx * gx + gy * gy) > reach(row)) keep = false;
        }
    }
    const unsigned long long b = __ballot(keep);
    if ((tid & 63) == 0 && tid < Obstacles::kMax) { s_keep[tid >> 5] = (unsigned)b; s_keep[(tid >> 5) + 1] = (unsigned)(b >> 32); }
    __syncthreads();
    if (tid == 0 && cull && n > 0) {
        int k = 0;
        for (int w = 0; w < Obstacles::kMax / 32; ++w) k += __popc(s_keep[w]);
        if (n - k > 0) atomicAdd(&stat[TimePlanCore::kStatSkipped], (unsigned long long)(n - k));
    }
}

// The closest approach of two points that each move on a chord over one slot: A = their offset at the slot's start, A + B at its
// end.  Returns the least distance and in t where in the slot, [0, 1], it is reached (0 where the offset does not change).
__device__ __forceinline__ double closest_approach(double Ax, double Ay, double Bx, double By, double& t) {
    const double bb = Bx * Bx + By * By, ab = Ax * Bx + Ay * By;
    t = 0.0;
    if (bb > 0.0) {
        t = (-ab) / bb;
        t = t > 0.0 ? t : 0.0;
        t = t < 1.0 ? t : 1.0;
    }
    const double qx = Ax + t * Bx, qy = Ay + t * By;
    const double s2 = qx * qx + qy * qy;
    return sqrt(s2);
}

// A check kernel's opening, one workgroup per path: o = the path's first point, A = its intervals.  False where there is
// nothing to check (no path, no balls, a path of one point): thread 0 has written the empty result and the workgroup leaves.
// out_d[tr][2] = min_sep, min_time; out_i[tr][4] = min_obstacle, first_hit, collides, min_ball.
__device__ __forceinline__ bool check_begin(const long long* __restrict__ off, const unsigned char* __restrict__ status, int n, long long& o,
                                            int& A, double* __restrict__ out_d, int* __restrict__ out_i) {
    const int tr = blockIdx.x;
    o = off[tr];
    A = (int)(off[tr + 1] - o) - 1;
    if (status[tr] == 0 && n != 0 && A > 0) return true;
    if (threadIdx.x == 0) {
        out_d[(size_t)tr * 2] = status[tr] == 0 ? (double)INFINITY : (double)NAN; out_d[(size_t)tr * 2 + 1] = (double)NAN;
        out_i[(size_t)tr * 4] = -1; out_i[(size_t)tr * 4 + 1] = -1; out_i[(size_t)tr * 4 + 2] = 0; out_i[(size_t)tr * 4 + 3] = -1;
    }
    return false;
}

// A check kernel's close, for blocks of kBlock threads.  Each thread brings its own least separation `best`, the key of where it
// found it (~0: nowhere; the keys order as (interval, ball ...) do) and the first interval `hit` below the clearance (0x7fffffff:
// none).  The block takes the least separation, then the least key among the threads that hold it.  Thread 0 writes first_hit
// and collides, and the result of a path none of whose separations was a number.  True in the one thread that holds the
// winner: it writes min_sep, min_time and the indices of its key.
__device__ __forceinline__ bool check_finish(double best, unsigned long long key, int hit, double* __restrict__ out_d, int* __restrict__ out_i) {
    __shared__ double shd[kBlock / 64];
    __shared__ unsigned long long shk[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const double bmin = block_reduce(best, OpMin(), shd, kBlock, (double)INFINITY);
    if (tid == 0) shd[0] = bmin;
    __syncthreads();
    const double least = shd[0];
    if (!(best == least)) key = ~0ull;
    const unsigned long long kmin = block_reduce(key, OpMin(), shk, kBlock, ~0ull);
    if (tid == 0) shk[0] = kmin;
    __syncthreads();
    const unsigned long long win = shk[0];
    const int fh = block_reduce(hit, OpMin(), shi, kBlock, 0x7fffffff);
    if (tid == 0) {
        out_i[(size_t)tr * 4 + 1] = fh == 0x7fffffff ? -1 : fh;
        out_i[(size_t)tr * 4 + 2] = fh == 0x7fffffff ? 0 : 1;
        if (win == ~0ull) {                              // no separation was a number
            out_d[(size_t)tr * 2] = (double)INFINITY; out_d[(size_t)tr * 2 + 1] = (double)NAN;
            out_i[(size_t)tr * 4] = -1; out_i[(size_t)tr * 4 + 3] = -1;
        }
    }
    return key == win && win != ~0ull;
}

// cost0 = the last layer; counts of free states and of states with a finite cost at slot 0, the largest such cost
static __global__ void __launch_bounds__(kBlock) tplan_finish_kernel(const float* __restrict__ c, const float* __restrict__ lay, long long ns,
                                                                     float* __restrict__ cost0, unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_cnt[3];
    counts_begin(s_cnt);
    unsigned nf = 0, nr = 0, mx = 0;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < ns; p += (long long)gridDim.x * blockDim.x) {
        const float v = lay[p];
        cost0[p] = v;
        if (c[p] > 0.f) {
            ++nf;
            if (v < INFINITY) { ++nr; mx = max(mx, __float_as_uint(v)); }
        }
    }
    commit_counts(s_cnt, nf, nr, mx, stat + TimePlanCore::kStatFree);
}

// Control sequences along the paths: the second stage of the timing's controls (§7p) on the path's own points, the position of
// step k being the point of slot min(k0 + k, arrive): a wait repeats its point, and so does a turn.  One workgroup per path,
// blockDim.x = 64 ceil(T / 64), thread k = step k; a start is `width` floats.  U[tr][T][2], hp[tr][4] = heading0, p_0,
// clamped[tr].
static __global__ void __launch_bounds__(kBlock) tplan_controls_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ status,
                                                                       const float* __restrict__ pts, const float* __restrict__ starts,
                                                                       int width, int T, int k0, double dt, double w_limit, double min_move,
                                                                       double* __restrict__ U, double* __restrict__ hp,
                                                                       int* __restrict__ clamped) {
    __shared__ double sh[2][kBlock];
    __shared__ int swi[2 * (kBlock / 64)];
    __shared__ int sidx[kBlock];
    const int tr = blockIdx.x, k = threadIdx.x, nthr = blockDim.x;
    double* Uo = U + (size_t)tr * T * 2;
    double* hpo = hp + (size_t)tr * 4;
    if (status[tr] != 0) {                               // no path: stand still at the start as given
        if (k < T) { Uo[(size_t)k * 2] = 0.0; Uo[(size_t)k * 2 + 1] = 0.0; }
        if (k == 0) {
            hpo[0] = 1.0; hpo[1] = 0.0;
            hpo[2] = (double)starts[(size_t)tr * width]; hpo[3] = (double)starts[(size_t)tr * width + 1];
            clamped[tr] = 0;
        }
        return;
    }
    const long long o = off[tr];
    const int A = (int)(off[tr + 1] - o) - 1;
    double p[2] = {0.0, 0.0}, D[2] = {0.0, 0.0};
    double n = 0.0;
    bool mov = false;
    if (k < T) {
        const int ia = min(k0 + k, A), ib = min(k0 + k + 1, A);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            p[a] = (double)pts[(size_t)(o + ia) * 2 + a];
            D[a] = (double)pts[(size_t)(o + ib) * 2 + a] - p[a];
        }
        n = sqrt(D[0] * D[0] + D[1] * D[1]);
        mov = n > min_move;
    }
    if (mov) { sh[0][k] = D[0] / n; sh[1][k] = D[1] / n; }
    int fst;
    int last = block_latest_flag(mov, swi, nthr, &fst);  // (its barriers publish sh)
    if (last < 0) last = fst;
    sidx[k] = last;
    __syncthreads();
    int cl = 0;
    if (k < T) {
        const int nxt = k + 1 < T ? sidx[k + 1] : last;  // h_T = h_{T-1}
        double c = 1.0, s = 0.0, c1 = 1.0, s1 = 0.0;
        if (last >= 0) { c = sh[0][last]; s = sh[1][last]; }
        if (nxt >= 0) { c1 = sh[0][nxt]; s1 = sh[1][nxt]; }
        double* u = Uo + (size_t)k * 2;
        u[0] = (c * D[0] + s * D[1]) / dt;
        const double num = c * s1 - s * c1, den = 1.0 + (c * c1 + s * s1);
        double w;
        if (den <= 0.0) {
            w = w_limit > 0.0 ? (num >= 0.0 ? w_limit : -w_limit) : 0.0;
            cl = 1;
        } else {
            w = (num / den) / (0.5 * dt);
            if (w_limit > 0.0 && w > w_limit) { w = w_limit; cl = 1; }
            else if (w_limit > 0.0 && w < -w_limit) { w = -w_limit; cl = 1; }
        }
        u[1] = w;
        if (k == 0) { hpo[0] = c; hpo[1] = s; hpo[2] = p[0]; hpo[3] = p[1]; }
    }
    const int total = block_reduce(cl, OpAdd(), swi, nthr, 0);
    if (k == 0) clamped[tr] = total;
}

}  // namespace tplan_dev
}  // namespace gpis
