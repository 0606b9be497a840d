// Planning through space and time around moving balls (tplan.h; the contract: tests/tplan_ref.py).
//
// Lattice point (i, j): index p = j nx + i, world point P = (double)(o + (float)i * s) per axis.  State (p, s): index s np + p.
// Move slot m = 0 .. 8 of the offset (dx, dy) = (m % 3 - 1, m / 3 - 1): the planner's code 9 + m, and m = 4 is the wait (code 27).
//
// Layer kernel: one workgroup of 1024 threads per tile of 32 x 32 points advances L layers in one launch.  It loads c and the
// cost of layer s_hi on the tile and a ghost zone of L points into LDS, then computes layer s_hi - 1 on the region one ring
// smaller, layer s_hi - 2 on the next smaller one, ... and layer s_hi - L on the tile alone; two LDS cost buffers take turns.  A
// point of a ring is computed by every tile whose ghost zone holds it, from the same operands by the same operations, and only
// the tile that owns it stores its policy byte (and its cost, with keep_cost), so the bits do not depend on L.  Global cost
// layers take turns too: a launch reads one and writes the other, so no workgroup reads what another writes.
//
// Broad phase (cull): before the layers, thread i decides whether ball i can come within dyn_clearance of any move of this
// (tile, batch): the region's box against the box of the ball's centre over the batch's time span (§7y has the proof).  The
// kept balls are a 256-bit mask in LDS; the loop over them is the same in every lane, so a row of the table comes through scalar
// loads.  A skipped ball is work left out, not an early-out inside the expression.
#include <chrono>
#include <cmath>
#include <vector>
#include "tplan.h"
#include "dfield.h"
#include "plan_host.h"
#include "block_ops.h"

namespace gpis {

namespace {

using namespace plan_dev;

constexpr int kBlock = 256;
constexpr int kLayerBlock = 1024;        // the layer kernel: one thread per tile point, so that a point's chain over the balls is short
constexpr int kT = TimePlanner::kTile;
enum { kTStatKept = 0, kTStatSkipped, kTStatFree, kTStatFinite, kTStatMax, kTStatWords };

struct TLat {
    int nx, ny;
    float ox, oy, step;
};

__device__ __forceinline__ double world(float o, int i, float step) { return (double)(o + (float)i * step); }

// c[p] = point cost (0: not free), the top layer's cost +inf and policy 255
__global__ void __launch_bounds__(kBlock) tplan_setup_kernel(const float* __restrict__ dist, int np, float clearance, float margin, float gain,
                                                             float* __restrict__ c, float* __restrict__ top, unsigned char* __restrict__ pol_top) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < np; p += gridDim.x * blockDim.x) {
        c[p] = point_cost(dist[p], clearance, margin, gain);
        top[p] = INFINITY;
        pol_top[p] = 255;
    }
}

// the kept goals: cost 0 and policy 13 in the top layer (idempotent: duplicates write the same bits)
__global__ void __launch_bounds__(kBlock) tplan_goal_kernel(PlanLat L, const float* __restrict__ goals, int ngoals, const float* __restrict__ c,
                                                            float* __restrict__ top, unsigned char* __restrict__ pol_top,
                                                            unsigned long long* __restrict__ stat) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngoals; g += gridDim.x * blockDim.x) {
        int q[3];
        if (!snap(L, goals + (size_t)g * 2, q)) continue;
        const int p = q[1] * L.nx + q[0];
        if (!(c[p] > 0.f)) continue;
        top[p] = 0.f;
        pol_top[p] = 13;
        atomicAdd(&stat[kTStatKept], 1ull);
    }
}

// Layers s_hi - 1 .. s_hi - Lb from layer s_hi (hin) into hout (layer s_hi - Lb); dynamic LDS: 3 W W floats, W = 32 + 2 Lb.
// A goal is known by its cost 0 in the layer above: every translation weighs at least `step` > 0, and a wait of weight 0 keeps
// a cost that was 0 only at a goal, so by induction from the top layer no other point ever has cost 0.
__global__ void __launch_bounds__(kLayerBlock) tplan_layer_kernel(TLat G, int tnx, const float* __restrict__ c, const float* __restrict__ hin,
                                                             float* __restrict__ hout, unsigned char* __restrict__ policy,
                                                             float* __restrict__ cost_all, int s_hi, int Lb, int conn, float wwait,
                                                             double slot, double TB, double clr, const double* __restrict__ tab, int n,
                                                             int cull, unsigned long long* __restrict__ stat) {
    extern __shared__ float lds[];
    __shared__ unsigned s_keep[Obstacles::kMax / 32];
    const int W = kT + 2 * Lb, NW = W * W;
    float* s_c = lds;
    float* s_h0 = lds + NW;
    float* s_h1 = s_h0 + NW;
    const int tid = threadIdx.x, ti = blockIdx.x % tnx, tj = blockIdx.x / tnx;
    const int gi0 = ti * kT - Lb, gj0 = tj * kT - Lb;
    const size_t np = (size_t)G.nx * G.ny;
    for (int h = tid; h < NW; h += kLayerBlock) {
        const int gi = gi0 + h % W, gj = gj0 + h / W;
        const bool in = gi >= 0 && gi < G.nx && gj >= 0 && gj < G.ny;
        const int p = in ? gj * G.nx + gi : 0;
        s_c[h] = in ? c[p] : 0.f;
        s_h0[h] = in ? hin[p] : INFINITY;
    }
    {   // the broad phase: thread i decides for ball i
        bool keep = tid < n;
        if (keep && cull) {
            const double* row = tab + (size_t)tid * Obstacles::kRow;
            const double e_lo = TB + (double)(s_hi - Lb) * slot, e_hi = TB + (double)s_hi * slot;
            const double ax = row[0] + row[3] * e_lo, bx = row[0] + row[3] * e_hi;
            const double ay = row[1] + row[4] * e_lo, by = row[1] + row[4] * e_hi;
            if (isfinite(ax) && isfinite(bx) && isfinite(ay) && isfinite(by)) {
                const double rx0 = world(G.ox, gi0, G.step), rx1 = world(G.ox, gi0 + W - 1, G.step);
                const double ry0 = world(G.oy, gj0, G.step), ry1 = world(G.oy, gj0 + W - 1, G.step);
                const double gx = fmax(0.0, fmax(rx0 - fmax(ax, bx), fmin(ax, bx) - rx1));
                const double gy = fmax(0.0, fmax(ry0 - fmax(ay, by), fmin(ay, by) - ry1));
                // (the proof needs > r + clr; two lattice steps more are the margin)
                if (sqrt(gx * gx + gy * gy) > (row[6] + clr) + 2.0 * (double)G.step) keep = false;
            }
        }
        const unsigned long long b = __ballot(keep);
        if ((tid & 63) == 0 && tid < Obstacles::kMax) { s_keep[tid >> 5] = (unsigned)b; s_keep[(tid >> 5) + 1] = (unsigned)(b >> 32); }
    }
    __syncthreads();
    if (tid == 0 && cull && n > 0) {
        int k = 0;
        for (int w = 0; w < Obstacles::kMax / 32; ++w) k += __popc(s_keep[w]);
        if (n - k > 0) atomicAdd(&stat[kTStatSkipped], (unsigned long long)(n - k));
    }

    const float ls1 = G.step, ls2 = sqrtf(2.f) * G.step;
    for (int l = 0; l < Lb; ++l) {
        const int s = s_hi - 1 - l, r = l + 1, Wv = W - 2 * r;
        const float* src = (l & 1) ? s_h1 : s_h0;
        float* dst = (l & 1) ? s_h0 : s_h1;
        const double e0 = TB + (double)s * slot, e1 = TB + (double)(s + 1) * slot;
        const bool last = l == Lb - 1;
        for (int idx = tid; idx < Wv * Wv; idx += kLayerBlock) {
            const int li = r + idx % Wv, lj = r + idx / Wv, hh = lj * W + li;
            const int gi = gi0 + li, gj = gj0 + lj;
            const float cp = s_c[hh];
            float hv = INFINITY;
            unsigned char pol = 255;
            if (cp > 0.f) {
                if (src[hh] == 0.f) { hv = 0.f; pol = 13; }
                else {
                    float cn[9], hq[9];
#pragma unroll
                    for (int m = 0; m < 9; ++m) {
                        const int q = hh + (m / 3 - 1) * W + (m % 3 - 1);
                        cn[m] = s_c[q];
                        hq[m] = src[q];
                    }
                    unsigned cand = 0;
#pragma unroll
                    for (int m = 0; m < 9; ++m) {
                        const int dx = m % 3 - 1, dy = m / 3 - 1;
                        bool ex = cn[m] > 0.f;
                        if (dx != 0 && dy != 0) ex = ex && conn && cn[4 + dx] > 0.f && cn[4 + 3 * dy] > 0.f;
                        if (ex && hq[m] < INFINITY) cand |= 1u << m;
                    }
                    if (cand && n > 0) {
                        const double Px = world(G.ox, gi, G.step), Py = world(G.oy, gj, G.step);
                        const double dpx[3] = {world(G.ox, gi - 1, G.step) - Px, 0.0, world(G.ox, gi + 1, G.step) - Px};
                        const double dpy[3] = {world(G.oy, gj - 1, G.step) - Py, 0.0, world(G.oy, gj + 1, G.step) - Py};
                        unsigned blocked = 0;
                        for (int w = 0; w < Obstacles::kMax / 32; ++w) {
                            unsigned mk = __builtin_amdgcn_readfirstlane(s_keep[w]);
                            while (mk) {
                                const int i = w * 32 + (__ffs(mk) - 1);
                                mk &= mk - 1;
                                const double* __restrict__ row = tab + (size_t)i * Obstacles::kRow;
                                const double o0x = row[0] + row[3] * e0, o1x = row[0] + row[3] * e1;
                                const double o0y = row[1] + row[4] * e0, o1y = row[1] + row[4] * e1;
                                const double Ax = Px - o0x, Ay = Py - o0y, dox = o1x - o0x, doy = o1y - o0y, rad = row[6];
#pragma unroll
                                for (int m = 0; m < 9; ++m) {
                                    if ((cand >> m) & 1u) {
                                        const double Bx = dpx[m % 3] - dox, By = dpy[m / 3] - doy;
                                        const double bb = Bx * Bx + By * By, ab = Ax * Bx + Ay * By;
                                        double t = 0.0;
                                        if (bb > 0.0) {
                                            t = (-ab) / bb;
                                            t = t > 0.0 ? t : 0.0;
                                            t = t < 1.0 ? t : 1.0;
                                        }
                                        const double qx = Ax + t * Bx, qy = Ay + t * By;
                                        const double s2 = qx * qx + qy * qy;
                                        const double sep = sqrt(s2) - rad;
                                        if (sep < clr) blocked |= 1u << m;       // (a NaN separation is not below the clearance)
                                    }
                                }
                            }
                        }
                        cand &= ~blocked;
                    }
                    float best = INFINITY, bestq = INFINITY;
#pragma unroll
                    for (int m = 0; m < 9; ++m) {
                        if (m == 4) continue;
                        if ((cand >> m) & 1u) {
                            const float len = (m % 3 != 1 && m / 3 != 1) ? ls2 : ls1;
                            better_move(hq[m] + len * (0.5f * (cp + cn[m])), hq[m], 9 + m, best, bestq, pol);
                        }
                    }
                    if ((cand >> 4) & 1u) better_move(hq[4] + wwait * cp, hq[4], 27, best, bestq, pol);
                    hv = best;
                }
            }
            dst[hh] = hv;
            if (li >= Lb && li < Lb + kT && lj >= Lb && lj < Lb + kT && gi < G.nx && gj < G.ny) {    // (gi, gj >= 0 inside the tile)
                const size_t p = (size_t)gj * G.nx + gi;
                policy[(size_t)s * np + p] = pol;
                if (cost_all) cost_all[(size_t)s * np + p] = hv;
                if (last) hout[p] = hv;
            }
        }
        __syncthreads();
    }
}

// cost0 = the last layer; counts of free points and of points with a finite cost at slot 0, the largest such cost
__global__ void __launch_bounds__(kBlock) tplan_finish_kernel(const float* __restrict__ c, const float* __restrict__ lay, int np,
                                                              float* __restrict__ cost0, unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_cnt[3];
    counts_begin(s_cnt);
    unsigned nf = 0, nr = 0, mx = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < np; p += gridDim.x * blockDim.x) {
        const float v = lay[p];
        cost0[p] = v;
        if (c[p] > 0.f) {
            ++nf;
            if (v < INFINITY) { ++nr; mx = max(mx, __float_as_uint(v)); }
        }
    }
    commit_counts(s_cnt, nf, nr, mx, stat + kTStatFree);
}

// One thread per start follows the policy from slot 0.  WRITE = false: off[t] = points of the path (arrive + 1; 0 without a
// path), status, start cost.  WRITE = true: the same walk again, one point per slot stored from off[t] on.
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) tplan_walk_kernel(PlanLat L, int S, const float* __restrict__ c, const float* __restrict__ cost0,
                                                            const unsigned char* __restrict__ policy, const float* __restrict__ starts, int m,
                                                            long long* __restrict__ off, float* __restrict__ scost,
                                                            unsigned char* __restrict__ status, float* __restrict__ points) {
    const size_t np = (size_t)L.nx * L.ny;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        int q[3];
        long long cnt = 0;
        unsigned char st = 0;
        float sc = NAN;
        if (!snap(L, starts + (size_t)t * 2, q)) st = 1;
        else {
            int p = q[1] * L.nx + q[0];
            sc = cost0[p];
            if (!(c[p] > 0.f)) st = 2;
            else if (!(sc < INFINITY)) st = 3;
            else {
                float* out = WRITE ? points + (size_t)off[t] * 2 : nullptr;
                for (int s = 0;; ++s) {
                    if (WRITE) {
                        out[(size_t)cnt * 2] = L.ox + (float)q[0] * L.step;
                        out[(size_t)cnt * 2 + 1] = L.oy + (float)q[1] * L.step;
                    }
                    ++cnt;
                    const int k = policy[(size_t)s * np + p];
                    if (k == 13) break;
                    if (s >= S || !(k == 27 || (k >= 9 && k <= 17))) { st = 4; break; }     // (cannot happen on a finished plan)
                    if (k != 27) {
                        const int qi = q[0] + off_dx(k), qj = q[1] + off_dy(k);
                        if (qi < 0 || qi >= L.nx || qj < 0 || qj >= L.ny) { st = 4; break; }
                        q[0] = qi; q[1] = qj; p = qj * L.nx + qi;
                    }
                }
            }
        }
        if (!WRITE) { off[t] = cnt; scost[t] = sc; status[t] = st; }
    }
}

// A path against a set of moving balls: traj_obst_check_kernel's rule (traj.hip, §7q) on the path's own points, one per slot.
// One workgroup per path; a thread per interval loops over the table (scalar loads) and keeps its own least (sep, s, i) by a
// strict comparison in ascending order; the block takes the least sep, then the least key among the threads that hold it.
// out_d[tr][2] = min_sep, min_time; out_i[tr][3] = min_obstacle, first_hit, collides.
__global__ void __launch_bounds__(kBlock) tplan_check_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ status,
                                                             const float* __restrict__ pts, double dt, double TB, double clearance,
                                                             const double* __restrict__ tab, int n, double* __restrict__ out_d,
                                                             int* __restrict__ out_i) {
    __shared__ double shd[kBlock / 64];
    __shared__ unsigned long long shk[kBlock / 64];
    __shared__ int shi[kBlock / 64];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const long long o = off[tr];
    const int A = (int)(off[tr + 1] - o) - 1;
    if (status[tr] != 0 || n == 0 || A <= 0) {
        if (tid == 0) {
            out_d[(size_t)tr * 2] = status[tr] == 0 ? (double)INFINITY : (double)NAN; out_d[(size_t)tr * 2 + 1] = (double)NAN;
            out_i[(size_t)tr * 3] = -1; out_i[(size_t)tr * 3 + 1] = -1; out_i[(size_t)tr * 3 + 2] = 0;
        }
        return;
    }
    double best = INFINITY, best_s = 0.0;
    int best_k = -1, best_i = -1, hit = 0x7fffffff;
    for (int k = tid; k < A; k += kBlock) {
        const double e0 = TB + (double)k * dt, e1 = TB + (double)(k + 1) * dt;
        double p0[2], dp[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            p0[a] = (double)pts[(size_t)(o + k) * 2 + a];
            dp[a] = (double)pts[(size_t)(o + k + 1) * 2 + a] - p0[a];
        }
        const double* __restrict__ row = tab;
        for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
            double Aa[2], B[2], bb = 0.0, ab = 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const double o0 = row[a] + row[3 + a] * e0, o1 = row[a] + row[3 + a] * e1;
                Aa[a] = p0[a] - o0;
                B[a] = dp[a] - (o1 - o0);
                bb = a ? bb + B[a] * B[a] : B[a] * B[a];
                ab = a ? ab + Aa[a] * B[a] : Aa[a] * B[a];
            }
            double s = 0.0;
            if (bb > 0.0) {
                s = (-ab) / bb;
                s = s > 0.0 ? s : 0.0;
                s = s < 1.0 ? s : 1.0;
            }
            double s2 = 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const double q = Aa[a] + s * B[a];
                s2 = a ? s2 + q * q : q * q;
            }
            const double sep = sqrt(s2) - row[6];
            if (sep < best) { best = sep; best_s = s; best_k = k; best_i = i; }
            if (sep < clearance && k < hit) hit = k;
        }
    }
    const double bmin = block_reduce(best, OpMin(), shd, kBlock, (double)INFINITY);
    if (tid == 0) shd[0] = bmin;
    __syncthreads();
    const double least = shd[0];
    unsigned long long key = best_k >= 0 && best == least ? ((unsigned long long)best_k << 8) | (unsigned long long)best_i : ~0ull;
    const unsigned long long kmin = block_reduce(key, OpMin(), shk, kBlock, ~0ull);
    if (tid == 0) shk[0] = kmin;
    __syncthreads();
    const unsigned long long win = shk[0];
    const int fh = block_reduce(hit, OpMin(), shi, kBlock, 0x7fffffff);
    if (tid == 0) {
        out_i[(size_t)tr * 3 + 1] = fh == 0x7fffffff ? -1 : fh;
        out_i[(size_t)tr * 3 + 2] = fh == 0x7fffffff ? 0 : 1;
        if (win == ~0ull) {                              // no separation was a number
            out_d[(size_t)tr * 2] = (double)INFINITY; out_d[(size_t)tr * 2 + 1] = (double)NAN; out_i[(size_t)tr * 3] = -1;
        }
    }
    if (key == win && win != ~0ull) {
        out_d[(size_t)tr * 2] = best;
        out_d[(size_t)tr * 2 + 1] = (double)best_k * dt + best_s * dt;
        out_i[(size_t)tr * 3] = best_i;
    }
}

// Control sequences along the paths: the second stage of the timing's controls (§7p) restated on the path's own points, the
// position of step k being the point of slot min(k0 + k, arrive).  One workgroup per path, blockDim.x = 64 ceil(T / 64), thread
// k = step k.  U[tr][T][2], hp[tr][4] = heading0, p_0, clamped[tr].  Double, nothing contracted.
__global__ void __launch_bounds__(kBlock) tplan_controls_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ status,
                                                                const float* __restrict__ pts, const float* __restrict__ starts, int T,
                                                                int k0, double dt, double w_limit, double min_move,
                                                                double* __restrict__ U, double* __restrict__ hp, int* __restrict__ clamped) {
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
            hpo[2] = (double)starts[(size_t)tr * 2]; hpo[3] = (double)starts[(size_t)tr * 2 + 1];
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

}  // namespace

int tplan_check_opts(const TimePlanOpts& o) {
    if (!std::isfinite(o.clearance) || !(std::isfinite(o.margin) && o.margin >= 0.f) || !(std::isfinite(o.gain) && o.gain >= 0.f))
        return GPIS_ERR_ARG;
    if (o.gain > 1e4f || (o.connectivity != 0 && o.connectivity != 1)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.slot) && o.slot > 0.0) || !(std::isfinite(o.dyn_clearance) && o.dyn_clearance >= 0.0)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.wait) && o.wait >= 0.f && o.wait <= TimePlanner::kMaxWait)) return GPIS_ERR_ARG;
    if (o.horizon < 1 || o.horizon > TimePlanner::kMaxHorizon || (o.keep_cost != 0 && o.keep_cost != 1)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

TimePlanner::TimePlanner() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

TimePlanner::~TimePlanner() { (void)bind(-1); }

int TimePlanner::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_policy, (void*)d_c, (void*)d_cost0, (void*)d_lay, (void*)d_all, (void*)d_tab, (void*)d_stat, (void*)d_goals,
                        (void*)d_starts, (void*)d_off, (void*)d_scost, (void*)d_status, (void*)d_points, (void*)d_cd, (void*)d_ci, (void*)d_u,
                        (void*)d_hp, (void*)d_cl})
            (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_policy = nullptr; d_c = d_cost0 = d_lay = d_all = nullptr; d_tab = nullptr; d_stat = nullptr; d_goals = d_starts = nullptr;
    d_off = nullptr; d_scost = nullptr; d_status = nullptr; d_points = nullptr; d_cd = nullptr; d_ci = nullptr; d_u = d_hp = nullptr;
    d_cl = nullptr; own = nullptr;
    cap_policy = cap_n = cap_all = cap_goals = cap_starts = cap_points = cap_cd = cap_ci = cap_u = cap_hp = cap_cl = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int TimePlanner::solve(const DistanceField& df, const Obstacles* ob, const float* goals, int ngoals, double tb, const TimePlanOpts& o,
                       hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int H = o.horizon, nb = ob ? ob->n : 0;
    const long long pts = df.ngrid;
    if (!d_stat) GPIS_HIP(hipMalloc((void**)&d_stat, sizeof(unsigned long long) * kTStatWords));
    if (!d_tab) GPIS_HIP(hipMalloc((void**)&d_tab, sizeof(double) * Obstacles::kMax * Obstacles::kRow));
    if ((size_t)pts > cap_n) {
        for (void* p : {(void*)d_c, (void*)d_cost0, (void*)d_lay}) (void)hipFree(p);
        d_c = d_cost0 = d_lay = nullptr; cap_n = 0;
        GPIS_HIP(hipMalloc((void**)&d_c, sizeof(float) * pts));
        GPIS_HIP(hipMalloc((void**)&d_cost0, sizeof(float) * pts));
        GPIS_HIP(hipMalloc((void**)&d_lay, sizeof(float) * 2 * pts));
        cap_n = (size_t)pts;
    }
    if (int rc = grow(d_policy, cap_policy, (size_t)pts * (H + 1))) return rc;
    if (o.keep_cost)
        if (int rc = grow(d_all, cap_all, (size_t)pts * (H + 1))) return rc;
    if (int rc = grow(d_goals, cap_goals, (size_t)ngoals * 2)) return rc;

    const int gx = df.n[0], gy = df.n[1], tnx = (gx + kT - 1) / kT, tny = (gy + kT - 1) / kT;
    const PlanLat L{2, gx, gy, 1, df.origin[0], df.origin[1], 0.f, df.step};
    const TLat G{gx, gy, df.origin[0], df.origin[1], df.step};
    const double TB = nb ? tb - ob->epoch : 0.0;
    GPIS_HIP(hipMemcpyAsync(d_goals, goals, sizeof(float) * (size_t)ngoals * 2, hipMemcpyHostToDevice, s));
    if (nb) GPIS_HIP(hipMemcpyAsync(d_tab, ob->d_tab, sizeof(double) * (size_t)nb * Obstacles::kRow, hipMemcpyDeviceToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * kTStatWords, s));
    float* top = d_lay;
    unsigned char* pol_top = d_policy + (size_t)H * pts;
    hipLaunchKernelGGL(tplan_setup_kernel, dim3(grid_for(pts)), dim3(kBlock), 0, s, df.d_dist, (int)pts, o.clearance, o.margin, o.gain, d_c,
                       top, pol_top);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(tplan_goal_kernel, dim3(grid_for(ngoals)), dim3(kBlock), 0, s, L, d_goals, ngoals, d_c, top, pol_top, d_stat);
    GPIS_HIP(hipGetLastError());
    if (o.keep_cost) GPIS_HIP(hipMemcpyAsync(d_all + (size_t)H * pts, top, sizeof(float) * pts, hipMemcpyDeviceToDevice, s));

    // (0: the faster of the measured schedules, §7y: without balls a layer is launch-bound and four share a launch; with
    // balls the ghost rings' repeated separations cost more than the launches save)
    const int Lmax = layers_per_launch > 0 ? std::min(layers_per_launch, (int)kMaxLayers) : (nb == 0 ? (int)kLayersNoBalls : 1);
    const float wwait = o.wait * df.step;
    int cur = 0;
    long long nl = 0;
    for (int s_hi = H; s_hi > 0;) {
        const int Lb = std::min(Lmax, s_hi), W = kT + 2 * Lb;
        hipLaunchKernelGGL(tplan_layer_kernel, dim3((unsigned)(tnx * tny)), dim3(kLayerBlock), sizeof(float) * 3 * W * W, s, G, tnx, d_c,
                           d_lay + (size_t)cur * pts, d_lay + (size_t)(cur ^ 1) * pts, d_policy, o.keep_cost ? d_all : nullptr, s_hi, Lb,
                           o.connectivity, wwait, o.slot, TB, o.dyn_clearance, d_tab, nb, cull, d_stat);
        GPIS_HIP(hipGetLastError());
        s_hi -= Lb; cur ^= 1; ++nl;
    }
    hipLaunchKernelGGL(tplan_finish_kernel, dim3(grid_for(pts)), dim3(kBlock), 0, s, d_c, d_lay + (size_t)cur * pts, (int)pts, d_cost0, d_stat);
    GPIS_HIP(hipGetLastError());
    unsigned long long st[kTStatWords];
    GPIS_HIP(hipMemcpyAsync(st, d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    nx = gx; ny = gy; S = H; n = nb; np = pts; step = df.step; origin[0] = df.origin[0]; origin[1] = df.origin[1];
    opts = o; t_begin = tb;
    goals_given = ngoals; goals_kept = (long long)st[kTStatKept]; skipped = (long long)st[kTStatSkipped];
    nfree = (long long)st[kTStatFree]; nfinite = (long long)st[kTStatFinite]; launches = nl;
    const unsigned mb = (unsigned)st[kTStatMax];
    std::memcpy(&max_cost0, &mb, sizeof(float));
    solve_ms = plan_host::ms_since(t0);
    kept = o.keep_cost != 0;
    valid = true;
    return GPIS_OK;
}

int TimePlanner::paths(const float* starts, int m, hipStream_t s) {
    paths_valid = false;
    const PlanLat L{2, nx, ny, 1, origin[0], origin[1], 0.f, step};
    const auto walk = [&](auto kernel, float* points) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, L, S, d_c, d_cost0, d_policy, d_starts, m, d_off, d_scost, d_status,
                           points);
    };
    if (int rc = plan_host::run_paths(
            s, starts, m, 2, d_starts, cap_starts, d_off, d_scost, d_status, npoints, [&] { walk(tplan_walk_kernel<false>, nullptr); },
            [&](size_t total) { return grow(d_points, cap_points, total * 2); }, [&] { walk(tplan_walk_kernel<true>, d_points); }))
        return rc;
    npaths = m;
    paths_valid = true;
    return GPIS_OK;
}

int TimePlanner::check(const Obstacles& ob, double clearance, double* min_sep, double* min_time, int* min_obstacle, int* first_hit,
                       int* collides) {
    const size_t m = (size_t)npaths;
    if (int rc = grow(d_cd, cap_cd, m * 2)) return rc;
    if (int rc = grow(d_ci, cap_ci, m * 3)) return rc;
    hipLaunchKernelGGL(tplan_check_kernel, dim3((unsigned)m), dim3(kBlock), 0, own, d_off, d_status, d_points, opts.slot,
                       t_begin - ob.epoch, clearance, ob.d_tab, ob.n, d_cd, d_ci);
    GPIS_HIP(hipGetLastError());
    std::vector<double> hd(m * 2);
    std::vector<int> hi(m * 3);
    GPIS_HIP(hipMemcpyAsync(hd.data(), d_cd, sizeof(double) * m * 2, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipMemcpyAsync(hi.data(), d_ci, sizeof(int) * m * 3, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    for (size_t k = 0; k < m; ++k) {
        if (min_sep) min_sep[k] = hd[2 * k];
        if (min_time) min_time[k] = hd[2 * k + 1];
        if (min_obstacle) min_obstacle[k] = hi[3 * k];
        if (first_hit) first_hit[k] = hi[3 * k + 1];
        if (collides) collides[k] = hi[3 * k + 2];
    }
    return GPIS_OK;
}

int TimePlanner::controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    const size_t m = (size_t)npaths;
    if (int rc = grow(d_u, cap_u, m * T * 2)) return rc;
    if (int rc = grow(d_hp, cap_hp, m * 4)) return rc;
    if (int rc = grow(d_cl, cap_cl, m)) return rc;
    const int threads = 64 * ((T + 63) / 64);
    hipLaunchKernelGGL(tplan_controls_kernel, dim3((unsigned)m), dim3(threads), 0, own, d_off, d_status, d_points, d_starts, T, k0,
                       opts.slot, w_limit, min_move, d_u, d_hp, d_cl);
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

}  // namespace gpis
