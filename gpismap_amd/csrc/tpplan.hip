// Planning through space and time for the robot's footprint (tpplan.h; the contract: tests/tpplan_ref.py).
//
// State (i, j, h, s): index (h ny + j) nx + i within layer s; world point P = (double)(o + (float)i * step) per axis.  Move bits
// b = 0 .. 8 of the offset (dx, dy) = (b % 3 - 1, b / 3 - 1): the planner's code 9 + b, and bit 4 is the wait (code 29); bit 9 is
// the turn to h + 1 (code 27), bit 10 the turn to h - 1 (code 28).  Every move takes one slot.
//
// Layer kernel: the pose planner's tile (8 x 8 lattice points x all H headings, 256 threads), so the heading's wrap-around stays
// inside a tile and only a one-point xy halo of c and of the layer above is loaded into LDS.  One launch computes one layer: a
// launch reads one global cost layer and writes the other, so no workgroup reads what another writes.  A thread owns a point in
// H / 4 heading layers; the heading of a state is the same in every lane of a wavefront, so the rotated body offsets rot[h][j] =
// (c_h b0 - s_h b1, s_h b0 + c_h b1) (tabulated on the host in double, the body rule's own operations) and the ball table come
// through scalar loads.  Per (state, moving ball, body ball) W0 - o_s and o_{s+1} - o_s are formed once and shared by the moves;
// a move's separation is evaluated only where the move exists and its target is finite.
//
// Broad phase (cull): thread i decides whether ball i can come within dyn_clearance of any body ball during any move of this
// (tile, layer): the box of the tile's and its halo's world points against the box of the ball's centre at the layer's two ends,
// with beta = the largest |rot[h][j]| + rho_j (§7z has the proof).  A skipped ball is work left out, not an early-out in the
// expression.
#include <chrono>
#include <cmath>
#include <vector>
#include "tpplan.h"
#include "dfield.h"
#include "plan_host.h"
#include "tplan_dev.h"

namespace gpis {

namespace {

using namespace tplan_dev;

constexpr int kT = TimePosePlanner::kTile, kW = kT + 2, kLayer = kW * kW;
constexpr int kMB = Footprint::kMax;
constexpr unsigned kBitWait = 1u << 4, kBitUp = 1u << 9, kBitDown = 1u << 10;

struct TPLat {
    int nx, ny, H;
    float ox, oy, step;
};

// what the layer kernel takes of the moving balls and of the body
struct TPBalls {
    const double* tab;               // [n][Obstacles::kRow]
    int n;
    const double* rot;               // [H][kMB][2]
    const double* body;              // [mb][4]: the radius at [3]
    int mb;
    double e0, e1;                   // the elapsed times of the layer's two ends
    double clr;
    double reach;                    // beta + dyn_clearance + 2 step (beta: the body's reach, radii included)
    int cull;
};

constexpr int b_dx(int b) { return b % 3 - 1; }
constexpr int b_dy(int b) { return b / 3 - 1; }
constexpr int b_nnz(int b) { return (b_dx(b) != 0) + (b_dy(b) != 0); }
// the free bits translation b needs: the state itself and p + every non-empty subset of the offset's components
constexpr unsigned b_need(int b) {
    unsigned m = (1u << 4) | (1u << b);
    if (b_dx(b)) m |= 1u << (3 + b_dx(b) + 1);
    if (b_dy(b)) m |= 1u << ((b_dy(b) + 1) * 3 + 1);
    return m;
}

// The pose planner's set-up (pplan.hip) for the top layer: one thread per state, one heading per blockIdx.y.  c = the point cost of
// (float)D (0: not free; a NaN D is not free), the top layer's cost +inf and policy 255
__global__ void __launch_bounds__(kBlock) tpplan_setup_kernel(const float* __restrict__ F, DfLattice L, BodyArgs bd, const double* __restrict__ head,
                                                              float clearance, float margin, float gain, float* __restrict__ c,
                                                              float* __restrict__ top, unsigned char* __restrict__ pol_top) {
    const int h = blockIdx.y, nxy = L.nx * L.ny;
    const int p = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= nxy) return;
    const double ch = head[2 * h], sh = head[2 * h + 1];
    const int i = p % L.nx, j = p / L.nx;
    const double pos[2] = {(double)(L.ox + (float)i * L.st), (double)(L.oy + (float)j * L.st)};
    const float d = (float)body_clearance_at<2>(F, L, bd.tab, bd.m, pos, ch, sh);
    const size_t s = (size_t)h * nxy + p;
    c[s] = point_cost(d, clearance, margin, gain);
    top[s] = INFINITY;
    pol_top[s] = 255;
}

// the kept goal states: cost 0 and policy 13 in the top layer (idempotent: duplicates write the same bits).  A goal's heading -1
// stands for every free heading at its point, each counted.
__global__ void __launch_bounds__(kBlock) tpplan_goal_kernel(TPLat L, const float* __restrict__ goals, int ngoals, const float* __restrict__ c,
                                                             float* __restrict__ top, unsigned char* __restrict__ pol_top,
                                                             unsigned long long* __restrict__ stat) {
    const PlanLat L2{2, L.nx, L.ny, 1, L.ox, L.oy, 0.f, L.step};
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngoals; g += gridDim.x * blockDim.x) {
        int q[3];
        if (!snap(L2, goals + (size_t)g * 3, q)) continue;
        const int hg = (int)goals[(size_t)g * 3 + 2];
        const int h0 = hg < 0 ? 0 : hg, h1 = hg < 0 ? L.H - 1 : hg;
        unsigned kept = 0;
        for (int h = h0; h <= h1; ++h) {
            const size_t s = ((size_t)h * L.ny + q[1]) * L.nx + q[0];
            if (!(c[s] > 0.f)) continue;
            top[s] = 0.f;
            pol_top[s] = 13;
            ++kept;
        }
        if (kept) atomicAdd(&stat[TimePlanCore::kStatKept], (unsigned long long)kept);
    }
}

// Layer s from layer s + 1 (hin) into hout.  A goal is known by its cost 0 in the layer above: every translation and every turn
// weighs more than 0 (c >= 1 at a free state, step > 0, turn > 0), and a wait of weight 0 keeps a cost that was 0 only at a goal,
// so by induction from the top layer no other state ever has cost 0.
template <int HH>
__global__ void __launch_bounds__(kBlock) tpplan_layer_kernel(TPLat G, int tnx, const float* __restrict__ c, const float* __restrict__ hin,
                                                              float* __restrict__ hout, unsigned char* __restrict__ policy,
                                                              float* __restrict__ cost_s, const unsigned short* __restrict__ moves,
                                                              float turn, float wwait, TPBalls B, unsigned long long* __restrict__ stat) {
    constexpr int NH = kLayer * HH, CPT = HH * kT * kT / kBlock;
    static_assert(HH * kT * kT % kBlock == 0 && (HH & (HH - 1)) == 0, "states per thread");
    __shared__ float s_h[NH];
    __shared__ float s_c[NH];
    __shared__ unsigned short s_mv[HH];
    __shared__ unsigned s_keep[Obstacles::kMax / 32];
    static_assert(Obstacles::kMax == kBlock, "one thread per ball in the broad phase");
    const int tid = threadIdx.x, ti = blockIdx.x % tnx, tj = blockIdx.x / tnx;
    if (tid < HH) s_mv[tid] = moves[tid];
    for (int e = tid; e < NH; e += kBlock) {
        const int lh = e / kLayer, r = e % kLayer;
        const int gi = ti * kT + r % kW - 1, gj = tj * kT + r / kW - 1;
        const bool in = gi >= 0 && gi < G.nx && gj >= 0 && gj < G.ny;
        const size_t s = in ? ((size_t)lh * G.ny + gj) * G.nx + gi : 0;
        s_c[e] = in ? c[s] : 0.f;
        s_h[e] = in ? hin[s] : INFINITY;
    }
    // the broad phase over this layer and the tile with its halo (the proof needs > beta + r + clr; two lattice steps more are
    // the margin); its barrier publishes s_mv, s_c and s_h
    broad_phase(B.tab, B.n, B.cull, B.e0, B.e1, world(G.ox, ti * kT - 1, G.step), world(G.ox, ti * kT + kT, G.step),
                world(G.oy, tj * kT - 1, G.step), world(G.oy, tj * kT + kT, G.step),
                [reach = B.reach](const double* row) { return reach + row[6]; }, s_keep, stat);

    // thread tid: the point (li, lj) of the tile in the layers l0, l0 + 4, ...; l0 is the wavefront's index
    const int li = tid & (kT - 1), lj = (tid >> 3) & (kT - 1), l0 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gi = ti * kT + li, gj = tj * kT + lj;
    const bool inside = gi < G.nx && gj < G.ny;
    const int base = (lj + 1) * kW + li + 1;
    const double Px[3] = {world(G.ox, gi - 1, G.step), world(G.ox, gi, G.step), world(G.ox, gi + 1, G.step)};
    const double Py[3] = {world(G.oy, gj - 1, G.step), world(G.oy, gj, G.step), world(G.oy, gj + 1, G.step)};
    const float ls[2] = {G.step, sqrtf(2.f) * G.step};
#pragma unroll 1
    for (int s = 0; s < CPT; ++s) {
        const int lh = l0 + 4 * s, lu = (lh + 1) & (HH - 1), ld = (lh + HH - 1) & (HH - 1);
        const int hi = lh * kLayer + base, up = lu * kLayer + base, dn = ld * kLayer + base;
        const float cp = s_c[hi];
        float hv = INFINITY;
        unsigned char pol = 255;
        if (cp > 0.f) {
            if (s_h[hi] == 0.f) { hv = 0.f; pol = 13; }
            else {
                unsigned nb = 0;
#pragma unroll
                for (int b = 0; b < 9; ++b)
                    if (s_c[hi + b_dy(b) * kW + b_dx(b)] > 0.f) nb |= 1u << b;
                unsigned open = kBitWait;                // (the state is free)
#pragma unroll
                for (int b = 0; b < 9; ++b) {
                    if (b == 4) continue;
                    if ((nb & b_need(b)) == b_need(b)) open |= 1u << b;
                }
                open &= (unsigned)s_mv[lh] | kBitWait;
                if (s_c[up] > 0.f) open |= kBitUp;
                if (s_c[dn] > 0.f) open |= kBitDown;
                unsigned cand = 0;
#pragma unroll
                for (int b = 0; b < 9; ++b)
                    if (((open >> b) & 1u) && s_h[hi + b_dy(b) * kW + b_dx(b)] < INFINITY) cand |= 1u << b;
                if ((open & kBitUp) && s_h[up] < INFINITY) cand |= kBitUp;
                if ((open & kBitDown) && s_h[dn] < INFINITY) cand |= kBitDown;
                if (cand && B.n > 0) {
                    unsigned blocked = 0;
                    const double* __restrict__ rh = B.rot + (size_t)lh * kMB * 2;
                    const double* __restrict__ ru = B.rot + (size_t)lu * kMB * 2;
                    const double* __restrict__ rd = B.rot + (size_t)ld * kMB * 2;
                    for (int w = 0; w < Obstacles::kMax / 32; ++w) {
                        unsigned mk = __builtin_amdgcn_readfirstlane(s_keep[w]);
                        while (mk) {
                            const int i = w * 32 + (__ffs(mk) - 1);
                            mk &= mk - 1;
                            const double* __restrict__ row = B.tab + (size_t)i * Obstacles::kRow;
                            const double o0x = row[0] + row[3] * B.e0, o1x = row[0] + row[3] * B.e1;
                            const double o0y = row[1] + row[4] * B.e0, o1y = row[1] + row[4] * B.e1;
                            const double dox = o1x - o0x, doy = o1y - o0y, rad = row[6];
                            for (int j = 0; j < B.mb; ++j) {
                                const double r0 = rh[2 * j], r1 = rh[2 * j + 1], rho = B.body[4 * j + 3];
                                const double W0x = Px[1] + r0, W0y = Py[1] + r1;
                                const double Ax = W0x - o0x, Ay = W0y - o0y;
#pragma unroll
                                for (int m = 0; m < 11; ++m) {
                                    if ((cand >> m) & 1u) {
                                        double W1x, W1y;
                                        if (m < 9) { W1x = Px[m % 3] + r0; W1y = Py[m / 3] + r1; }
                                        else if (m == 9) { W1x = Px[1] + ru[2 * j]; W1y = Py[1] + ru[2 * j + 1]; }
                                        else { W1x = Px[1] + rd[2 * j]; W1y = Py[1] + rd[2 * j + 1]; }
                                        const double Bx = (W1x - W0x) - dox, By = (W1y - W0y) - doy;
                                        double t;
                                        const double sep = (closest_approach(Ax, Ay, Bx, By, t) - rad) - rho;
                                        if (sep < B.clr) blocked |= 1u << m;   // (a NaN separation is not below the clearance)
                                    }
                                }
                            }
                        }
                    }
                    cand &= ~blocked;
                }
                float best = INFINITY, bestq = INFINITY;
#pragma unroll
                for (int b = 0; b < 9; ++b) {
                    if (b == 4) continue;
                    if ((cand >> b) & 1u) {
                        const int hq = hi + b_dy(b) * kW + b_dx(b);
                        better_move(s_h[hq] + ls[b_nnz(b) - 1] * (0.5f * (cp + s_c[hq])), s_h[hq], 9 + b, best, bestq, pol);
                    }
                }
                if (cand & kBitUp) better_move(s_h[up] + turn * (0.5f * (cp + s_c[up])), s_h[up], TimePosePlanner::kTurnUp, best, bestq, pol);
                if (cand & kBitDown) better_move(s_h[dn] + turn * (0.5f * (cp + s_c[dn])), s_h[dn], TimePosePlanner::kTurnDown, best, bestq, pol);
                if (cand & kBitWait) better_move(s_h[hi] + wwait * cp, s_h[hi], TimePosePlanner::kWait, best, bestq, pol);
                hv = best;
            }
        }
        if (inside) {
            const size_t p = ((size_t)lh * G.ny + gj) * G.nx + gi;
            policy[p] = pol;
            if (cost_s) cost_s[p] = hv;
            hout[p] = hv;
        }
    }
}

// One thread per start follows the policy from slot 0.  WRITE = false: off[t] = entries of the path (arrive + 1; 0 without a
// path), status, start cost.  WRITE = true: the same walk again, one point and one heading index per slot stored from off[t]
// on.  A start's heading -1 stands for the free heading of least slot-0 cost at its point (ties: the smaller h; none free:
// status 2, start cost +inf).
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) tpplan_walk_kernel(TPLat L, int S, const float* __restrict__ c, const float* __restrict__ cost0,
                                                             const unsigned char* __restrict__ policy, const float* __restrict__ starts, int m,
                                                             long long* __restrict__ off, float* __restrict__ scost,
                                                             unsigned char* __restrict__ status, float* __restrict__ points,
                                                             int* __restrict__ pheading) {
    const PlanLat L2{2, L.nx, L.ny, 1, L.ox, L.oy, 0.f, L.step};
    const size_t nxy = (size_t)L.nx * L.ny, ns = nxy * L.H;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        int q[3];
        long long cnt = 0;
        unsigned char st = 0;
        float sc = NAN;
        if (!snap(L2, starts + (size_t)t * 3, q)) st = 1;
        else {
            int h = (int)starts[(size_t)t * 3 + 2];
            const size_t p0 = (size_t)q[1] * L.nx + q[0];
            if (h < 0) {
                float bc = INFINITY;
                for (int hh = 0; hh < L.H; ++hh) {
                    const size_t s = hh * nxy + p0;
                    if (c[s] > 0.f && (h < 0 || cost0[s] < bc)) { h = hh; bc = cost0[s]; }
                }
            }
            if (h < 0) { st = 2; sc = INFINITY; }
            else {
                size_t p = h * nxy + p0;
                sc = cost0[p];
                if (!(c[p] > 0.f)) st = 2;
                else if (!(sc < INFINITY)) st = 3;
                else {
                    const long long o = WRITE ? off[t] : 0;
                    for (int s = 0;; ++s) {
                        if (WRITE) {
                            points[(size_t)(o + cnt) * 2] = L.ox + (float)q[0] * L.step;
                            points[(size_t)(o + cnt) * 2 + 1] = L.oy + (float)q[1] * L.step;
                            pheading[o + cnt] = h;
                        }
                        ++cnt;
                        const int k = policy[(size_t)s * ns + p];
                        if (k == 13) break;
                        if (s >= S) { st = 4; break; }                      // (cannot happen on a finished plan)
                        int qi = q[0], qj = q[1], qh = h;
                        if (k == TimePosePlanner::kTurnUp) qh = (h + 1) % L.H;
                        else if (k == TimePosePlanner::kTurnDown) qh = (h + L.H - 1) % L.H;
                        else if (k >= 9 && k < 18) { qi += b_dx(k - 9); qj += b_dy(k - 9); }
                        else if (k != TimePosePlanner::kWait) { st = 4; break; }
                        if (qi < 0 || qi >= L.nx || qj < 0 || qj >= L.ny) { st = 4; break; }
                        q[0] = qi; q[1] = qj; h = qh;
                        p = ((size_t)h * L.ny + qj) * L.nx + qi;
                    }
                }
            }
        }
        if (!WRITE) { off[t] = cnt; scost[t] = sc; status[t] = st; }
    }
}

// A pose path against a set of moving balls with a footprint: traj_body_time_check_kernel's rule (traj.hip, §7x) on the path's
// own poses, one per slot.  One workgroup per path; a thread per interval takes the moving balls i and inside them the body
// balls j (both tables through scalar loads) and keeps its own least (sep, s, i, j) by a strict comparison in ascending order;
// the block takes the least sep, then the least key (s << 12 | i << 4 | j) among the threads that hold it.
// out_d[tr][2] = min_sep, min_time; out_i[tr][4] = min_obstacle, first_hit, collides, min_ball (check_begin() / check_finish()).
__global__ void __launch_bounds__(kBlock) tpplan_check_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ status,
                                                              const float* __restrict__ pts, const int* __restrict__ hd,
                                                              const double* __restrict__ head, double dt, double TB, double clearance,
                                                              const double* __restrict__ tab, int n, BodyArgs bd,
                                                              double* __restrict__ out_d, int* __restrict__ out_i) {
    typedef unsigned long long u64;
    const int tr = blockIdx.x, tid = threadIdx.x;
    long long o;
    int A;
    if (!check_begin(off, status, n, o, A, out_d, out_i)) return;
    double best = INFINITY, best_s = 0.0;
    int best_k = -1, best_i = -1, best_j = -1, hit = 0x7fffffff;
    for (int k = tid; k < A; k += kBlock) {
        const double e0 = TB + (double)k * dt, e1 = TB + (double)(k + 1) * dt;
        const double p0x = (double)pts[(size_t)(o + k) * 2], p0y = (double)pts[(size_t)(o + k) * 2 + 1];
        const double p1x = (double)pts[(size_t)(o + k + 1) * 2], p1y = (double)pts[(size_t)(o + k + 1) * 2 + 1];
        const int h0 = hd[o + k], h1 = hd[o + k + 1];
        const double c0 = head[2 * h0], s0 = head[2 * h0 + 1], c1 = head[2 * h1], s1 = head[2 * h1 + 1];
        const double* __restrict__ row = tab;
        for (int i = 0; i < n; ++i, row += Obstacles::kRow) {
            const double o0x = row[0] + row[3] * e0, o1x = row[0] + row[3] * e1;
            const double o0y = row[1] + row[4] * e0, o1y = row[1] + row[4] * e1;
            const double dox = o1x - o0x, doy = o1y - o0y, rad = row[6];
            const double* __restrict__ brow = bd.tab;
            for (int j = 0; j < bd.m; ++j, brow += 4) {
                const double b0 = brow[0], b1 = brow[1];
                const double W0x = p0x + (c0 * b0 - s0 * b1), W0y = p0y + (s0 * b0 + c0 * b1);
                const double W1x = p1x + (c1 * b0 - s1 * b1), W1y = p1y + (s1 * b0 + c1 * b1);
                const double Ax = W0x - o0x, Ay = W0y - o0y;
                const double Bx = (W1x - W0x) - dox, By = (W1y - W0y) - doy;
                double t;
                const double sep = (closest_approach(Ax, Ay, Bx, By, t) - rad) - brow[3];
                if (sep < best) { best = sep; best_s = t; best_k = k; best_i = i; best_j = j; }
                if (sep < clearance && k < hit) hit = k;
            }
        }
    }
    const u64 key = best_k >= 0 ? ((u64)best_k << 12) | ((u64)best_i << 4) | (u64)best_j : ~0ull;
    if (check_finish(best, key, hit, out_d, out_i)) {
        out_d[(size_t)tr * 2] = best;
        out_d[(size_t)tr * 2 + 1] = (double)best_k * dt + best_s * dt;
        out_i[(size_t)tr * 4] = best_i; out_i[(size_t)tr * 4 + 3] = best_j;
    }
}

}  // namespace

int tpplan_check_opts(const TimePosePlanOpts& o, float step) {
    if (!std::isfinite(o.clearance) || !(std::isfinite(o.margin) && o.margin >= 0.f) || !(std::isfinite(o.gain) && o.gain >= 0.f) ||
        !std::isfinite(o.turn))
        return GPIS_ERR_ARG;
    if (o.gain > 1e4f || !(o.turn > 0.f)) return GPIS_ERR_ARG;
    if (step > 0.f && !(o.turn >= step / 64.f && o.turn <= 1e4f * step)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.slot) && o.slot > 0.0) || !(std::isfinite(o.dyn_clearance) && o.dyn_clearance >= 0.0)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.wait) && o.wait >= 0.f && o.wait <= TimePosePlanner::kMaxWait)) return GPIS_ERR_ARG;
    if (o.horizon < 1 || o.horizon > TimePosePlanner::kMaxHorizon || (o.keep_cost != 0 && o.keep_cost != 1)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int TimePosePlanner::solve(const DistanceField& df, const Obstacles* ob, const Footprint& body, const double* headings,
                           const unsigned short* move_bits, int nh, const float* goals, int ngoals, double tb, const TimePosePlanOpts& o,
                           hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int Sn = o.horizon, nb = ob ? ob->n : 0, nbody = body.m;
    const int gx = df.n[0], gy = df.n[1], tnx = (gx + kTile - 1) / kTile, tny = (gy + kTile - 1) / kTile;
    const long long nxy = (long long)gx * gy, states = nxy * nh;
    if (int rc = reserve(states, Sn, o.keep_cost, ngoals, 3)) return rc;
    if (!d_body) GPIS_HIP(hipMalloc((void**)&d_body, sizeof(double) * kMB * Footprint::kRow));
    if (!d_head) GPIS_HIP(hipMalloc((void**)&d_head, sizeof(double) * 2 * kMaxH));
    if (!d_rot) GPIS_HIP(hipMalloc((void**)&d_rot, sizeof(double) * 2 * kMaxH * kMB));
    if (!d_moves) GPIS_HIP(hipMalloc((void**)&d_moves, sizeof(unsigned short) * kMaxH));
    // the footprint's rows and its rotated offsets per (heading, ball): the body rule's own operations, in double; beta = the
    // farthest any body ball reaches from the reference point: the largest |rot[h][j]| + rho_j
    std::vector<double> hbody((size_t)kMB * Footprint::kRow, 0.0), hrot((size_t)2 * kMaxH * kMB, 0.0);
    double beta = 0.0;
    for (int j = 0; j < nbody; ++j) {
        for (int a = 0; a < 3; ++a) hbody[(size_t)j * 4 + a] = body.b[j][a];
        hbody[(size_t)j * 4 + 3] = body.rho[j];
    }
    for (int h = 0; h < nh; ++h) {
        const double ch = headings[2 * h], sh = headings[2 * h + 1];
        for (int j = 0; j < nbody; ++j) {
            const double b0 = body.b[j][0], b1 = body.b[j][1];
            const double r0 = ch * b0 - sh * b1, r1 = sh * b0 + ch * b1;
            hrot[((size_t)h * kMB + j) * 2] = r0;
            hrot[((size_t)h * kMB + j) * 2 + 1] = r1;
            beta = std::max(beta, std::hypot(r0, r1) + body.rho[j]);
        }
    }
    const TPLat L{gx, gy, nh, df.origin[0], df.origin[1], df.step};
    DfLattice DL = df.lattice();
    DL.dim = 2;
    const double TB = nb ? tb - ob->epoch : 0.0;
    GPIS_HIP(hipMemcpyAsync(d_goals, goals, sizeof(float) * (size_t)ngoals * 3, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_head, headings, sizeof(double) * 2 * nh, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_moves, move_bits, sizeof(unsigned short) * nh, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_body, hbody.data(), sizeof(double) * hbody.size(), hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_rot, hrot.data(), sizeof(double) * hrot.size(), hipMemcpyHostToDevice, s));
    if (nb) GPIS_HIP(hipMemcpyAsync(d_tab, ob->d_tab, sizeof(double) * (size_t)nb * Obstacles::kRow, hipMemcpyDeviceToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * kStatWords, s));
    float* top = d_lay;
    unsigned char* pol_top = d_policy + (size_t)Sn * states;
    hipLaunchKernelGGL(tpplan_setup_kernel, dim3((unsigned)((nxy + kBlock - 1) / kBlock), (unsigned)nh), dim3(kBlock), 0, s, (const float*)df.d_dist,
                       DL, BodyArgs{d_body, nbody}, (const double*)d_head, o.clearance, o.margin, o.gain, d_c, top, pol_top);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(tpplan_goal_kernel, dim3(grid_for(ngoals)), dim3(kBlock), 0, s, L, (const float*)d_goals, ngoals, (const float*)d_c, top,
                       pol_top, d_stat);
    GPIS_HIP(hipGetLastError());
    if (o.keep_cost) GPIS_HIP(hipMemcpyAsync(d_all + (size_t)Sn * states, top, sizeof(float) * states, hipMemcpyDeviceToDevice, s));

    const auto layer_kernel = nh == 8 ? tpplan_layer_kernel<8> : nh == 16 ? tpplan_layer_kernel<16> : nh == 32 ? tpplan_layer_kernel<32>
                                                                                                               : tpplan_layer_kernel<64>;
    const float wwait = o.wait * df.step;
    TPBalls B{d_tab, nb, d_rot, d_body, nbody, 0.0, 0.0, o.dyn_clearance, (beta + o.dyn_clearance) + 2.0 * (double)df.step, cull};
    int cur = 0;
    for (int sl = Sn - 1; sl >= 0; --sl) {
        B.e0 = TB + (double)sl * o.slot;
        B.e1 = TB + (double)(sl + 1) * o.slot;
        hipLaunchKernelGGL(layer_kernel, dim3((unsigned)(tnx * tny)), dim3(kBlock), 0, s, L, tnx, (const float*)d_c,
                           (const float*)(d_lay + (size_t)cur * states), d_lay + (size_t)(cur ^ 1) * states, d_policy + (size_t)sl * states,
                           o.keep_cost ? d_all + (size_t)sl * states : nullptr, (const unsigned short*)d_moves, o.turn, wwait, B, d_stat);
        GPIS_HIP(hipGetLastError());
        cur ^= 1;
    }
    hipLaunchKernelGGL(tplan_finish_kernel, dim3(grid_for(states)), dim3(kBlock), 0, s, (const float*)d_c,
                       (const float*)(d_lay + (size_t)cur * states), states, d_cost0, d_stat);
    GPIS_HIP(hipGetLastError());
    if (int rc = read_stats(s)) return rc;
    nx = gx; ny = gy; H = nh; S = Sn; n = nb; mb = nbody; ns = states; step = df.step; origin[0] = df.origin[0]; origin[1] = df.origin[1];
    opts = o; t_begin = tb;
    goals_given = ngoals; launches = Sn;
    solve_ms = ms_since(t0);
    kept = o.keep_cost != 0;
    valid = true;
    return GPIS_OK;
}

int TimePosePlanner::paths(const float* starts, int m, hipStream_t s) {
    paths_valid = false;
    const TPLat L{nx, ny, H, origin[0], origin[1], step};
    const auto walk = [&](auto kernel, float* points, int* pheading) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, L, S, (const float*)d_c, (const float*)d_cost0,
                           (const unsigned char*)d_policy, (const float*)d_starts, m, d_off, d_scost, d_status, points, pheading);
    };
    const auto grow_points = [&](size_t need) -> int {          // both buffers at once, under the one capacity
        if (need <= cap_points) return GPIS_OK;
        (void)hipFree(d_points); (void)hipFree(d_pheading);
        d_points = nullptr; d_pheading = nullptr; cap_points = 0;
        GPIS_HIP(hipMalloc((void**)&d_points, sizeof(float) * 2 * need));
        GPIS_HIP(hipMalloc((void**)&d_pheading, sizeof(int) * need));
        cap_points = need;
        return GPIS_OK;
    };
    if (int rc = plan_host::run_paths(
            s, starts, m, 3, d_starts, cap_starts, d_off, d_scost, d_status, npoints, [&] { walk(tpplan_walk_kernel<false>, nullptr, nullptr); },
            grow_points, [&] { walk(tpplan_walk_kernel<true>, d_points, d_pheading); }))
        return rc;
    npaths = m;
    paths_valid = true;
    return GPIS_OK;
}

int TimePosePlanner::check(const Obstacles& ob, const Footprint* body, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                           int* min_ball, int* first_hit, int* collides) {
    const BodyArgs bd = body ? BodyArgs{body->d_tab, body->m} : BodyArgs{d_body, mb};
    return run_check(
        [&] {
            hipLaunchKernelGGL(tpplan_check_kernel, dim3((unsigned)npaths), dim3(kBlock), 0, own, (const long long*)d_off,
                               (const unsigned char*)d_status, (const float*)d_points, (const int*)d_pheading, (const double*)d_head,
                               opts.slot, t_begin - ob.epoch, clearance, (const double*)ob.d_tab, ob.n, bd, d_cd, d_ci);
        },
        min_sep, min_time, min_obstacle, min_ball, first_hit, collides);
}

int TimePosePlanner::controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    return run_controls(tplan_controls_kernel, 3, opts.slot, T, k0, w_limit, min_move, U, heading0, p0, clamped);
}

}  // namespace gpis
