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
#include "tplan.h"
#include "dfield.h"
#include "plan_host.h"
#include "tplan_dev.h"

namespace gpis {

namespace {

using namespace tplan_dev;

constexpr int kLayerBlock = 1024;        // the layer kernel: one thread per tile point, so that a point's chain over the balls is short
constexpr int kT = TimePlanner::kTile;

struct TLat {
    int nx, ny;
    float ox, oy, step;
};

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
        atomicAdd(&stat[TimePlanCore::kStatKept], 1ull);
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
    // the broad phase over the launch's Lb layers and the tile with its ghost zone (the proof needs > r + clr; two lattice steps
    // more are the margin); its barrier publishes s_c and s_h0
    broad_phase(tab, n, cull, TB + (double)(s_hi - Lb) * slot, TB + (double)s_hi * slot, world(G.ox, gi0, G.step),
                world(G.ox, gi0 + W - 1, G.step), world(G.oy, gj0, G.step), world(G.oy, gj0 + W - 1, G.step),
                [clr, step = G.step](const double* row) { return (row[6] + clr) + 2.0 * (double)step; }, s_keep, stat);

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
                                        double t;
                                        const double sep = closest_approach(Ax, Ay, Bx, By, t) - rad;
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
// out_d[tr][2] = min_sep, min_time; out_i[tr][4] = min_obstacle, first_hit, collides, -1 (check_begin() / check_finish()).
__global__ void __launch_bounds__(kBlock) tplan_check_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ status,
                                                             const float* __restrict__ pts, double dt, double TB, double clearance,
                                                             const double* __restrict__ tab, int n, double* __restrict__ out_d,
                                                             int* __restrict__ out_i) {
    const int tr = blockIdx.x, tid = threadIdx.x;
    long long o;
    int A;
    if (!check_begin(off, status, n, o, A, out_d, out_i)) return;
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
            const double o0x = row[0] + row[3] * e0, o1x = row[0] + row[3] * e1;
            const double o0y = row[1] + row[4] * e0, o1y = row[1] + row[4] * e1;
            double s;
            const double sep = closest_approach(p0[0] - o0x, p0[1] - o0y, dp[0] - (o1x - o0x), dp[1] - (o1y - o0y), s) - row[6];
            if (sep < best) { best = sep; best_s = s; best_k = k; best_i = i; }
            if (sep < clearance && k < hit) hit = k;
        }
    }
    const unsigned long long key = best_k >= 0 ? ((unsigned long long)best_k << 8) | (unsigned long long)best_i : ~0ull;
    if (check_finish(best, key, hit, out_d, out_i)) {
        out_d[(size_t)tr * 2] = best;
        out_d[(size_t)tr * 2 + 1] = (double)best_k * dt + best_s * dt;
        out_i[(size_t)tr * 4] = best_i;
    }
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

int TimePlanner::solve(const DistanceField& df, const Obstacles* ob, const float* goals, int ngoals, double tb, const TimePlanOpts& o,
                       hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int H = o.horizon, nb = ob ? ob->n : 0;
    const long long pts = df.ngrid;
    if (int rc = reserve(pts, H, o.keep_cost, ngoals, 2)) return rc;

    const int gx = df.n[0], gy = df.n[1], tnx = (gx + kT - 1) / kT, tny = (gy + kT - 1) / kT;
    const PlanLat L{2, gx, gy, 1, df.origin[0], df.origin[1], 0.f, df.step};
    const TLat G{gx, gy, df.origin[0], df.origin[1], df.step};
    const double TB = nb ? tb - ob->epoch : 0.0;
    GPIS_HIP(hipMemcpyAsync(d_goals, goals, sizeof(float) * (size_t)ngoals * 2, hipMemcpyHostToDevice, s));
    if (nb) GPIS_HIP(hipMemcpyAsync(d_tab, ob->d_tab, sizeof(double) * (size_t)nb * Obstacles::kRow, hipMemcpyDeviceToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * kStatWords, s));
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
    hipLaunchKernelGGL(tplan_finish_kernel, dim3(grid_for(pts)), dim3(kBlock), 0, s, d_c, d_lay + (size_t)cur * pts, pts, d_cost0, d_stat);
    GPIS_HIP(hipGetLastError());
    if (int rc = read_stats(s)) return rc;
    nx = gx; ny = gy; S = H; n = nb; ns = pts; step = df.step; origin[0] = df.origin[0]; origin[1] = df.origin[1];
    opts = o; t_begin = tb;
    goals_given = ngoals; launches = nl;
    solve_ms = ms_since(t0);
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
    return run_check(
        [&] {
            hipLaunchKernelGGL(tplan_check_kernel, dim3((unsigned)npaths), dim3(kBlock), 0, own, d_off, d_status, d_points, opts.slot,
                               t_begin - ob.epoch, clearance, ob.d_tab, ob.n, d_cd, d_ci);
        },
        min_sep, min_time, min_obstacle, nullptr, first_hit, collides);
}

int TimePlanner::controls(int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0, int* clamped) {
    return run_controls(tplan_controls_kernel, 2, opts.slot, T, k0, w_limit, min_move, U, heading0, p0, clamped);
}

}  // namespace gpis
