// Routes for the robot's footprint (pplan.h): the path planner's solve on the lattice of poses (x, y, heading).
//
// State (i, j, h): index (h ny + j) nx + i, world point o + (float)i * step (no FMA: -ffp-contract=off).  Move codes: 9 + b for
// the translation by (dx, dy) with b = (dy + 1) 3 + (dx + 1) (the planner's 2-D direction codes; 13 is "stay"), 27 for the turn
// h -> h + 1 mod H, 28 for h -> h - 1 mod H.  c[s] = 0 marks a state that is not free (a free one has c >= 1).
//
// Solve: plan.hip's schedule and its invariant.  The lattice is cut into tiles of 8 x 8 points x all H layers, one workgroup of
// 256 threads per tile and outer round, so the heading's wrap-around is resolved inside a tile and only the xy halo of one point
// is loaded.  An active workgroup relaxes its states in place in LDS until an iteration changes nothing (or inner_cap
// iterations), stores the states it lowered, and raises the NEXT round's flag of every xy neighbour tile that has a lowered
// state in its halo (and its own at the cap).  Values only fall and fl(a + w) is monotone in a, so a stale read is merely
// larger, and the flag raised after the store makes the reader run again.  Integer atomics only (flags, counters).
#include <cmath>
#include "pplan.h"
#include "dfield.h"
#include "plan_host.h"

namespace gpis {

namespace {

using namespace plan_dev;

constexpr int kBlock = 256;
constexpr int kT = PosePlanner::kTile, kW = kT + 2, kLayer = kW * kW;
constexpr unsigned kBitUp = 1u << 9, kBitDown = 1u << 10;

struct PLat {
    int nx, ny, H;
    float ox, oy, step;
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
// the moves open at a state: nb = the free bits of its 9 xy neighbours in its layer (bit 4: the state itself), allowed = its
// heading's move bits, up / down = the same point is free in the layer above / below
__device__ __forceinline__ unsigned open_moves(unsigned nb, unsigned allowed, bool up, bool down) {
    if (!((nb >> 4) & 1u)) return 0;
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        if (b == 4) continue;
        if ((nb & b_need(b)) == b_need(b)) m |= 1u << b;
    }
    m &= allowed;
    if (up) m |= kBitUp;
    if (down) m |= kBitDown;
    return m;
}

// One thread per state, one heading per blockIdx.y: the heading and the footprint's table come through scalar loads.
// c = the point cost of (float)D (0: not free; a NaN D is not free), cost = +inf, policy = 255
__global__ void __launch_bounds__(kBlock) pplan_setup_kernel(const float* __restrict__ F, DfLattice L, BodyArgs bd, const double* __restrict__ head,
                                                             float clearance, float margin, float gain, float* __restrict__ c,
                                                             float* __restrict__ cost, unsigned char* __restrict__ policy) {
    const int h = blockIdx.y, nxy = L.nx * L.ny;
    const int p = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= nxy) return;
    const double ch = head[2 * h], sh = head[2 * h + 1];
    const int i = p % L.nx, j = p / L.nx;
    const double pos[2] = {(double)(L.ox + (float)i * L.st), (double)(L.oy + (float)j * L.st)};
    const float d = (float)body_clearance_at<2>(F, L, bd.tab, bd.m, pos, ch, sh);
    const size_t s = (size_t)h * nxy + p;
    c[s] = point_cost(d, clearance, margin, gain);
    cost[s] = INFINITY;
    policy[s] = 255;
}

// cost = 0 at the kept goal states (idempotent: duplicates write the same bits), their tiles active in round 0.  A goal's
// heading -1 stands for every free heading at its point.
__global__ void __launch_bounds__(kBlock) pplan_goal_kernel(PLat L, const float* __restrict__ goals, int ngoals, const float* __restrict__ c,
                                                            float* __restrict__ cost, int tnx, int* __restrict__ flags,
                                                            unsigned long long* __restrict__ stat) {
    const PlanLat L2{2, L.nx, L.ny, 1, L.ox, L.oy, 0.f, L.step};
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngoals; g += gridDim.x * blockDim.x) {
        int q[3];
        if (!snap(L2, goals + (size_t)g * 3, q)) continue;
        const int hg = (int)goals[(size_t)g * 3 + 2];
        const int h0 = hg < 0 ? 0 : hg, h1 = hg < 0 ? L.H - 1 : hg;
        unsigned kept = 0;
        for (int h = h0; h <= h1; ++h) {
            const int s = (h * L.ny + q[1]) * L.nx + q[0];
            if (!(c[s] > 0.f)) continue;
            cost[s] = 0.f;
            ++kept;
        }
        if (kept) {
            flags[(q[1] / kT) * tnx + q[0] / kT] = 1;
            atomicAdd(&stat[kStatKept], (unsigned long long)kept);
        }
    }
}

template <int HH>
__global__ void __launch_bounds__(kBlock) pplan_tile_kernel(PLat L, const float* __restrict__ c, float* cost, const unsigned short* __restrict__ moves,
                                                            int tnx, int tny, int* flags_cur, int* flags_next, float turn, int inner_cap,
                                                            unsigned long long* stat, unsigned long long* raised) {
    constexpr int NH = kLayer * HH, CPT = HH * kT * kT / kBlock;
    static_assert(HH * kT * kT % kBlock == 0 && (HH & (HH - 1)) == 0, "states per thread");
    __shared__ float s_cost[NH];
    __shared__ float s_c[NH];
    __shared__ unsigned short s_mv[HH];
    __shared__ int s_act;
    __shared__ unsigned s_nbr;
    const int tid = threadIdx.x, tile = blockIdx.x;
    if (!tile_begin(flags_cur, tile, s_act, s_nbr)) return;
    const int ti = tile % tnx, tj = tile / tnx;
    if (tid < HH) s_mv[tid] = moves[tid];
    for (int e = tid; e < NH; e += kBlock) {
        const int lh = e / kLayer, r = e % kLayer;
        const int gi = ti * kT + r % kW - 1, gj = tj * kT + r / kW - 1;
        const bool in = gi >= 0 && gi < L.nx && gj >= 0 && gj < L.ny;
        const int s = in ? (lh * L.ny + gj) * L.nx + gi : 0;
        s_c[e] = in ? c[s] : 0.f;
        s_cost[e] = in ? ld_cost(cost + s) : INFINITY;
    }
    __syncthreads();

    // thread tid: the point (li, lj) of the tile in the layers l0, l0 + 4, ...
    const int li = tid & (kT - 1), lj = (tid >> 3) & (kT - 1), l0 = tid >> 6;
    const int base = l0 * kLayer + (lj + 1) * kW + li + 1;
    unsigned open[CPT];
    float first[CPT];
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        const int lh = l0 + 4 * s, hi = base + 4 * kLayer * s;
        unsigned nb = 0;
#pragma unroll
        for (int b = 0; b < 9; ++b)
            if (s_c[hi + b_dy(b) * kW + b_dx(b)] > 0.f) nb |= 1u << b;
        const int up = hi + (((lh + 1) & (HH - 1)) - lh) * kLayer, dn = hi + (((lh + HH - 1) & (HH - 1)) - lh) * kLayer;
        open[s] = open_moves(nb, s_mv[lh], s_c[up] > 0.f, s_c[dn] > 0.f);
        first[s] = s_cost[hi];
    }
    const float ls[2] = {L.step, sqrtf(2.f) * L.step};
    bool capped = false;
    for (int it = 0;; ++it) {
        int ch = 0;
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
            if (!open[s]) continue;
            const int lh = l0 + 4 * s, hi = base + 4 * kLayer * s;
            const float cur = s_cost[hi], cp = s_c[hi];
            float best = cur;
#pragma unroll
            for (int b = 0; b < 9; ++b) {
                if (b == 4) continue;
                if ((open[s] >> b) & 1u) {
                    const int hq = hi + b_dy(b) * kW + b_dx(b);
                    const float w = ls[b_nnz(b) - 1] * (0.5f * (cp + s_c[hq]));
                    best = fminf(best, s_cost[hq] + w);
                }
            }
            if (open[s] & kBitUp) {
                const int hq = hi + (((lh + 1) & (HH - 1)) - lh) * kLayer;
                best = fminf(best, s_cost[hq] + turn * (0.5f * (cp + s_c[hq])));
            }
            if (open[s] & kBitDown) {
                const int hq = hi + (((lh + HH - 1) & (HH - 1)) - lh) * kLayer;
                best = fminf(best, s_cost[hq] + turn * (0.5f * (cp + s_c[hq])));
            }
            if (best < cur) { s_cost[hi] = best; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        if (it + 1 >= inner_cap) { capped = true; break; }
    }

    // store the lowered states; note the xy neighbour tiles whose halo holds one of them
    const int gi = ti * kT + li, gj = tj * kT + lj;
    bool lowered = false;
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        const float v = s_cost[base + 4 * kLayer * s];
        if (!(v < first[s])) continue;
        st_cost(cost + (((l0 + 4 * s) * L.ny + gj) * L.nx + gi), v);      // (a lowered state is free, hence inside the lattice)
        lowered = true;
    }
    // (translation b is the planner's offset 9 + b, so the tiles form a one-layer tile lattice: no z bits, tnz = 1)
    if (lowered) note_border(s_nbr, li, lj, 0, kT, 0);
    tile_finish(s_nbr, capped, true, tile, ti, tj, 0, tnx, tny, 1, flags_next, stat, raised);
}

// policy[s]: 13 at a goal, the code of the move minimising fl(cost[s'] + w) (ties: the smaller cost[s'], then the smaller code)
// at a free state of finite cost, 255 elsewhere; counts of free and reachable states, the largest finite cost
__global__ void __launch_bounds__(kBlock) pplan_policy_kernel(PLat L, const float* __restrict__ c, const float* __restrict__ cost,
                                                              const unsigned short* __restrict__ moves, float turn,
                                                              unsigned char* __restrict__ policy, unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_cnt[3];
    counts_begin(s_cnt);
    const int nxy = L.nx * L.ny, n = nxy * L.H;
    const float ls[2] = {L.step, sqrtf(2.f) * L.step};
    unsigned nf = 0, nr = 0, mx = 0;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const float cp = c[s], cur = cost[s];
        unsigned char pol = 255;
        if (cp > 0.f) {
            ++nf;
            if (cur < INFINITY) {
                ++nr;
                mx = max(mx, __float_as_uint(cur));
                if (cur == 0.f) pol = 13;
                else {
                    const int i = s % L.nx, j = (s / L.nx) % L.ny, h = s / nxy;
                    unsigned nb = 0;
#pragma unroll
                    for (int b = 0; b < 9; ++b) {
                        const int qi = i + b_dx(b), qj = j + b_dy(b);
                        if (qi >= 0 && qi < L.nx && qj >= 0 && qj < L.ny && c[s + b_dy(b) * L.nx + b_dx(b)] > 0.f) nb |= 1u << b;
                    }
                    const int su = s + (((h + 1) % L.H) - h) * nxy, sd = s + (((h + L.H - 1) % L.H) - h) * nxy;
                    const unsigned open = open_moves(nb, moves[h], c[su] > 0.f, c[sd] > 0.f);
                    float best = INFINITY, bestq = INFINITY;
#pragma unroll
                    for (int b = 0; b < 9; ++b) {
                        if (b == 4) continue;
                        if ((open >> b) & 1u) {
                            const int q = s + b_dy(b) * L.nx + b_dx(b);
                            const float cq = cost[q];
                            const float v = cq + ls[b_nnz(b) - 1] * (0.5f * (cp + c[q]));
                            better_move(v, cq, 9 + b, best, bestq, pol);
                        }
                    }
                    if (open & kBitUp) {
                        const float cq = cost[su];
                        const float v = cq + turn * (0.5f * (cp + c[su]));
                        better_move(v, cq, PosePlanner::kTurnUp, best, bestq, pol);
                    }
                    if (open & kBitDown) {
                        const float cq = cost[sd];
                        const float v = cq + turn * (0.5f * (cp + c[sd]));
                        better_move(v, cq, PosePlanner::kTurnDown, best, bestq, pol);
                    }
                }
            }
        }
        policy[s] = pol;
    }
    commit_counts(s_cnt, nf, nr, mx, stat + kStatFree);
}

// One thread per start follows the policy.  WRITE = false: cnt[t] = states of the path, status, start cost.  WRITE = true: the
// same walk again, the states stored from off[t] on (off = the exclusive scan of cnt).  A start's heading -1 stands for the free
// heading of least cost at its point (ties: the smaller h; none free: status 2, start cost +inf).
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) pplan_walk_kernel(PLat L, const float* __restrict__ c, const float* __restrict__ cost,
                                                            const unsigned char* __restrict__ policy, const float* __restrict__ starts, int m,
                                                            int max_points, long long* __restrict__ off, float* __restrict__ scost,
                                                            unsigned char* __restrict__ status, float* __restrict__ points,
                                                            int* __restrict__ pheading) {
    const PlanLat L2{2, L.nx, L.ny, 1, L.ox, L.oy, 0.f, L.step};
    const int nxy = L.nx * L.ny;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        int q[3];
        long long cnt = 0;
        unsigned char st = 0;
        float sc = NAN;
        if (!snap(L2, starts + (size_t)t * 3, q)) st = 1;
        else {
            int h = (int)starts[(size_t)t * 3 + 2];
            const int p0 = q[1] * L.nx + q[0];
            if (h < 0) {
                float bc = INFINITY;
                for (int hh = 0; hh < L.H; ++hh) {
                    const int s = hh * nxy + p0;
                    if (c[s] > 0.f && (h < 0 || cost[s] < bc)) { h = hh; bc = cost[s]; }
                }
            }
            if (h < 0) { st = 2; sc = INFINITY; }
            else {
                int s = h * nxy + p0;
                sc = cost[s];
                if (!(c[s] > 0.f)) st = 2;
                else if (!(sc < INFINITY)) st = 3;
                else {
                    const long long o = WRITE ? off[t] : 0;
                    float cur = sc;
                    for (;;) {
                        if (WRITE) {
                            points[(size_t)(o + cnt) * 2] = L.ox + (float)q[0] * L.step;
                            points[(size_t)(o + cnt) * 2 + 1] = L.oy + (float)q[1] * L.step;
                            pheading[o + cnt] = h;
                        }
                        ++cnt;
                        const int k = policy[s];
                        if (k == 13) break;
                        if (k == 255 || cnt >= max_points) { st = 4; break; }
                        int qi = q[0], qj = q[1], qh = h;
                        if (k == PosePlanner::kTurnUp) qh = (h + 1) % L.H;
                        else if (k == PosePlanner::kTurnDown) qh = (h + L.H - 1) % L.H;
                        else if (k >= 9 && k < 18) { qi += b_dx(k - 9); qj += b_dy(k - 9); }
                        else { st = 4; break; }
                        if (qi < 0 || qi >= L.nx || qj < 0 || qj >= L.ny) { st = 4; break; }
                        const int sn = (qh * L.ny + qj) * L.nx + qi;
                        const float nxt = cost[sn];
                        if (!(nxt < cur)) { st = 4; break; }
                        s = sn; cur = nxt; q[0] = qi; q[1] = qj; h = qh;
                    }
                }
            }
        }
        if (!WRITE) { off[t] = cnt; scost[t] = sc; status[t] = st; }
    }
}

// The projection, one thread per lattice point: cost2 = the least cost over the headings, heading2 = the first heading that
// attains it (255: cost2 is +inf), c2 = the least c over the free headings (0: none)
__global__ void __launch_bounds__(kBlock) pplan_project_kernel(PLat L, const float* __restrict__ c, const float* __restrict__ cost,
                                                               float* __restrict__ cost2, float* __restrict__ c2,
                                                               unsigned char* __restrict__ heading2) {
    const int nxy = L.nx * L.ny;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nxy; p += gridDim.x * blockDim.x) {
        float best = INFINITY, cb = INFINITY;
        int hb = 255;
        for (int h = 0; h < L.H; ++h) {
            const float v = cost[(size_t)h * nxy + p], cc = c[(size_t)h * nxy + p];
            if (v < best) { best = v; hb = h; }
            if (cc > 0.f && cc < cb) cb = cc;
        }
        cost2[p] = best;
        c2[p] = cb < INFINITY ? cb : 0.f;
        heading2[p] = (unsigned char)hb;
    }
}

// policy2[p]: 13 where cost2 == 0, 255 where it is +inf, else the code 9 .. 17 whose in-lattice neighbour has the least cost2
// (ties: the smaller code); counts of the points with a free heading and of those of finite cost2, the largest finite cost2
__global__ void __launch_bounds__(kBlock) pplan_project_policy_kernel(PLat L, const float* __restrict__ cost2, const float* __restrict__ c2,
                                                                      unsigned char* __restrict__ policy2, unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_cnt[3];
    counts_begin(s_cnt);
    const int nxy = L.nx * L.ny;
    unsigned nf = 0, nr = 0, mx = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nxy; p += gridDim.x * blockDim.x) {
        const float cur = cost2[p];
        unsigned char pol = 255;
        if (c2[p] > 0.f) ++nf;
        if (cur < INFINITY) {
            ++nr;
            mx = max(mx, __float_as_uint(cur));
            if (cur == 0.f) pol = 13;
            else {
                const int i = p % L.nx, j = p / L.nx;
                float bestq = INFINITY;
#pragma unroll
                for (int b = 0; b < 9; ++b) {
                    if (b == 4) continue;
                    const int qi = i + b_dx(b), qj = j + b_dy(b);
                    if (qi < 0 || qi >= L.nx || qj < 0 || qj >= L.ny) continue;
                    const float cq = cost2[p + b_dy(b) * L.nx + b_dx(b)];
                    if (cq < bestq) { bestq = cq; pol = (unsigned char)(9 + b); }
                }
            }
        }
        policy2[p] = pol;
    }
    commit_counts(s_cnt, nf, nr, mx, stat + kStatFree2);
}

}  // namespace

int pplan_check_opts(const PPlanOpts& o, float step) {
    if (!std::isfinite(o.clearance) || !(std::isfinite(o.margin) && o.margin >= 0.f) || !(std::isfinite(o.gain) && o.gain >= 0.f) ||
        !std::isfinite(o.turn))
        return GPIS_ERR_ARG;
    if (o.gain > PosePlanner::kMaxGain || o.max_rounds < 0) return GPIS_ERR_ARG;
    if (!(o.turn > 0.f)) return GPIS_ERR_ARG;
    if (step > 0.f && !(o.turn >= step / 64.f && o.turn <= 1e4f * step)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

PosePlanner::PosePlanner() {
    std::memset(head, 0, sizeof(head)); std::memset(moves, 0, sizeof(moves));
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

PosePlanner::~PosePlanner() { (void)bind(-1); }

int PosePlanner::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_cost, (void*)d_c, (void*)d_policy, (void*)d_flags, (void*)d_stat, (void*)d_head, (void*)d_moves, (void*)d_goals,
                        (void*)d_heading2, (void*)d_starts, (void*)d_off, (void*)d_scost, (void*)d_status, (void*)d_points, (void*)d_pheading})
            (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_cost = d_c = nullptr; d_policy = nullptr; d_flags = nullptr; d_stat = nullptr; d_head = nullptr; d_moves = nullptr; d_goals = nullptr;
    d_heading2 = nullptr; d_starts = nullptr; d_off = nullptr; d_scost = nullptr; d_status = nullptr; d_points = nullptr; d_pheading = nullptr;
    own = nullptr;
    cap_n = cap_tiles = cap_goals = cap_n2 = cap_starts = cap_points = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int PosePlanner::solve(const DistanceField& df, const Footprint& body, const double* headings, const unsigned short* move_bits, int nh,
                       const float* goals, int ngoals, const PPlanOpts& o, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int nx = df.n[0], ny = df.n[1];
    const int tnx = (nx + kTile - 1) / kTile, tny = (ny + kTile - 1) / kTile;
    const long long nxy = (long long)nx * ny, ns = nxy * nh, tiles = (long long)tnx * tny;
    if (!d_stat) GPIS_HIP(hipMalloc((void**)&d_stat, sizeof(unsigned long long) * kStatWords));
    if (!d_head) GPIS_HIP(hipMalloc((void**)&d_head, sizeof(double) * 2 * kMaxH));
    if (!d_moves) GPIS_HIP(hipMalloc((void**)&d_moves, sizeof(unsigned short) * kMaxH));
    if (int rc = grow(d_flags, cap_tiles, (size_t)(2 * tiles))) return rc;
    if ((size_t)ns > cap_n) {
        for (void* p : {(void*)d_cost, (void*)d_c, (void*)d_policy}) (void)hipFree(p);
        d_cost = d_c = nullptr; d_policy = nullptr; cap_n = 0;
        GPIS_HIP(hipMalloc((void**)&d_cost, sizeof(float) * ns));
        GPIS_HIP(hipMalloc((void**)&d_c, sizeof(float) * ns));
        GPIS_HIP(hipMalloc((void**)&d_policy, (size_t)ns));
        cap_n = (size_t)ns;
    }
    if (int rc = grow(d_goals, cap_goals, (size_t)ngoals * 3)) return rc;
    std::memcpy(head, headings, sizeof(double) * 2 * nh);
    std::memcpy(moves, move_bits, sizeof(unsigned short) * nh);
    const PLat L{nx, ny, nh, df.origin[0], df.origin[1], df.step};
    DfLattice DL = df.lattice();
    DL.dim = 2;
    GPIS_HIP(hipMemcpyAsync(d_head, head, sizeof(double) * 2 * nh, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_moves, moves, sizeof(unsigned short) * nh, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_goals, goals, sizeof(float) * (size_t)ngoals * 3, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * kStatWords, s));
    GPIS_HIP(hipMemsetAsync(d_flags, 0, sizeof(int) * (size_t)(2 * tiles), s));
    GPIS_HIP(hipStreamSynchronize(s));
    const auto t1 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(pplan_setup_kernel, dim3((unsigned)((nxy + kBlock - 1) / kBlock), (unsigned)nh), dim3(kBlock), 0, s, (const float*)df.d_dist, DL,
                       BodyArgs{body.d_tab, body.m}, (const double*)d_head, o.clearance, o.margin, o.gain, d_c, d_cost, d_policy);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));              // (the field and the footprint are not read after this point)
    setup_ms = ms_since(t1);
    hipLaunchKernelGGL(pplan_goal_kernel, dim3(grid_for(ngoals)), dim3(kBlock), 0, s, L, (const float*)d_goals, ngoals, (const float*)d_c, d_cost,
                       tnx, d_flags, d_stat);
    GPIS_HIP(hipGetLastError());

    const auto tile_kernel = nh == 8 ? pplan_tile_kernel<8> : nh == 16 ? pplan_tile_kernel<16> : nh == 32 ? pplan_tile_kernel<32>
                                                                                                         : pplan_tile_kernel<64>;
    const long long done = plan_host::run_rounds(
        s, d_flags, tiles, d_stat + kStatRaised, o.max_rounds > 0 ? (long long)o.max_rounds : ns + 1, sched,
        [&](int* cur, int* nxt, unsigned long long* raised) {
            hipLaunchKernelGGL(tile_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, L, (const float*)d_c, d_cost,
                               (const unsigned short*)d_moves, tnx, tny, cur, nxt, o.turn, sched.inner_cap, d_stat, raised);
        });
    if (done < 0) return (int)done;

    hipLaunchKernelGGL(pplan_policy_kernel, dim3(grid_for(ns)), dim3(kBlock), 0, s, L, (const float*)d_c, (const float*)d_cost,
                       (const unsigned short*)d_moves, o.turn, d_policy, d_stat);
    GPIS_HIP(hipGetLastError());
    unsigned long long st[kStatRaised];
    GPIS_HIP(hipMemcpyAsync(st, d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    H = nh; nstates = ns; step = df.step;
    for (int a = 0; a < 2; ++a) { n[a] = df.n[a]; origin[a] = df.origin[a]; }
    cnt = plan_host::counters(st, kStatFree, ngoals, done, ms_since(t0));
    valid = true;
    return GPIS_OK;
}

int PosePlanner::paths(const float* starts, int m, int max_points, hipStream_t s) {
    paths_valid = false;
    const PLat L{n[0], n[1], H, origin[0], origin[1], step};
    const auto walk = [&](auto kernel, float* points, int* pheading) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, L, (const float*)d_c, (const float*)d_cost,
                           (const unsigned char*)d_policy, (const float*)d_starts, m, max_points, d_off, d_scost, d_status, points, pheading);
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
            s, starts, m, 3, d_starts, cap_starts, d_off, d_scost, d_status, npoints, [&] { walk(pplan_walk_kernel<false>, nullptr, nullptr); },
            grow_points, [&] { walk(pplan_walk_kernel<true>, d_points, d_pheading); }))
        return rc;
    npaths = m;
    paths_valid = true;
    return GPIS_OK;
}

int PosePlanner::project(Planner& plan, unsigned char* heading2) {
    const long long nxy = (long long)n[0] * n[1];
    if (int rc = grow(d_heading2, cap_n2, (size_t)nxy)) return rc;
    if (int rc = plan.install_begin(device, n[0], n[1], origin, step)) return rc;
    const PLat L{n[0], n[1], H, origin[0], origin[1], step};
    hipStream_t s = own;
    GPIS_HIP(hipMemsetAsync(d_stat + kStatFree2, 0, sizeof(unsigned long long) * 3, s));
    hipLaunchKernelGGL(pplan_project_kernel, dim3(grid_for(nxy)), dim3(kBlock), 0, s, L, (const float*)d_c, (const float*)d_cost, plan.d_cost,
                       plan.d_c, d_heading2);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(pplan_project_policy_kernel, dim3(grid_for(nxy)), dim3(kBlock), 0, s, L, (const float*)plan.d_cost, (const float*)plan.d_c,
                       plan.d_policy, d_stat);
    GPIS_HIP(hipGetLastError());
    unsigned long long st[kStatRaised];
    GPIS_HIP(hipMemcpyAsync(st, d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
    if (heading2) GPIS_HIP(hipMemcpyAsync(heading2, d_heading2, (size_t)nxy, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    // (the goals kept and the launches are the solve's, still in their words)
    plan.install_end(plan_host::counters(st, kStatFree2, cnt.goals_given, cnt.rounds, cnt.solve_ms));
    return GPIS_OK;
}

}  // namespace gpis
