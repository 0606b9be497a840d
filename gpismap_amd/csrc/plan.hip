// Path planning through a distance field (plan.h).
//
// Lattice point (i, j, k): index p = (k ny + j) nx + i, world point o + (float)i * s (no FMA: -ffp-contract=off).  Direction index
// of the offset (dx, dy, dz): ((dz + 1) 3 + (dy + 1)) 3 + (dx + 1); 13 is "stay".  c[p] = 0 marks a point that is not free (a free
// point has c >= 1), so one array carries the free mask and the point cost.
//
// Solve: the lattice is cut into tiles of 32 x 32 (2-D) or 8 x 8 x 8 (3-D) points, one workgroup of 256 threads per tile and outer
// round.  A workgroup whose flag of this round is down leaves at once.  An active one loads its tile and a one-point halo of cost
// and c into LDS, relaxes its own points in place until an iteration changes nothing (or inner_cap iterations), stores the points
// it lowered, and raises the NEXT round's flag of every neighbour tile that has a lowered point in its halo (and its own at the
// cap).  Values only fall and fl(a + w) is monotone in a, so reading a neighbour's point while its workgroup lowers it is
// harmless: the old value is merely larger, and the flag raised after the store makes the reader run again in the next launch,
// which sees the store.  The host ends the solve after a round that raised no flag.  Integer atomics only (flags, counters).
#include <cmath>
#include "plan.h"
#include "dfield.h"
#include "plan_host.h"

namespace gpis {

namespace {

using namespace plan_dev;

constexpr int kBlock = 256;

constexpr int off_index(int dx, int dy, int dz) { return ((dz + 1) * 3 + (dy + 1)) * 3 + (dx + 1); }
// bits of the points a move along offset k passes: p + every non-empty subset of the offset's non-zero components
constexpr unsigned off_subsets(int k) {
    unsigned m = 0;
    for (int a = 0; a < 8; ++a) {
        const int dx = (a & 1) ? off_dx(k) : 0, dy = (a & 2) ? off_dy(k) : 0, dz = (a & 4) ? off_dz(k) : 0;
        if (dx || dy || dz) m |= 1u << off_index(dx, dy, dz);
    }
    return m;
}
// the moves open at a point whose 27-neighbourhood has the free bits nb (bit 13: the point itself)
__device__ __forceinline__ unsigned open_moves(unsigned nb, int dim, int conn) {
    unsigned m = 0;
    if (!((nb >> 13) & 1u)) return 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        const unsigned need = off_subsets(k);
        if ((nb & need) == need) m |= 1u << k;
    }
    if (dim == 2) m &= 0x1ffu << 9;
    if (!conn) m &= (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);
    return m;
}

// c[p] = point cost (0: not free), cost[p] = +inf, policy[p] = 255
__global__ void __launch_bounds__(kBlock) plan_setup_kernel(const float* __restrict__ dist, int n, float clearance, float margin, float gain,
                                                            float* __restrict__ c, float* __restrict__ cost,
                                                            unsigned char* __restrict__ policy) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        c[p] = point_cost(dist[p], clearance, margin, gain);
        cost[p] = INFINITY;
        policy[p] = 255;
    }
}

// cost = 0 at the kept goals (idempotent: duplicates write the same bits), their tiles active in round 0
__global__ void __launch_bounds__(kBlock) plan_goal_kernel(PlanLat L, const float* __restrict__ goals, int ngoals, const float* __restrict__ c,
                                                           float* __restrict__ cost, int T, int tnx, int tny, int* __restrict__ flags,
                                                           unsigned long long* __restrict__ stat) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngoals; g += gridDim.x * blockDim.x) {
        int q[3];
        if (!snap(L, goals + (size_t)g * L.dim, q)) continue;
        const int p = (q[2] * L.ny + q[1]) * L.nx + q[0];
        if (!(c[p] > 0.f)) continue;
        cost[p] = 0.f;
        const int tk = L.dim == 3 ? q[2] / T : 0;
        flags[(tk * tny + q[1] / T) * tnx + q[0] / T] = 1;
        atomicAdd(&stat[kStatKept], 1ull);
    }
}

template <int DIM>
__global__ void __launch_bounds__(kBlock) plan_tile_kernel(PlanLat L, const float* __restrict__ c, float* cost, int tnx, int tny, int tnz,
                                                           int* flags_cur, int* flags_next, int conn, int inner_cap,
                                                           unsigned long long* stat, unsigned long long* raised) {
    constexpr int T = DIM == 2 ? Planner::kTile2 : Planner::kTile3;
    constexpr int TZ = DIM == 2 ? 1 : T;
    constexpr int H = T + 2, HZ = DIM == 2 ? 1 : T + 2, ZO = DIM == 2 ? 0 : 1;
    constexpr int NH = H * H * HZ, NC = T * T * TZ, CPT = NC / kBlock;
    static_assert(NC % kBlock == 0, "tile points per thread");
    __shared__ float s_cost[NH];
    __shared__ float s_c[NH];
    __shared__ int s_act;
    __shared__ unsigned s_nbr;
    const int tid = threadIdx.x, tile = blockIdx.x;
    if (!tile_begin(flags_cur, tile, s_act, s_nbr)) return;
    const int ti = tile % tnx, tj = (tile / tnx) % tny, tk = tile / (tnx * tny);
    for (int h = tid; h < NH; h += kBlock) {
        const int gi = ti * T + h % H - 1, gj = tj * T + (h / H) % H - 1, gk = DIM == 3 ? tk * T + h / (H * H) - 1 : 0;
        const bool in = gi >= 0 && gi < L.nx && gj >= 0 && gj < L.ny && gk >= 0 && gk < L.nz;
        const int p = in ? (gk * L.ny + gj) * L.nx + gi : 0;
        s_c[h] = in ? c[p] : 0.f;
        s_cost[h] = in ? ld_cost(cost + p) : INFINITY;
    }
    __syncthreads();

    int hh[CPT];
    unsigned moves[CPT];
    float first[CPT];
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        const int q = tid + s * kBlock;
        hh[s] = ((q / (T * T) + ZO) * H + (q / T) % T + 1) * H + q % T + 1;
        unsigned nb = 0;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (DIM == 2 && off_dz(k) != 0) continue;
            if (s_c[hh[s] + (off_dz(k) * H + off_dy(k)) * H + off_dx(k)] > 0.f) nb |= 1u << k;
        }
        moves[s] = open_moves(nb, DIM, conn);
        first[s] = s_cost[hh[s]];
    }
    const float ls[3] = {L.step, sqrtf(2.f) * L.step, sqrtf(3.f) * L.step};
    bool capped = false;
    for (int it = 0;; ++it) {
        int ch = 0;
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
            if (!moves[s]) continue;
            const float cur = s_cost[hh[s]], cp = s_c[hh[s]];
            float best = cur;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                if (k == 13 || (DIM == 2 && off_dz(k) != 0)) continue;
                if ((moves[s] >> k) & 1u) {
                    const int hq = hh[s] + (off_dz(k) * H + off_dy(k)) * H + off_dx(k);
                    const float w = ls[off_nnz(k) - 1] * (0.5f * (cp + s_c[hq]));
                    best = fminf(best, s_cost[hq] + w);
                }
            }
            if (best < cur) { s_cost[hh[s]] = best; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
        if (it + 1 >= inner_cap) { capped = true; break; }
    }

    // store the lowered points; note the neighbour tiles whose halo holds one of them
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        const float v = s_cost[hh[s]];
        if (!(v < first[s])) continue;
        const int q = tid + s * kBlock;
        const int li = q % T, lj = (q / T) % T, lk = q / (T * T);
        const int gi = ti * T + li, gj = tj * T + lj, gk = DIM == 3 ? tk * T + lk : 0;
        st_cost(cost + ((gk * L.ny + gj) * L.nx + gi), v);      // (a lowered point is free, hence inside the lattice)
        note_border(s_nbr, li, lj, lk, T, DIM == 2 ? 0 : T);
    }
    tile_finish(s_nbr, capped, conn != 0, tile, ti, tj, tk, tnx, tny, tnz, flags_next, stat, raised);
}

// policy[p]: 13 at a goal, the direction of the move minimising fl(cost[q] + w) (ties: the smaller cost[q], then the smaller
// index) at a free point of finite cost, 255 elsewhere; counts of free and reachable points, the largest finite cost
__global__ void __launch_bounds__(kBlock) plan_policy_kernel(PlanLat L, const float* __restrict__ c, const float* __restrict__ cost, int conn,
                                                             unsigned char* __restrict__ policy, unsigned long long* __restrict__ stat) {
    __shared__ unsigned s_cnt[3];
    counts_begin(s_cnt);
    const int nxy = L.nx * L.ny, n = nxy * L.nz;
    const float ls[3] = {L.step, sqrtf(2.f) * L.step, sqrtf(3.f) * L.step};
    unsigned nf = 0, nr = 0, mx = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const float cp = c[p], cur = cost[p];
        unsigned char pol = 255;
        if (cp > 0.f) {
            ++nf;
            if (cur < INFINITY) {
                ++nr;
                mx = max(mx, __float_as_uint(cur));
                if (cur == 0.f) pol = 13;
                else {
                    const int i = p % L.nx, j = (p / L.nx) % L.ny, kz = p / nxy;
                    unsigned nb = 0;
#pragma unroll
                    for (int k = 0; k < 27; ++k) {
                        const int qi = i + off_dx(k), qj = j + off_dy(k), qk = kz + off_dz(k);
                        if (qi >= 0 && qi < L.nx && qj >= 0 && qj < L.ny && qk >= 0 && qk < L.nz &&
                            c[p + (off_dz(k) * L.ny + off_dy(k)) * L.nx + off_dx(k)] > 0.f)
                            nb |= 1u << k;
                    }
                    const unsigned moves = open_moves(nb, L.dim, conn);
                    float best = INFINITY, bestq = INFINITY;
#pragma unroll
                    for (int k = 0; k < 27; ++k) {
                        if (k == 13) continue;
                        if ((moves >> k) & 1u) {
                            const int q = p + (off_dz(k) * L.ny + off_dy(k)) * L.nx + off_dx(k);
                            const float cq = cost[q];
                            const float v = cq + ls[off_nnz(k) - 1] * (0.5f * (cp + c[q]));
                            better_move(v, cq, k, best, bestq, pol);
                        }
                    }
                }
            }
        }
        policy[p] = pol;
    }
    commit_counts(s_cnt, nf, nr, mx, stat + kStatFree);
}

// One thread per start follows the policy.  WRITE = false: cnt[t] = points of the path, status, start cost.  WRITE = true: the
// same walk again, the points stored from off[t] on (off = the exclusive scan of cnt).
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) plan_walk_kernel(PlanLat L, const float* __restrict__ c, const float* __restrict__ cost,
                                                           const unsigned char* __restrict__ policy, const float* __restrict__ starts, int m,
                                                           int max_points, long long* __restrict__ off, float* __restrict__ scost,
                                                           unsigned char* __restrict__ status, float* __restrict__ points) {
    const float o[3] = {L.ox, L.oy, L.oz};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        int q[3];
        long long cnt = 0;
        unsigned char st = 0;
        float sc = NAN;
        if (!snap(L, starts + (size_t)t * L.dim, q)) st = 1;
        else {
            int p = (q[2] * L.ny + q[1]) * L.nx + q[0];
            sc = cost[p];
            if (!(c[p] > 0.f)) st = 2;
            else if (!(sc < INFINITY)) st = 3;
            else {
                float* out = WRITE ? points + (size_t)off[t] * L.dim : nullptr;
                float cur = sc;
                for (;;) {
                    if (WRITE) {
#pragma unroll
                        for (int a = 0; a < 3; ++a)
                            if (a < L.dim) out[(size_t)cnt * L.dim + a] = o[a] + (float)q[a] * L.step;
                    }
                    ++cnt;
                    const int k = policy[p];
                    if (k == 13) break;
                    if (k > 26 || cnt >= max_points) { st = 4; break; }
                    const int qi = q[0] + off_dx(k), qj = q[1] + off_dy(k), qk = q[2] + off_dz(k);
                    if (qi < 0 || qi >= L.nx || qj < 0 || qj >= L.ny || qk < 0 || qk >= L.nz) { st = 4; break; }
                    const int pn = (qk * L.ny + qj) * L.nx + qi;
                    const float nxt = cost[pn];
                    if (!(nxt < cur)) { st = 4; break; }
                    p = pn; cur = nxt; q[0] = qi; q[1] = qj; q[2] = qk;
                }
            }
        }
        if (!WRITE) { off[t] = cnt; scost[t] = sc; status[t] = st; }
    }
}

}  // namespace

int plan_check_opts(const PlanOpts& o) {
    if (!std::isfinite(o.clearance) || !(std::isfinite(o.margin) && o.margin >= 0.f) || !(std::isfinite(o.gain) && o.gain >= 0.f))
        return GPIS_ERR_ARG;
    if (o.gain > Planner::kMaxGain || (o.connectivity != 0 && o.connectivity != 1) || o.max_rounds < 0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

Planner::Planner() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Planner::~Planner() { (void)bind(-1); }

int Planner::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_cost, (void*)d_c, (void*)d_policy, (void*)d_flags, (void*)d_stat, (void*)d_goals, (void*)d_starts,
                        (void*)d_off, (void*)d_scost, (void*)d_status, (void*)d_points})
            (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_cost = d_c = nullptr; d_policy = nullptr; d_flags = nullptr; d_stat = nullptr; d_goals = d_starts = nullptr; d_off = nullptr;
    d_scost = nullptr; d_status = nullptr; d_points = nullptr; own = nullptr;
    cap_n = cap_tiles = cap_goals = cap_starts = cap_points = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int Planner::ensure(long long np, long long tiles) {
    if (!d_stat) GPIS_HIP(hipMalloc((void**)&d_stat, sizeof(unsigned long long) * kStatWords));
    if (int rc = grow(d_flags, cap_tiles, (size_t)(2 * tiles))) return rc;
    if ((size_t)np <= cap_n) return GPIS_OK;
    for (void* p : {(void*)d_cost, (void*)d_c, (void*)d_policy}) (void)hipFree(p);
    d_cost = d_c = nullptr; d_policy = nullptr; cap_n = 0;
    GPIS_HIP(hipMalloc((void**)&d_cost, sizeof(float) * np));
    GPIS_HIP(hipMalloc((void**)&d_c, sizeof(float) * np));
    GPIS_HIP(hipMalloc((void**)&d_policy, (size_t)np));
    cap_n = (size_t)np;
    return GPIS_OK;
}

int Planner::solve(const DistanceField& df, const float* goals, int ngoals, const PlanOpts& o, hipStream_t s) {
    if (!df.valid) return GPIS_ERR_STATE;
    if (!goals || ngoals < 1) return GPIS_ERR_ARG;
    if (int rc = plan_check_opts(o)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int dm = df.dim, T = dm == 2 ? kTile2 : kTile3;
    const int nx = df.n[0], ny = df.n[1], nz = dm == 3 ? df.n[2] : 1;
    const int tnx = (nx + T - 1) / T, tny = (ny + T - 1) / T, tnz = dm == 3 ? (nz + T - 1) / T : 1;
    const long long np = df.ngrid, tiles = (long long)tnx * tny * tnz;
    if (int rc = ensure(np, tiles)) return rc;
    if (int rc = grow(d_goals, cap_goals, (size_t)ngoals * dm)) return rc;
    const PlanLat L{dm, nx, ny, nz, df.origin[0], df.origin[1], dm == 3 ? df.origin[2] : 0.f, df.step};
    GPIS_HIP(hipMemcpyAsync(d_goals, goals, sizeof(float) * (size_t)ngoals * dm, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_stat, 0, sizeof(unsigned long long) * kStatWords, s));
    GPIS_HIP(hipMemsetAsync(d_flags, 0, sizeof(int) * (size_t)(2 * tiles), s));
    hipLaunchKernelGGL(plan_setup_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, df.d_dist, (int)np, o.clearance, o.margin, o.gain, d_c,
                       d_cost, d_policy);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(plan_goal_kernel, dim3(grid_for(ngoals)), dim3(kBlock), 0, s, L, d_goals, ngoals, d_c, d_cost, T, tnx, tny, d_flags,
                       d_stat);
    GPIS_HIP(hipGetLastError());

    const auto tile_kernel = dm == 2 ? plan_tile_kernel<2> : plan_tile_kernel<3>;
    const long long done = plan_host::run_rounds(
        s, d_flags, tiles, d_stat + kStatRaised, o.max_rounds > 0 ? (long long)o.max_rounds : np + 1, sched,
        [&](int* cur, int* nxt, unsigned long long* raised) {
            hipLaunchKernelGGL(tile_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, L, d_c, d_cost, tnx, tny, tnz, cur, nxt,
                               o.connectivity, sched.inner_cap, d_stat, raised);
        });
    if (done < 0) return (int)done;

    hipLaunchKernelGGL(plan_policy_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, L, d_c, d_cost, o.connectivity, d_policy, d_stat);
    GPIS_HIP(hipGetLastError());
    unsigned long long st[kStatRaised];
    GPIS_HIP(hipMemcpyAsync(st, d_stat, sizeof(st), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    dim = dm; ngrid = np; step = df.step;
    for (int a = 0; a < 3; ++a) { n[a] = a < dm ? df.n[a] : 1; origin[a] = a < dm ? df.origin[a] : 0.f; }
    cnt = plan_host::counters(st, kStatFree, ngoals, done, ms_since(t0));
    valid = true;
    return GPIS_OK;
}

int Planner::install_begin(int dev, int nx, int ny, const float* origin2, float lattice_step) {
    if (int rc = bind(dev)) return rc;
    clear_result();
    const long long np = (long long)nx * ny;
    if (int rc = ensure(np, (long long)((nx + kTile2 - 1) / kTile2) * ((ny + kTile2 - 1) / kTile2))) return rc;
    dim = 2; ngrid = np; step = lattice_step;
    n[0] = nx; n[1] = ny; n[2] = 1;
    origin[0] = origin2[0]; origin[1] = origin2[1]; origin[2] = 0.f;
    return GPIS_OK;
}

int Planner::paths(const float* starts, int m, int max_points, hipStream_t s) {
    if (!starts || m < 1 || max_points < 2) return GPIS_ERR_ARG;
    if (!valid) return GPIS_ERR_STATE;
    if (m > kMaxStarts) return GPIS_ERR_LIMIT;
    paths_valid = false;
    const PlanLat L{dim, n[0], n[1], n[2], origin[0], origin[1], origin[2], step};
    const auto walk = [&](auto kernel, float* points) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, L, d_c, d_cost, d_policy, d_starts, m, max_points, d_off, d_scost,
                           d_status, points);
    };
    if (int rc = plan_host::run_paths(
            s, starts, m, dim, d_starts, cap_starts, d_off, d_scost, d_status, npoints, [&] { walk(plan_walk_kernel<false>, nullptr); },
            [&](size_t total) { return grow(d_points, cap_points, total * dim); }, [&] { walk(plan_walk_kernel<true>, d_points); }))
        return rc;
    npaths = m;
    paths_valid = true;
    return GPIS_OK;
}

}  // namespace gpis
