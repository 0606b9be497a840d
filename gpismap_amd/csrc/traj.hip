// Trajectory smoothing through a distance field (traj.h).
//
// Waypoint i of trajectory t: x[(t N + i) dim + a].  x_0 and x_{N-1} never move; n = N - 2 interior points.  One workgroup of
// 64 ceil(N / 64) threads owns a trajectory, lane i its waypoint i (in the evaluation also the segment i -> i + 1).  x and the
// gradient g live in LDS; an iteration is: sample the field at the own waypoint (4 / 8 corners through L2), g to LDS, the own row
// of inverse(tridiag(-1, 2, -1)) times g accumulated in registers over ascending j with g_j a broadcast LDS read, the largest
// step by a wavefront reduction (a max is exact in any order), the trust region, the update.  Sums of the evaluation use one
// fixed tree over 256 slots.  No floating-point atomics; -ffp-contract=off keeps every product and sum apart.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>
#include "traj.h"
#include "dfield.h"
#include "plan.h"

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
        const float w = (t - s[lo]) / (s[lo + 1] - s[lo]);
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

// One workgroup per trajectory, blockDim.x = 64 ceil(N / 64).  fres[t] = length, smoothness, obstacle cost, min_dist;
// ires[t] = status, iterations, non-finite samples, collides.
template <int DIM>
__global__ void __launch_bounds__(kBlock) traj_opt_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ xin,
                                                          const unsigned char* __restrict__ instat, int N, TrajOpts o,
                                                          float* __restrict__ xout, float* __restrict__ fres,
                                                          int* __restrict__ ires) {
    __shared__ float sx[DIM][kTree];
    __shared__ float sg[DIM][kTree];
    __shared__ float ssum[3][kTree];
    __shared__ float smin[kTree];
    __shared__ int scnt[kTree];
    __shared__ float swave[kBlock / 64];
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
        if (interior) {
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
    if (t < N) {
        float xi[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) { xi[a] = sx[a][t]; xout[base + (size_t)t * DIM + a] = xi[a]; }
        const TrajSample s = traj_sample<DIM>(F, L, xi);
        if (isfinite(s.d)) md = s.d; else ++nf;
        if (interior && s.fin) {
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
        for (void* p : {(void*)d_in, (void*)d_x, (void*)d_instat, (void*)d_fres, (void*)d_ires, (void*)d_arc}) (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_in = d_x = d_fres = d_arc = nullptr; d_instat = nullptr; d_ires = nullptr; own = nullptr;
    cap_x = cap_m = cap_arc = 0;
    has_input = valid = false;
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

int Trajectories::from_paths(const Planner& p, int NN) {
    if (NN < kMinN || NN > kMaxN) return GPIS_ERR_ARG;
    if (!p.valid || !p.paths_valid) return GPIS_ERR_STATE;
    if (p.npaths > kMaxTraj) return GPIS_ERR_LIMIT;
    has_input = valid = false;
    if (int rc = bind(p.device)) return rc;
    const int mm = (int)p.npaths;
    if (int rc = ensure(mm, NN, p.dim)) return rc;
    if (int rc = grow(d_arc, cap_arc, (size_t)std::max(1ll, p.npoints))) return rc;
    hipLaunchKernelGGL(traj_arc_kernel, dim3(grid_for(mm, kBlock, kGridCapTraj)), dim3(kBlock), 0, own, p.d_off, p.d_points, p.d_status, mm,
                       p.dim, d_arc);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(traj_resample_kernel, dim3(grid_for((long long)mm * NN, kBlock, kGridCapTraj)), dim3(kBlock), 0, own, p.d_off,
                       p.d_points, p.d_status, d_arc, mm, NN, p.dim, d_in, d_instat);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(own));
    m = mm; N = NN; dim = p.dim;
    has_input = true;
    return GPIS_OK;
}

int Trajectories::set(const float* x, int mm, int NN, int dd) {
    if (!x || mm < 1 || NN < kMinN || NN > kMaxN || (dd != 2 && dd != 3)) return GPIS_ERR_ARG;
    if (mm > kMaxTraj) return GPIS_ERR_LIMIT;
    has_input = valid = false;
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

int Trajectories::optimize(const DistanceField& df, const TrajOpts& o, hipStream_t s) {
    if (int rc = traj_check_opts(o)) return rc;
    if (!df.valid || !has_input) return GPIS_ERR_STATE;
    if (df.dim != dim) return GPIS_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    valid = false;
    if (int rc = bind(df.device)) return rc;
    const DfLattice L = df.lattice();
    const int threads = 64 * ((N + 63) / 64);
    if (dim == 2)
        hipLaunchKernelGGL(traj_opt_kernel<2>, dim3((unsigned)m), dim3(threads), 0, s, df.d_dist, L, d_in, d_instat, N, o, d_x, d_fres,
                           d_ires);
    else
        hipLaunchKernelGGL(traj_opt_kernel<3>, dim3((unsigned)m), dim3(threads), 0, s, df.d_dist, L, d_in, d_instat, N, o, d_x, d_fres,
                           d_ires);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    opt_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    valid = true;
    return GPIS_OK;
}

}  // namespace gpis
