// The particle filter on the device (pf.h; the contract: tests/pf_ref.py).  Per step: predict (one thread per
// particle: three / six Philox blocks, the motion in the body frame, the state and the float32 pose written), then update: the
// tracker's set-up, the scorer's launch (locate.h), L += beta cost with block minima, their minimum, q = floor(exp(-(L - Lmin))
// 2^32) with block totals (integers: any order gives the same bits) and the block's best (max q, lowest index), their totals,
// the estimate's terms through the tracker's tree (256-point segments, the partials padded to a power of two), one copy of
// PfStats back.  The host divides, normalises and decides; the resampling is a uint64 scan in separate launches (block scan,
// scan of the block sums, add), then one thread per output slot: a binary search in the prefix sums and the gather into the
// other half of the ping-pong buffers.  No kernel waits on another workgroup; no floating-point atomics; every double
// expression is written left to right as the reference states it (-ffp-contract=off).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include "dfield.h"
#include "locate.h"
#include "pf.h"
#include "block_ops.h"
#include "philox.h"

namespace gpis {

namespace {

typedef unsigned long long u64;
constexpr int kBlock = ParticleFilter::kBlock;
constexpr double kTwo32 = 4294967296.0;
constexpr u64 kIdxMask = (1ull << 24) - 1;

// ---- the generator (philox.h) -----------------------------------------------------------------------------------------------
// deviate k of a slot at a tick: tag 0
__device__ __forceinline__ double deviate(uint32_t slot, uint32_t tick, uint32_t k, uint32_t k0, uint32_t k1) {
    return philox_deviate(slot, tick, k, 0u, k0, k1);
}

// ---- state and pose ---------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void quat_to_mat(const double* __restrict__ q, double* __restrict__ R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y + w * z);       R[2] = 2.0 * (x * z - w * y);
    R[3] = 2.0 * (x * y - w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z + w * x);
    R[6] = 2.0 * (x * z + w * y);       R[7] = 2.0 * (y * z - w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// the float32 pose of a state: every component cast from the double
template <int D>
__host__ __device__ __forceinline__ void pose_of_state(const double* __restrict__ st, float* __restrict__ P) {
    if constexpr (D == 2) {
        P[0] = (float)st[0]; P[1] = (float)st[1]; P[2] = (float)st[2]; P[3] = (float)st[3]; P[4] = (float)(-st[3]); P[5] = (float)st[2];
    } else {
        double R[9];
        quat_to_mat(st + 3, R);
#pragma unroll
        for (int a = 0; a < 3; ++a) P[a] = (float)st[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) P[3 + a] = (float)R[a];
    }
}

__device__ __forceinline__ void qmul(const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ o) {
    o[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
    o[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
    o[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
    o[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

struct PfMotion {
    double d[3];       // the translation of the relative pose, body frame
    double q[4];       // its rotation: 2-D (cu, su), 3-D the quaternion
    double st[3];      // sigma_t
    double half_r;     // 0.5 * sigma_r
};

template <int D>
__global__ void __launch_bounds__(kBlock) pf_predict_kernel(double* __restrict__ state, float* __restrict__ pose, int m, uint32_t tick,
                                                            uint32_t k0, uint32_t k1, PfMotion mo) {
    constexpr int NS = D == 3 ? 7 : 4, NP = D == 3 ? 12 : 6;
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= m) return;
    double* __restrict__ S = state + (size_t)i * NS;
    double st[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) st[a] = S[a];
    if constexpr (D == 2) {
        const double z0 = deviate(i, tick, 0, k0, k1), z1 = deviate(i, tick, 1, k0, k1), z2 = deviate(i, tick, 2, k0, k1);
        const double bx = mo.d[0] + mo.st[0] * z0, by = mo.d[1] + mo.st[1] * z1;
        const double a = mo.half_r * z2;
        const double den = 1.0 + a * a;
        const double cn = (1.0 - a * a) / den, sn = (a + a) / den;
        const double c = st[2], s = st[3];
        st[0] = st[0] + (c * bx - s * by);
        st[1] = st[1] + (s * bx + c * by);
        const double c1 = c * mo.q[0] - s * mo.q[1], s1 = c * mo.q[1] + s * mo.q[0];
        const double c2 = c1 * cn - s1 * sn, s2 = c1 * sn + s1 * cn;
        const double n = sqrt(c2 * c2 + s2 * s2);
        st[2] = c2 / n; st[3] = s2 / n;
    } else {
        double b[3], A[4], R[9], Q1[4], Q2[4];
#pragma unroll
        for (int a = 0; a < 3; ++a) b[a] = mo.d[a] + mo.st[a] * deviate(i, tick, a, k0, k1);
        A[0] = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) A[1 + a] = mo.half_r * deviate(i, tick, 3 + a, k0, k1);
        quat_to_mat(st + 3, R);
#pragma unroll
        for (int a = 0; a < 3; ++a) st[a] = st[a] + (R[a] * b[0] + R[3 + a] * b[1] + R[6 + a] * b[2]);
        qmul(st + 3, mo.q, Q1);
        qmul(Q1, A, Q2);
        const double n = sqrt(Q2[0] * Q2[0] + Q2[1] * Q2[1] + Q2[2] * Q2[2] + Q2[3] * Q2[3]);
#pragma unroll
        for (int a = 0; a < 4; ++a) st[3 + a] = Q2[a] / n;
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) S[a] = st[a];
    float P[NP];
    pose_of_state<D>(st, P);
#pragma unroll
    for (int a = 0; a < NP; ++a) pose[(size_t)i * NP + a] = P[a];
}

// after init: uniform weights, no cost yet, every particle its own ancestor
__global__ void __launch_bounds__(kBlock) pf_fill_kernel(int m, double* __restrict__ L, u64* __restrict__ q, double* __restrict__ cost,
                                                         int* __restrict__ inl, int* __restrict__ anc) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= m) return;
    L[i] = 0.0; q[i] = 1ull << 32; cost[i] = 0.0; inl[i] = 0; anc[i] = i;
}

// ---- block reductions (block_ops.h: block_reduce) of order-free operations only: min of doubles without NaN, integer sums
// and maxima ------------------------------------------------------------------------------------------------------------------
// L += beta cost and the block's minimum of the new L
__global__ void __launch_bounds__(kBlock) pf_accum_kernel(double* __restrict__ L, const double* __restrict__ cost, int m, double beta,
                                                          double* __restrict__ bmin) {
    __shared__ double sh[kBlock / kWave];
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    double v = INFINITY;
    if (i < m) {
        v = L[i] + beta * cost[i];
        L[i] = v;
    }
    v = block_reduce(v, OpMin(), sh, kBlock, (double)INFINITY);
    if (threadIdx.x == 0) bmin[blockIdx.x] = v;
}

__global__ void __launch_bounds__(1024) pf_min_top_kernel(const double* __restrict__ bmin, int nb, PfStats* __restrict__ st) {
    __shared__ double sh[1024 / kWave];
    double v = INFINITY;
    for (int b = threadIdx.x; b < nb; b += 1024) v = OpMin()(v, bmin[b]);
    v = block_reduce(v, OpMin(), sh, 1024, (double)INFINITY);
    if (threadIdx.x == 0) st->lmin = v;
}

// q = floor(exp(-(L - Lmin)) 2^32) and the block's integer totals and best key
__global__ void __launch_bounds__(kBlock) pf_weigh_kernel(const double* __restrict__ L, int m, int nb, const PfStats* __restrict__ st,
                                                          u64* __restrict__ q, u64* __restrict__ bsum, u64* __restrict__ bkey) {
    __shared__ u64 sh[kBlock / kWave];
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    u64 v = 0, key = 0;
    if (i < m) {
        const double w = exp(-(L[i] - st->lmin));
        v = (u64)floor(w * kTwo32);
        q[i] = v;
        key = (v << 24) | (kIdxMask - (u64)i);
    }
    const u64 h = v >> 16;
    const u64 t = block_reduce(v, OpAdd(), sh, kBlock, 0ull);
    const u64 th = block_reduce(h, OpAdd(), sh, kBlock, 0ull);
    const u64 s2 = block_reduce(h * h, OpAdd(), sh, kBlock, 0ull);
    const u64 kb = block_reduce(key, OpMax(), sh, kBlock, 0ull);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = t; bsum[(size_t)nb + blockIdx.x] = th; bsum[2 * (size_t)nb + blockIdx.x] = s2;
        bkey[blockIdx.x] = kb;
    }
}

__global__ void __launch_bounds__(1024) pf_totals_top_kernel(const u64* __restrict__ bsum, const u64* __restrict__ bkey, int nb,
                                                             PfStats* __restrict__ st) {
    __shared__ u64 sh[1024 / kWave];
    u64 t = 0, th = 0, s2 = 0, key = 0;
    for (int b = threadIdx.x; b < nb; b += 1024) {
        t += bsum[b]; th += bsum[(size_t)nb + b]; s2 += bsum[2 * (size_t)nb + b];
        key = OpMax()(key, bkey[b]);
    }
    t = block_reduce(t, OpAdd(), sh, 1024, 0ull);
    th = block_reduce(th, OpAdd(), sh, 1024, 0ull);
    s2 = block_reduce(s2, OpAdd(), sh, 1024, 0ull);
    key = block_reduce(key, OpMax(), sh, 1024, 0ull);
    if (threadIdx.x == 0) {
        st->T = t; st->Th = th; st->S2 = s2;
        st->qmax = key >> 24;
        st->best = (int)(kIdxMask - (key & kIdxMask));
        st->pad = 0;
    }
}

// ---- the estimate: the tracker's tree (block_ops.h: segment_reduce and tree_top state the order) ---------------------------
// the terms (double)q * state column (3-D: the quaternion times +-1 towards the best particle's) and their sum per segment
template <int D>
__global__ void __launch_bounds__(kBlock) pf_est_terms_kernel(const double* __restrict__ state, const u64* __restrict__ q, int m,
                                                              int nseg_pow2, const PfStats* __restrict__ st, double* __restrict__ part) {
    constexpr int NS = D == 3 ? 7 : 4;
    __shared__ double sh[NS][kBlock / 2];
    const int tid = threadIdx.x;
    double Q0[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (D == 3) {
        const int best = min(max(st->best, 0), m - 1);     // (totals_top wrote an index below m; bounded whatever it holds)
#pragma unroll
        for (int a = 0; a < 4; ++a) Q0[a] = state[(size_t)best * NS + 3 + a];
    }
    for (int seg = blockIdx.x; seg < nseg_pow2; seg += gridDim.x) {
        const int j = seg * kBlock + tid;
        double a[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) a[c] = 0.0;
        if (j < m) {
            const double w = (double)q[j];
            const double* __restrict__ S = state + (size_t)j * NS;
            if constexpr (D == 2) {
#pragma unroll
                for (int c = 0; c < NS; ++c) a[c] = w * S[c];
            } else {
                const double dot = S[3] * Q0[0] + S[4] * Q0[1] + S[5] * Q0[2] + S[6] * Q0[3];
                const double sg = dot >= 0.0 ? 1.0 : -1.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = w * S[c];
#pragma unroll
                for (int c = 3; c < NS; ++c) a[c] = w * (S[c] * sg);
            }
        }
        segment_reduce<NS, kBlock>(a, sh, tid, seg, nseg_pow2, part);
    }
}

// the segment partials of every sum reduced by the same halving tree (tree_top; P a power of two, in place); one block
__global__ void __launch_bounds__(1024) pf_est_top_kernel(int ns, int P, double* __restrict__ part, PfStats* __restrict__ st) {
    tree_top(ns, P, part);
    if ((int)threadIdx.x < ns) st->sums[threadIdx.x] = part[(size_t)threadIdx.x * P];
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------
// out[i] = the inclusive sum of in[] within the block of 256; sums[block] = the block's total.  in == out is allowed (a thread
// reads its own element, then writes it).  A one-shot scan with one barrier: block_ops.h's block_incl_scan, made for loops, pays
// a second barrier and 10 more VGPRs here and measured slower.
__global__ void __launch_bounds__(kBlock) pf_scan_block_kernel(const u64* in, u64* out, int n, u64* __restrict__ sums) {
    __shared__ u64 sh[kBlock / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int i = (int)(blockIdx.x * kBlock + tid);
    u64 v = i < n ? in[i] : 0ull;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const u64 t = __shfl_up(v, d, kWave);
        if (lane >= d) v += t;
    }
    if (lane == kWave - 1) sh[wv] = v;
    __syncthreads();
    u64 off = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave - 1; ++w) off += w < wv ? sh[w] : 0ull;
    v += off;
    if (i < n) out[i] = v;
    if (tid == kBlock - 1) sums[blockIdx.x] = v;
}

// out[i] += scanned[block - 1] for every block after the first
__global__ void __launch_bounds__(kBlock) pf_scan_add_kernel(u64* __restrict__ out, int n, const u64* __restrict__ scanned) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (blockIdx.x == 0 || i >= n) return;
    out[i] += scanned[blockIdx.x - 1];
}

// ---- the resampling -----------------------------------------------------------------------------------------------------------
// output slot j: p = j qs + (j rem) div m + r; its ancestor is the first i with C[i] > p (p < T = C[m - 1], so there is one;
// the search is bounded to m - 1 whatever C holds); state and pose gathered from the other half; L = 0
template <int D>
__global__ void __launch_bounds__(kBlock) pf_resample_kernel(const u64* __restrict__ C, int m, u64 qs, u64 rem, u64 r,
                                                             const double* __restrict__ s_in, const float* __restrict__ p_in,
                                                             double* __restrict__ s_out, float* __restrict__ p_out,
                                                             double* __restrict__ L, int* __restrict__ anc) {
    constexpr int NS = D == 3 ? 7 : 4, NP = D == 3 ? 12 : 6;
    const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (j >= m) return;
    const u64 p = (u64)j * qs + ((u64)j * rem) / (u64)m + r;
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (C[mid] > p) hi = mid;
        else lo = mid + 1;
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) s_out[(size_t)j * NS + a] = s_in[(size_t)lo * NS + a];
#pragma unroll
    for (int a = 0; a < NP; ++a) p_out[(size_t)j * NP + a] = p_in[(size_t)lo * NP + a];
    L[j] = 0.0;
    anc[j] = lo;
}

// blocks of kBlock that cover n elements, uncapped: it sizes buffers and scan levels as well as launches
int blocks_of(long long n) { return (int)((n + kBlock - 1) / kBlock); }

}  // namespace

// ---- host -------------------------------------------------------------------------------------------------------------------
int pf_check_opts(const PfOpts& o) {
    auto ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
    if (!ok(o.max_residual) || !ok(o.beta) || !ok(o.sigma_t[0]) || !ok(o.sigma_t[1]) || !ok(o.sigma_t[2]) || !ok(o.sigma_r) ||
        !ok(o.resample_below) || o.stride < 1)
        return GPIS_ERR_ARG;
    return GPIS_OK;
}

void pf_mat_to_quat(const double* R, double* q) {
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        const double s = std::sqrt(tr + 1.0) * 2.0;
        q[0] = 0.25 * s; q[1] = (R[5] - R[7]) / s; q[2] = (R[6] - R[2]) / s; q[3] = (R[1] - R[3]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        q[0] = (R[5] - R[7]) / s; q[1] = 0.25 * s; q[2] = (R[3] + R[1]) / s; q[3] = (R[6] + R[2]) / s;
    } else if (R[4] > R[8]) {
        const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        q[0] = (R[6] - R[2]) / s; q[1] = (R[3] + R[1]) / s; q[2] = 0.25 * s; q[3] = (R[7] + R[5]) / s;
    } else {
        const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        q[0] = (R[1] - R[3]) / s; q[1] = (R[6] + R[2]) / s; q[2] = (R[7] + R[5]) / s; q[3] = 0.25 * s;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int a = 0; a < 4; ++a) q[a] = q[a] / n;
}

void pf_quat_to_mat(const double* q, double* R) { quat_to_mat(q, R); }

void pf_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    philox10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

ParticleFilter::ParticleFilter() { (void)hipGetDevice(&device); }

ParticleFilter::~ParticleFilter() { (void)bind(-1); }

int ParticleFilter::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (trk.own) (void)hipStreamSynchronize(trk.own);
        for (void* p : {(void*)d_state[0], (void*)d_state[1], (void*)d_pose[0], (void*)d_pose[1], (void*)d_L, (void*)d_q, (void*)d_C,
                        (void*)d_cost, (void*)d_inl, (void*)d_anc, (void*)d_bmin, (void*)d_bsum, (void*)d_bkey, (void*)d_s1, (void*)d_s2,
                        (void*)d_part, (void*)d_stats})
            (void)hipFree(p);
        if (h_stats) (void)hipHostFree(h_stats);
        if (h_stage) (void)hipHostFree(h_stage);
    }
    d_state[0] = d_state[1] = nullptr; d_pose[0] = d_pose[1] = nullptr; d_L = nullptr; d_q = d_C = nullptr; d_cost = nullptr;
    d_inl = d_anc = nullptr; d_bmin = nullptr; d_bsum = d_bkey = d_s1 = d_s2 = nullptr; d_part = nullptr; d_stats = nullptr;
    h_stats = nullptr; h_stage = nullptr; cap_m = 0;
    inited = have_estimate = false; dim = 0; m = 0;
    device = dev;
    return trk.bind(dev);
}

int ParticleFilter::ensure(long long mm) {
    if (!d_stats) GPIS_HIP(hipMalloc((void**)&d_stats, sizeof(PfStats)));
    if (!h_stats) GPIS_HIP(hipHostMalloc((void**)&h_stats, sizeof(PfStats)));
    if (!d_s2) GPIS_HIP(hipMalloc((void**)&d_s2, sizeof(u64) * 257));
    if ((size_t)mm <= cap_m) return GPIS_OK;
    for (void* p : {(void*)d_state[0], (void*)d_state[1], (void*)d_pose[0], (void*)d_pose[1], (void*)d_L, (void*)d_q, (void*)d_C,
                    (void*)d_cost, (void*)d_inl, (void*)d_anc, (void*)d_bmin, (void*)d_bsum, (void*)d_bkey, (void*)d_s1, (void*)d_part})
        (void)hipFree(p);
    if (h_stage) (void)hipHostFree(h_stage);
    d_state[0] = d_state[1] = nullptr; d_pose[0] = d_pose[1] = nullptr; d_L = nullptr; d_q = d_C = nullptr; d_cost = nullptr;
    d_inl = d_anc = nullptr; d_bmin = nullptr; d_bsum = d_bkey = d_s1 = nullptr; d_part = nullptr; h_stage = nullptr; cap_m = 0;
    const size_t n = (size_t)mm, nb = (size_t)blocks_of(mm), P = (size_t)pow2_at_least((long long)nb);
    for (int k = 0; k < 2; ++k) {
        GPIS_HIP(hipMalloc((void**)&d_state[k], sizeof(double) * 7 * n));
        GPIS_HIP(hipMalloc((void**)&d_pose[k], sizeof(float) * 12 * n));
    }
    GPIS_HIP(hipMalloc((void**)&d_L, sizeof(double) * n));
    GPIS_HIP(hipMalloc((void**)&d_q, sizeof(u64) * n));
    GPIS_HIP(hipMalloc((void**)&d_C, sizeof(u64) * n));
    GPIS_HIP(hipMalloc((void**)&d_cost, sizeof(double) * n));
    GPIS_HIP(hipMalloc((void**)&d_inl, sizeof(int) * n));
    GPIS_HIP(hipMalloc((void**)&d_anc, sizeof(int) * n));
    GPIS_HIP(hipMalloc((void**)&d_bmin, sizeof(double) * nb));
    GPIS_HIP(hipMalloc((void**)&d_bsum, sizeof(u64) * 3 * nb));
    GPIS_HIP(hipMalloc((void**)&d_bkey, sizeof(u64) * nb));
    GPIS_HIP(hipMalloc((void**)&d_s1, sizeof(u64) * nb));
    GPIS_HIP(hipMalloc((void**)&d_part, sizeof(double) * 7 * P));
    GPIS_HIP(hipHostMalloc((void**)&h_stage, (sizeof(double) * 7 + sizeof(float) * 12) * n));
    cap_m = n;
    return GPIS_OK;
}

int ParticleFilter::init(int dm, const float* poses, long long mm, uint64_t sd) {
    int dev = -1;
    GPIS_HIP(hipGetDevice(&dev));
    if (int rc = bind(dev)) return rc;
    if (!trk.own) return GPIS_ERR_HIP;
    inited = have_estimate = false;
    if (int rc = ensure(mm)) return rc;
    const int ns = dm == 3 ? 7 : 4, np = dm == 3 ? 12 : 6;
    const size_t n = (size_t)mm;
    double* hs = (double*)h_stage;
    float* hp = (float*)(h_stage + sizeof(double) * 7 * n);
    for (size_t i = 0; i < n; ++i) {
        const float* P = poses + i * np;
        double* S = hs + i * ns;
        if (dm == 2) {
            for (int a = 0; a < 4; ++a) S[a] = (double)P[a];
            pose_of_state<2>(S, hp + i * np);
        } else {
            double R[9];
            for (int a = 0; a < 3; ++a) S[a] = (double)P[a];
            for (int a = 0; a < 9; ++a) R[a] = (double)P[3 + a];
            pf_mat_to_quat(R, S + 3);
            pose_of_state<3>(S, hp + i * np);
        }
    }
    hipStream_t s = trk.own;
    GPIS_HIP(hipMemcpyAsync(d_state[0], hs, sizeof(double) * ns * n, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemcpyAsync(d_pose[0], hp, sizeof(float) * np * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pf_fill_kernel, dim3(blocks_of(mm)), dim3(kBlock), 0, s, (int)mm, d_L, d_q, d_cost, d_inl, d_anc);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    dim = dm; m = mm; cur = 0; tick = 0; seed = sd;
    npoints = pixels = updates = resamples = 0; resampled = false; neff = (double)mm; ms = 0.0;
    stats = PfStats{};
    stats.T = (u64)mm << 32; stats.Th = (u64)mm << 16; stats.S2 = (u64)mm << 32; stats.qmax = 1ull << 32;
    inited = true;
    return GPIS_OK;
}

int ParticleFilter::predict(const double* motion, const PfOpts& o, hipStream_t s) {
    PfMotion mo{};
    for (int a = 0; a < dim; ++a) { mo.d[a] = motion[a]; mo.st[a] = o.sigma_t[a]; }
    for (int a = 0; a < (dim == 3 ? 4 : 2); ++a) mo.q[a] = motion[dim + a];
    mo.half_r = 0.5 * o.sigma_r;
    tick += 1;
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
    if (dim == 3)
        hipLaunchKernelGGL(pf_predict_kernel<3>, dim3(blocks_of(m)), dim3(kBlock), 0, s, d_state[cur], d_pose[cur], (int)m, tick, k0, k1, mo);
    else
        hipLaunchKernelGGL(pf_predict_kernel<2>, dim3(blocks_of(m)), dim3(kBlock), 0, s, d_state[cur], d_pose[cur], (int)m, tick, k0, k1, mo);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}

int ParticleFilter::update(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n,
                           const PfOpts& o, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    // the tracker's set-up reads the stride alone; the rest are values its check accepts
    TrackOpts to{};
    to.max_residual = o.max_residual; to.huber = 1.0; to.max_var = INFINITY; to.stride = dim == 3 ? o.stride : 1;
    if (int rc = trk.setup(geo, in, cs, n, to, s)) return rc;
    const long long p = trk.points;
    const int mi = (int)m, nb = blocks_of(m), P = (int)pow2_at_least(nb), ns = dim == 3 ? 7 : 4;
    if (int rc = locate_score_launch(df, dim, d_pose[cur], mi, trk.d_loc, p, o.max_residual, d_cost, d_inl, s)) return rc;
    hipLaunchKernelGGL(pf_accum_kernel, dim3(nb), dim3(kBlock), 0, s, d_L, (const double*)d_cost, mi, o.beta, d_bmin);
    hipLaunchKernelGGL(pf_min_top_kernel, dim3(1), dim3(1024), 0, s, (const double*)d_bmin, nb, d_stats);
    hipLaunchKernelGGL(pf_weigh_kernel, dim3(nb), dim3(kBlock), 0, s, (const double*)d_L, mi, nb, (const PfStats*)d_stats, d_q, d_bsum, d_bkey);
    hipLaunchKernelGGL(pf_totals_top_kernel, dim3(1), dim3(1024), 0, s, (const u64*)d_bsum, (const u64*)d_bkey, nb, d_stats);
    const int eg = std::min(P, 1024);
    if (dim == 3)
        hipLaunchKernelGGL(pf_est_terms_kernel<3>, dim3(eg), dim3(kBlock), 0, s, (const double*)d_state[cur], (const u64*)d_q, mi, P,
                           (const PfStats*)d_stats, d_part);
    else
        hipLaunchKernelGGL(pf_est_terms_kernel<2>, dim3(eg), dim3(kBlock), 0, s, (const double*)d_state[cur], (const u64*)d_q, mi, P,
                           (const PfStats*)d_stats, d_part);
    hipLaunchKernelGGL(pf_est_top_kernel, dim3(1), dim3(1024), 0, s, ns, P, d_part, d_stats);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof(PfStats), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    stats = *h_stats;
    // the host's share: the division, the normalisation, the decision
    neff = (double)stats.Th * (double)stats.Th / (double)stats.S2;
    const double T = (double)stats.T;
    for (int c = 0; c < ns; ++c) est[c] = stats.sums[c] / T;
    if (dim == 2) {
        const double nn = std::sqrt(est[2] * est[2] + est[3] * est[3]);
        est[2] = est[2] / nn; est[3] = est[3] / nn;
        est_pose[0] = est[0]; est_pose[1] = est[1]; est_pose[2] = est[2]; est_pose[3] = est[3]; est_pose[4] = -est[3]; est_pose[5] = est[2];
    } else {
        const double nn = std::sqrt(est[3] * est[3] + est[4] * est[4] + est[5] * est[5] + est[6] * est[6]);
        for (int c = 3; c < 7; ++c) est[c] = est[c] / nn;
        for (int c = 0; c < 3; ++c) est_pose[c] = est[c];
        quat_to_mat(est + 3, est_pose + 3);
    }
    npoints = p; pixels = n; updates += 1; have_estimate = true;
    resampled = neff < o.resample_below * (double)m;
    if (resampled) {
        if (int rc = resample_launch(s)) return rc;
        GPIS_HIP(hipStreamSynchronize(s));
    }
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GPIS_OK;
}

int ParticleFilter::resample(hipStream_t s) {
    if (int rc = resample_launch(s)) return rc;
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}

// the scan of q (block scan, the scan of the block sums -- two more levels cover 2^24 -- and the adds), then the gather
int ParticleFilter::resample_launch(hipStream_t s) {
    tick += 1;
    const int mi = (int)m, nb1 = blocks_of(m), nb2 = blocks_of(nb1);
    const u64 T = stats.T, qs = T / (u64)m, rem = T % (u64)m;
    const uint32_t ctr[4] = {0xFFFFFFFFu, tick, 0u, 1u}, key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
    uint32_t w[4];
    pf_philox(ctr, key, w);
    const u64 r = (((u64)w[0] << 32) | (u64)w[1]) % qs;       // (qs >= 2^32 / 2^24: the best particle alone holds 2^32)
    hipLaunchKernelGGL(pf_scan_block_kernel, dim3(nb1), dim3(kBlock), 0, s, (const u64*)d_q, d_C, mi, d_s1);
    if (nb1 > 1) {
        hipLaunchKernelGGL(pf_scan_block_kernel, dim3(nb2), dim3(kBlock), 0, s, (const u64*)d_s1, d_s1, nb1, d_s2);
        if (nb2 > 1) {
            hipLaunchKernelGGL(pf_scan_block_kernel, dim3(1), dim3(kBlock), 0, s, (const u64*)d_s2, d_s2, nb2, d_s2 + 256);
            hipLaunchKernelGGL(pf_scan_add_kernel, dim3(nb2), dim3(kBlock), 0, s, d_s1, nb1, (const u64*)d_s2);
        }
        hipLaunchKernelGGL(pf_scan_add_kernel, dim3(nb1), dim3(kBlock), 0, s, d_C, mi, (const u64*)d_s1);
    }
    const int to = cur ^ 1;
    if (dim == 3)
        hipLaunchKernelGGL(pf_resample_kernel<3>, dim3(nb1), dim3(kBlock), 0, s, (const u64*)d_C, mi, qs, rem, r, (const double*)d_state[cur],
                           (const float*)d_pose[cur], d_state[to], d_pose[to], d_L, d_anc);
    else
        hipLaunchKernelGGL(pf_resample_kernel<2>, dim3(nb1), dim3(kBlock), 0, s, (const u64*)d_C, mi, qs, rem, r, (const double*)d_state[cur],
                           (const float*)d_pose[cur], d_state[to], d_pose[to], d_L, d_anc);
    GPIS_HIP(hipGetLastError());
    cur = to;
    resamples += 1;
    return GPIS_OK;
}

}  // namespace gpis
