// Pose-hypothesis scoring against a distance field (locate.h).  Per call: the tracker's set-up turns the frame
// into local points (16 B each), the poses go up in one copy, one kernel scores them -- a wavefront per pose, four poses per
// workgroup -- and 12 bytes per pose come back.  The kernel is bound by the field's gathers (4 / 8 loads per sample, cached: the
// poses of a batch and the lanes of a wavefront sample neighbouring cells); the local points are re-read by every wavefront
// from L2.
//
// Per point: the world point (world_point.h) with R, t straight from the float pose -- the tracker's function, so the point the
// tracker samples for that pose; d = df_sample_at's o[0]; e = |(double)d|; inlier iff d is finite and e <= max_residual; q = e
// for an inlier, else max_residual; the term is q * q in double.  Per pose: lane l adds the terms of points l, l + 64, ... in
// ascending order from 0.0, then v[k] = v[k] + v[k + h], h = 32 .. 1 through lane shuffles (block_ops.h: wave_reduce's order);
// lane 0 holds the sum.  One order, whatever the batch: a pose has the same bits alone and at any batch position.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include "dfield.h"
#include "locate.h"
#include "block_ops.h"
#include "world_point.h"

namespace gpis {

namespace {

constexpr int kBlock = Locator::kWaves * kWave;

template <int D>
__global__ void __launch_bounds__(kBlock) locate_score_kernel(const float* __restrict__ pose, int m, const float4* __restrict__ loc, int p,
                                                              const float* __restrict__ F, DfLattice L, double max_residual,
                                                              double* __restrict__ cost, int* __restrict__ inliers) {
    constexpr int NP = D == 3 ? 12 : 6;
    L.dim = D;
    const int lane = threadIdx.x & (kWave - 1);
    // the wavefront's pose: uniform, and provably so (scalar loads of R, t)
    const int k = (int)blockIdx.x * Locator::kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (k >= m) return;                        // (the whole wavefront)
    const float* __restrict__ P = pose + (size_t)k * NP;
    float t[D], R[D * D];
#pragma unroll
    for (int a = 0; a < D; ++a) t[a] = P[a];
#pragma unroll
    for (int a = 0; a < D * D; ++a) R[a] = P[D + a];
    double acc = 0.0;
    int cnt = 0;
    for (int i = lane; i < p; i += kWave) {
        const float4 l = loc[i];
        float x[3] = {0.f, 0.f, 0.f}, o[1 + D];
        world_point<D>(R, t, l, x);
        df_sample_at(F, L, x[0], x[1], x[2], o);
        const float d = o[0];
        const double e = fabs((double)d);
        const bool in = isfinite(d) && e <= max_residual;
        const double q = in ? e : max_residual;
        acc = acc + q * q;
        cnt += in ? 1 : 0;
    }
#pragma unroll
    for (int h = kWave / 2; h >= 1; h >>= 1) {       // (block_ops.h: wave_reduce's order, the two chains interleaved)
        acc = acc + __shfl_down(acc, h, kWave);
        cnt += __shfl_down(cnt, h, kWave);
    }
    if (lane == 0) {
        cost[k] = acc;
        inliers[k] = cnt;
    }
}

}  // namespace

int locate_check_opts(const LocateOpts& o) {
    if (!(std::isfinite(o.max_residual) && o.max_residual >= 0.0) || o.stride < 1 || o.top_k < 0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int locate_score_launch(const DistanceField& df, int dim, const float* d_pose, int m, const float* d_loc, long long p,
                        double max_residual, double* d_cost, int* d_inliers, hipStream_t s) {
    const int grid = (m + Locator::kWaves - 1) / Locator::kWaves;
    if (dim == 3)
        hipLaunchKernelGGL(locate_score_kernel<3>, dim3(grid), dim3(kBlock), 0, s, d_pose, m, (const float4*)d_loc, (int)p,
                           (const float*)df.d_dist, df.lattice(), max_residual, d_cost, d_inliers);
    else
        hipLaunchKernelGGL(locate_score_kernel<2>, dim3(grid), dim3(kBlock), 0, s, d_pose, m, (const float4*)d_loc, (int)p,
                           (const float*)df.d_dist, df.lattice(), max_residual, d_cost, d_inliers);
    GPIS_HIP(hipGetLastError());
    return GPIS_OK;
}

Locator::Locator() { (void)hipGetDevice(&device); }

Locator::~Locator() { (void)bind(-1); }

int Locator::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (trk.own) (void)hipStreamSynchronize(trk.own);
        (void)hipFree(d_pose);
        (void)hipFree(d_out);
        if (h_pose) (void)hipHostFree(h_pose);
        if (h_out) (void)hipHostFree(h_out);
    }
    d_pose = nullptr; d_out = nullptr; h_pose = nullptr; h_out = nullptr; cap_m = 0;
    clear_result();
    device = dev;
    return trk.bind(dev);
}

int Locator::ensure(long long m) {
    if ((size_t)m <= cap_m) return GPIS_OK;
    (void)hipFree(d_pose);
    (void)hipFree(d_out);
    if (h_pose) (void)hipHostFree(h_pose);
    if (h_out) (void)hipHostFree(h_out);
    d_pose = nullptr; d_out = nullptr; h_pose = nullptr; h_out = nullptr; cap_m = 0;
    GPIS_HIP(hipMalloc((void**)&d_pose, sizeof(float) * 12 * (size_t)m));
    GPIS_HIP(hipMalloc((void**)&d_out, (sizeof(double) + sizeof(int)) * (size_t)m));
    GPIS_HIP(hipHostMalloc((void**)&h_pose, sizeof(float) * 12 * (size_t)m));
    GPIS_HIP(hipHostMalloc((void**)&h_out, (sizeof(double) + sizeof(int)) * (size_t)m));
    cap_m = (size_t)m;
    return GPIS_OK;
}

int Locator::score(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n, const float* pose, int m,
                   const LocateOpts& o, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    clear_result();
    const int dm = geo.dim, np = dm == 3 ? 12 : 6;
    // the tracker's set-up reads the stride alone; the rest are values its check accepts
    TrackOpts to{};
    to.max_residual = o.max_residual; to.huber = 1.0; to.max_var = INFINITY; to.stride = dm == 3 ? o.stride : 1;
    if (int rc = trk.setup(geo, in, cs, n, to, s)) return rc;
    const long long p = trk.points;
    if (int rc = ensure(m)) return rc;
    const size_t mm = (size_t)m;
    std::memcpy(h_pose, pose, sizeof(float) * np * mm);
    GPIS_HIP(hipMemcpyAsync(d_pose, h_pose, sizeof(float) * np * mm, hipMemcpyHostToDevice, s));
    double* dc = (double*)d_out;
    int* di = (int*)(d_out + sizeof(double) * mm);
    if (int rc = locate_score_launch(df, dm, d_pose, m, trk.d_loc, p, o.max_residual, dc, di, s)) return rc;
    GPIS_HIP(hipMemcpyAsync(h_out, d_out, (sizeof(double) + sizeof(int)) * mm, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    cost.assign((const double*)h_out, (const double*)h_out + mm);
    inliers.assign((const int*)(h_out + sizeof(double) * mm), (const int*)(h_out + sizeof(double) * mm) + mm);
    // the ranking: cost ascending, ties by the lower index
    order.resize(mm);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [this](int a, int b) { return cost[a] < cost[b]; });
    order.resize(o.top_k == 0 ? mm : std::min(mm, (size_t)o.top_k));
    dim = dm; poses = m; npoints = p; pixels = n; valid = true;
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GPIS_OK;
}

}  // namespace gpis
