// Sensor tracking (track.h).  Per call: the valid pixels / beams are flagged and compacted once (the renderer's
// order-keeping scan) and back-projected to local points; per iteration: one transform + pre-fill pass, the map's test() on the
// points, one kernel that turns every record into its residual / Jacobian terms and reduces them per segment of 256 points, one
// block that reduces the segment partials; the sums (29 / 11 doubles) come back in one page-locked copy.  Memory-bound passes of
// a few bytes per point: grid-stride loops over at most kGridCap blocks of 256 threads (cdna_hip_programming.md Guideline 11).
//
// Point k of a 3-D frame is pixel (col, row) = (n * stride, m * stride), n < W / stride, m < H / stride, in column-major order
// (update()'s sampling with obs_skip = stride); it is used iff 0.4 < (double)z < 4 (isRangeValid).  u = ((float)col - cx) / fx,
// v = ((float)row - cy) / fy, local point (u z, v z, z), world R[i] x + R[3+i] y + R[6+i] z + t[i] left to right (no FMA:
// -ffp-contract=off) with the pose in float: the point update() would insert.  2-D: beams with 0.2 < (double)r < 30 in input
// order, local ((float)(r c) + off0, (float)(r s) + off1) with host-double (c, s), world R local + t.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include "dfield.h"
#include "map_query.h"
#include "render.h"
#include "track.h"
#include "block_ops.h"
#include "world_point.h"

namespace gpis {

namespace {

constexpr int kBlock = Tracker::kSeg;     // one segment per block in the term kernel

struct PassPose { float R[9], t[3]; };     // the pose of one pass in float (3-D R column-major; 2-D R[0..3], t[0..1])

// residual of a record: r = f - level (float); inlier iff f and the gradient are finite, var_f <= max_var and |r| <= max_residual
// (compared in double)
__device__ __forceinline__ bool residual(const float* __restrict__ rec, int dim, float level, double max_residual, double max_var,
                                         float& r) {
    const float f = rec[0];
    r = f - level;
    const bool g_ok = isfinite(rec[1]) && isfinite(rec[2]) && (dim == 2 || isfinite(rec[3]));
    return isfinite(f) && g_ok && (double)rec[1 + dim] <= max_var && fabs((double)r) <= max_residual;
}

// flag[q] = sample q of the grid is valid (3-D: q = n * mh + m over the W / stride x H / stride grid; 2-D: the beam q)
__global__ void __launch_bounds__(kBlock) track_flag_kernel(int dim, int height, int stride, int mh, int ngrid, const float* __restrict__ in,
                                                            uint8_t* __restrict__ flag) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < ngrid; q += gridDim.x * blockDim.x) {
        bool ok;
        if (dim == 3) {
            const int n = q / mh, m = q - n * mh;
            const double z = (double)in[(size_t)n * stride * height + (size_t)m * stride];
            ok = z > 4e-1 && z < 4e0;
        } else {
            const double r = (double)in[q];
            ok = r > 2e-1 && r < 3e1;
        }
        flag[q] = ok ? 1 : 0;
    }
}

// local point and pixel index of the listed samples: loc[j] = (x, y, z, pixel bits)
__global__ void __launch_bounds__(kBlock) track_gather_kernel(TrackGeom g, int stride, int mh, const int* __restrict__ list, int m,
                                                              const float* __restrict__ in, const double* __restrict__ cs,
                                                              float4* __restrict__ loc) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int q = list[j];
        float4 o;
        if (g.dim == 3) {
            const int n = q / mh, mm = q - n * mh;
            const int col = n * stride, row = mm * stride, k = col * g.height + row;
            const float z = in[k];
            const float u = ((float)col - g.cx) / g.fx, v = ((float)row - g.cy) / g.fy;
            o = make_float4(u * z, v * z, z, __int_as_float(k));
        } else {
            const double r = (double)in[q];
            o = make_float4((float)(r * cs[2 * (size_t)q]) + g.off[0], (float)(r * cs[2 * (size_t)q + 1]) + g.off[1], 0.f, __int_as_float(q));
        }
        loc[j] = o;
    }
}

// world points of the pass (world_point.h) and their pre-filled records (f = NaN, zeros elsewhere)
__global__ void __launch_bounds__(kBlock) track_transform_kernel(int dim, PassPose P, const float4* __restrict__ loc, int m,
                                                                 float* __restrict__ x, float* __restrict__ rec) {
    const int nc = 2 * (1 + dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const float4 l = loc[j];
        if (dim == 3) world_point<3>(P.R, P.t, l, x + 3 * (size_t)j);
        else world_point<2>(P.R, P.t, l, x + 2 * (size_t)j);
        rec[(size_t)j * nc] = __int_as_float(0x7fc00000);
        for (int c = 1; c < nc; ++c) rec[(size_t)j * nc + c] = 0.f;
    }
}

template <int D> struct Sums {
    static constexpr int NJ = D == 3 ? 6 : 3;
    static constexpr int NS = NJ * (NJ + 1) / 2 + NJ + 2;
};

// the terms of one inlier into a[]: r, its gradient g and its world point x in float; J = [g ; (x - t) x g] (2-D
// [gx, gy, (x - tx) gy - (y - ty) gx]) in double; the upper triangle of w J J^T row by row, w J r, w r^2, 1
template <int D>
__device__ __forceinline__ void point_terms(const PassPose& P, float r, const float* __restrict__ g, const float* __restrict__ x,
                                            double huber, double* __restrict__ a) {
    constexpr int NJ = Sums<D>::NJ, NS = Sums<D>::NS;
    const double rr = (double)r, ar = fabs(rr);
    const double w = ar <= huber ? 1.0 : huber / ar;
    double J[NJ];
    if constexpr (D == 3) {
        const double g0 = g[0], g1 = g[1], g2 = g[2];
        const double d0 = (double)x[0] - (double)P.t[0];
        const double d1 = (double)x[1] - (double)P.t[1];
        const double d2 = (double)x[2] - (double)P.t[2];
        J[0] = g0; J[1] = g1; J[2] = g2;
        J[3] = d1 * g2 - d2 * g1;
        J[4] = d2 * g0 - d0 * g2;
        J[5] = d0 * g1 - d1 * g0;
    } else {
        const double g0 = g[0], g1 = g[1];
        const double d0 = (double)x[0] - (double)P.t[0];
        const double d1 = (double)x[1] - (double)P.t[1];
        J[0] = g0; J[1] = g1;
        J[2] = d0 * g1 - d1 * g0;
    }
    int c = 0;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const double wj = w * J[i];
#pragma unroll
        for (int k = i; k < NJ; ++k) a[c++] = wj * J[k];
    }
#pragma unroll
    for (int i = 0; i < NJ; ++i) a[NJ * (NJ + 1) / 2 + i] = (w * J[i]) * rr;
    a[NS - 2] = (w * rr) * rr;
    a[NS - 1] = 1.0;
}

// The terms of every point and their sum per segment of 256 consecutive points (zero-padded; block_ops.h: segment_reduce states
// the order): part[c * P + segment], c < NS:
// the upper triangle of H = sum w J J^T row by row, b = sum w J r, sum w r^2, the inlier count.  Segments nseg .. P - 1 are
// all padding (+0).  Terms in double from the float values; non-inliers contribute +0.
template <int D>
__global__ void __launch_bounds__(kBlock) track_terms_kernel(PassPose P, const float* __restrict__ x, const float* __restrict__ rec, int m,
                                                             int nseg_pow2, float level, double max_residual, double huber,
                                                             double max_var, double* __restrict__ part) {
    constexpr int NS = Sums<D>::NS;
    constexpr int NC = 2 * (1 + D);
    __shared__ double sh[NS][kBlock / 2];
    const int tid = threadIdx.x;
    for (int seg = blockIdx.x; seg < nseg_pow2; seg += gridDim.x) {
        const int j = seg * kBlock + tid;
        double a[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) a[c] = 0.0;
        float r;
        if (j < m && residual(rec + (size_t)j * NC, D, level, max_residual, max_var, r))
            point_terms<D>(P, r, rec + (size_t)j * NC + 1, x + (size_t)j * D, huber, a);
        segment_reduce<NS, kBlock>(a, sh, tid, seg, nseg_pow2, part);
    }
}

// The field's residual of a local point at the pass pose: its world point x, the sampled distance and gradient o (df_sample_at);
// r = o[0] (the field's level is zero: o[0] - 0.0f has the same bits); inlier iff o is finite and |r| <= max_residual (compared
// in double; no variance test)
template <int D>
__device__ __forceinline__ bool field_residual(const PassPose& P, const float4 l, const float* __restrict__ F, const DfLattice& L,
                                               double max_residual, float* __restrict__ x, float* __restrict__ o) {
    world_point<D>(P.R, P.t, l, x);
    df_sample_at(F, L, x[0], x[1], D == 3 ? x[2] : 0.f, o);
    const bool g_ok = isfinite(o[1]) && isfinite(o[2]) && (D == 2 || isfinite(o[3]));
    return isfinite(o[0]) && g_ok && fabs((double)o[0]) <= max_residual;
}

// One pass against a distance field, fused: world point, sample, terms and the segment tree of track_terms_kernel, from the
// local points (16 B per point); nothing is written per point.  L.dim == D.
template <int D>
__global__ void __launch_bounds__(kBlock) track_field_terms_kernel(PassPose P, const float4* __restrict__ loc, int m, int nseg_pow2,
                                                                   const float* __restrict__ F, DfLattice L, double max_residual,
                                                                   double huber, double* __restrict__ part) {
    constexpr int NS = Sums<D>::NS;
    __shared__ double sh[NS][kBlock / 2];
    L.dim = D;
    const int tid = threadIdx.x;
    for (int seg = blockIdx.x; seg < nseg_pow2; seg += gridDim.x) {
        const int j = seg * kBlock + tid;
        double a[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) a[c] = 0.0;
        float x[D], o[1 + D];
        if (j < m && field_residual<D>(P, loc[j], F, L, max_residual, x, o)) point_terms<D>(P, o[0], o + 1, x, huber, a);
        segment_reduce<NS, kBlock>(a, sh, tid, seg, nseg_pow2, part);
    }
}

// The segment partials of every sum reduced by the same halving tree (block_ops.h: tree_top; P a power of two, in place);
// sum[c] = the result.  One block.
__global__ void __launch_bounds__(1024) track_top_kernel(int ns, int P, double* __restrict__ part, double* __restrict__ sum) {
    tree_top(ns, P, part);
    if ((int)threadIdx.x < ns) sum[threadIdx.x] = part[(size_t)threadIdx.x * P];
}

// the residual image of the final pass: r at the pixel of every inlier (the image is NaN-filled before)
__global__ void __launch_bounds__(kBlock) track_resid_kernel(int dim, const float4* __restrict__ loc, const float* __restrict__ rec, int m,
                                                             float level, double max_residual, double max_var, float* __restrict__ resid) {
    const int nc = 2 * (1 + dim);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        float r;
        if (residual(rec + (size_t)j * nc, dim, level, max_residual, max_var, r)) resid[__float_as_int(loc[j].w)] = r;
    }
}

// the residual image of the final pass against a field: the points sampled again at that pass's pose
template <int D>
__global__ void __launch_bounds__(kBlock) track_field_resid_kernel(PassPose P, const float4* __restrict__ loc, int m,
                                                                   const float* __restrict__ F, DfLattice L, double max_residual,
                                                                   float* __restrict__ resid) {
    L.dim = D;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const float4 l = loc[j];
        float x[D], o[1 + D];
        if (field_residual<D>(P, l, F, L, max_residual, x, o)) resid[__float_as_int(l.w)] = o[0];
    }
}

PassPose pass_pose(int dim, const double* pose) {
    PassPose P{};
    const int nt = dim, nr = dim * dim;
    for (int k = 0; k < nt; ++k) P.t[k] = (float)pose[k];
    for (int k = 0; k < nr; ++k) P.R[k] = (float)pose[nt + k];
    return P;
}

}  // namespace

bool track_solve(int n, const double* H, const double* b, double lambda, double* x) {
    double A[6][6], L[6][6] = {}, y[6];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A[i][j] = H[i * n + j];
    for (int i = 0; i < n; ++i) A[i][i] = H[i * n + i] + lambda * H[i * n + i];
    for (int j = 0; j < n; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > 0.0)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = -b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < n; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

void track_apply(int dim, const double* delta, double* pose) {
    if (dim == 3) {
        const double w0 = delta[3], w1 = delta[4], w2 = delta[5];
        const double th2 = w0 * w0 + w1 * w1 + w2 * w2, th = std::sqrt(th2);
        double A, B;
        if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }      // (Taylor terms below one ulp there)
        else { A = std::sin(th) / th; B = (1.0 - std::cos(th)) / th2; }
        const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
        double E[3][3], R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double kk = K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c];
                E[r][c] = ((r == c ? 1.0 : 0.0) + A * K[r][c]) + B * kk;
            }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r][c] = E[r][0] * pose[3 + 3 * c] + E[r][1] * pose[4 + 3 * c] + E[r][2] * pose[5 + 3 * c];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) pose[3 + 3 * c + r] = R[r][c];
        for (int k = 0; k < 3; ++k) pose[k] = pose[k] + delta[k];
    } else {
        const double c = std::cos(delta[2]), s = std::sin(delta[2]);
        const double E[2][2] = {{c, -s}, {s, c}};
        double R[2][2];
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < 2; ++k) R[r][k] = E[r][0] * pose[2 + 2 * k] + E[r][1] * pose[3 + 2 * k];
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < 2; ++k) pose[2 + 2 * k + r] = R[r][k];
        for (int k = 0; k < 2; ++k) pose[k] = pose[k] + delta[k];
    }
}

int track_check_opts(const TrackOpts& o) {
    auto nonneg = [](double v) { return !std::isnan(v) && v >= 0.0; };
    if (!nonneg(o.max_residual) || !nonneg(o.max_var) || !nonneg(o.damping) || !nonneg(o.eps_t) || !nonneg(o.eps_r)) return GPIS_ERR_ARG;
    if (!(std::isfinite(o.huber) && o.huber > 0.0) || !std::isfinite(o.level)) return GPIS_ERR_ARG;
    if (std::isinf(o.damping) || o.stride < 1 || o.max_iters < 0 || o.min_inliers < 0) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int track_check_geom(const TrackGeom& g, long long n) {
    if (g.dim == 3) {
        if (g.width < 1 || g.height < 1 || !std::isfinite(g.fx) || !std::isfinite(g.fy) || g.fx == 0.f || g.fy == 0.f ||
            !std::isfinite(g.cx) || !std::isfinite(g.cy))
            return GPIS_ERR_ARG;
        if (n != (long long)g.width * g.height) return GPIS_ERR_ARG;
    } else if (g.dim != 2 || n < 1 || !std::isfinite(g.off[0]) || !std::isfinite(g.off[1])) {
        return GPIS_ERR_ARG;
    }
    if (n > Tracker::kMaxPoints) return GPIS_ERR_LIMIT;
    return GPIS_OK;
}

Tracker::Tracker() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Tracker::~Tracker() { (void)bind(-1); }

int Tracker::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_in, (void*)d_cs, (void*)d_flag, (void*)d_list, (void*)d_loc, (void*)d_x, (void*)d_rec, (void*)d_part,
                        (void*)d_sum, (void*)d_resid, (void*)d_scan})
            (void)hipFree(p);
        for (void* p : {(void*)h_cnt, (void*)h_sum, (void*)h_in, (void*)h_cs})
            if (p) (void)hipHostFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_in = nullptr; d_cs = nullptr; d_flag = nullptr; d_list = nullptr; d_loc = d_x = d_rec = nullptr; d_part = d_sum = nullptr;
    d_resid = nullptr; d_scan = nullptr; h_cnt = nullptr; h_sum = nullptr; h_in = nullptr; h_cs = nullptr; own = nullptr;
    cap_pix = cap_grid = cap_part = cap_hin = cap_hcs = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

// per pixel: input, residual image; per grid sample (>= points): flags, list, local points, world points, records
int Tracker::ensure(long long npix, long long ngrid, int dm) {
    if ((size_t)npix > cap_pix) {
        for (void* p : {(void*)d_in, (void*)d_resid, (void*)d_cs}) (void)hipFree(p);
        if (h_in) (void)hipHostFree(h_in);
        if (h_cs) (void)hipHostFree(h_cs);
        d_in = d_resid = nullptr; d_cs = nullptr; h_in = nullptr; h_cs = nullptr; cap_pix = cap_hin = cap_hcs = 0;
        GPIS_HIP(hipMalloc((void**)&d_in, sizeof(float) * npix));
        GPIS_HIP(hipMalloc((void**)&d_resid, sizeof(float) * npix));
        GPIS_HIP(hipMalloc((void**)&d_cs, sizeof(double) * 2 * npix));
        GPIS_HIP(hipHostMalloc((void**)&h_in, sizeof(float) * npix));
        cap_pix = cap_hin = (size_t)npix;
    }
    if (dm == 2 && (size_t)npix > cap_hcs) {
        if (h_cs) (void)hipHostFree(h_cs);
        h_cs = nullptr; cap_hcs = 0;
        GPIS_HIP(hipHostMalloc((void**)&h_cs, sizeof(double) * 2 * npix));
        cap_hcs = (size_t)npix;
    }
    const long long ng = std::max(1ll, ngrid);
    if ((size_t)ng > cap_grid) {
        for (void* p : {(void*)d_flag, (void*)d_list, (void*)d_loc, (void*)d_x, (void*)d_rec}) (void)hipFree(p);
        d_flag = nullptr; d_list = nullptr; d_loc = d_x = d_rec = nullptr; cap_grid = 0;
        GPIS_HIP(hipMalloc((void**)&d_flag, ng));
        GPIS_HIP(hipMalloc((void**)&d_list, sizeof(int) * ng));
        GPIS_HIP(hipMalloc((void**)&d_loc, sizeof(float4) * ng));
        GPIS_HIP(hipMalloc((void**)&d_x, sizeof(float) * 3 * ng));
        GPIS_HIP(hipMalloc((void**)&d_rec, sizeof(float) * 8 * ng));
        cap_grid = (size_t)ng;
    }
    const long long np = pow2_at_least((ng + kSeg - 1) / kSeg);
    if ((size_t)np > cap_part) {
        (void)hipFree(d_part);
        d_part = nullptr; cap_part = 0;
        GPIS_HIP(hipMalloc((void**)&d_part, sizeof(double) * kSums3 * np));
        cap_part = (size_t)np;
    }
    if (!d_sum) GPIS_HIP(hipMalloc((void**)&d_sum, sizeof(double) * kSums3));
    if (!d_scan) GPIS_HIP(hipMalloc((void**)&d_scan, sizeof(int) * (kCompactBlocks + 1)));
    if (!h_cnt) GPIS_HIP(hipHostMalloc((void**)&h_cnt, sizeof(int)));
    if (!h_sum) GPIS_HIP(hipHostMalloc((void**)&h_sum, sizeof(double) * kSums3));
    return GPIS_OK;
}

// transform + pre-fill, test() in calls of at most `chunk` points, terms, reduction, the sums to the host
int Tracker::pass(MapQuery& mq, OnGPISStore& store, bool have_map, const TrackGeom& geo, const double* pose, const TrackOpts& o,
                  hipStream_t s, double* sums) {
    const auto t0 = std::chrono::steady_clock::now();
    const int dm = geo.dim, nc = 2 * (1 + dm);
    const long long m = points;
    const PassPose P = pass_pose(dm, pose);
    if (m > 0) {
        hipLaunchKernelGGL(track_transform_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, dm, P, (const float4*)d_loc, (int)m, d_x, d_rec);
        GPIS_HIP(hipGetLastError());
    }
    if (have_map) {
        const long long C = std::max(1, chunk);
        for (long long off = 0; off < m; off += C) {
            const int len = (int)std::min(C, m - off);
            if (int rc = mq.run_prepared(store, d_x + (size_t)off * dm, len, d_rec + (size_t)off * nc, s)) return rc;
            evals += mq.last_evals;
            k4_ms += mq.last_eval_ms;
        }
    }
    const long long np = pow2_at_least((m + kSeg - 1) / kSeg);
    const int grid = (int)std::min((long long)kGridCap, np);
    if (dm == 3)
        hipLaunchKernelGGL(track_terms_kernel<3>, dim3(grid), dim3(kBlock), 0, s, P, d_x, d_rec, (int)m, (int)np, o.level, o.max_residual,
                           o.huber, o.max_var, d_part);
    else
        hipLaunchKernelGGL(track_terms_kernel<2>, dim3(grid), dim3(kBlock), 0, s, P, d_x, d_rec, (int)m, (int)np, o.level, o.max_residual,
                           o.huber, o.max_var, d_part);
    return pass_sums(dm, np, s, sums, t0);
}

// one fused kernel (world point, sample, terms, segment tree), reduction, the sums to the host
int Tracker::field_pass(const DistanceField& df, int dm, const double* pose, const TrackOpts& o, hipStream_t s, double* sums) {
    const auto t0 = std::chrono::steady_clock::now();
    const long long m = points;
    const PassPose P = pass_pose(dm, pose);
    const long long np = pow2_at_least((m + kSeg - 1) / kSeg);
    const int grid = (int)std::min((long long)kGridCap, np);
    if (dm == 3)
        hipLaunchKernelGGL(track_field_terms_kernel<3>, dim3(grid), dim3(kBlock), 0, s, P, (const float4*)d_loc, (int)m, (int)np, df.d_dist,
                           df.lattice(), o.max_residual, o.huber, d_part);
    else
        hipLaunchKernelGGL(track_field_terms_kernel<2>, dim3(grid), dim3(kBlock), 0, s, P, (const float4*)d_loc, (int)m, (int)np, df.d_dist,
                           df.lattice(), o.max_residual, o.huber, d_part);
    return pass_sums(dm, np, s, sums, t0);
}

// the top tree over the np segment partials, the one page-locked copy of the sums; counts the pass and its host wall time
int Tracker::pass_sums(int dm, long long np, hipStream_t s, double* sums, std::chrono::steady_clock::time_point t0) {
    const int ns = dm == 3 ? kSums3 : kSums2;
    hipLaunchKernelGGL(track_top_kernel, dim3(1), dim3(1024), 0, s, ns, (int)np, d_part, d_sum);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_sum, d_sum, sizeof(double) * ns, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    std::memcpy(sums, h_sum, sizeof(double) * ns);
    ++passes;
    pass_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GPIS_OK;
}

// the set-up shared by every call: checks, buffers, the input uploaded, the valid samples flagged, compacted and gathered into
// local points (`points` of them)
int Tracker::setup(const TrackGeom& geo, const float* in, const double* cs, long long n, const TrackOpts& o, hipStream_t s) {
    clear_result();
    if (int rc = track_check_opts(o)) return rc;
    if (int rc = track_check_geom(geo, n)) return rc;
    const int dm = geo.dim;
    const int mh = dm == 3 ? geo.height / o.stride : 0;
    const long long ngrid = dm == 3 ? (long long)(geo.width / o.stride) * mh : n;
    if (int rc = ensure(n, ngrid, dm)) return rc;
    std::memcpy(h_in, in, sizeof(float) * (size_t)n);
    GPIS_HIP(hipMemcpyAsync(d_in, h_in, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    if (dm == 2) {
        std::memcpy(h_cs, cs, sizeof(double) * 2 * (size_t)n);
        GPIS_HIP(hipMemcpyAsync(d_cs, h_cs, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    long long m = 0;
    if (ngrid > 0) {
        hipLaunchKernelGGL(track_flag_kernel, dim3(grid_for(ngrid)), dim3(kBlock), 0, s, dm, geo.height, o.stride, mh, (int)ngrid, d_in, d_flag);
        GPIS_HIP(hipGetLastError());
        if (int rc = compact_flags(d_flag, nullptr, ngrid, d_list, d_scan, h_cnt, s, &m)) return rc;
    }
    if (m > 0) {
        hipLaunchKernelGGL(track_gather_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, geo, o.stride, mh, d_list, (int)m, d_in, d_cs,
                           (float4*)d_loc);
        GPIS_HIP(hipGetLastError());
    }
    points = m;
    return GPIS_OK;
}

// The Gauss-Newton loop from pose0 with `pass_at(pose, sums)` as the pass: cur = the returned pose, S = the sums of the last
// pass (which ran at cur), st / it the status and the steps taken; sets cost0
int Tracker::iterate(int dm, const double* pose0, const TrackOpts& o, const PassFn& pass_at, double* cur, double* S, int& st, int& it) {
    const int nj = dm == 3 ? 6 : 3, nt = dm, np = dm == 3 ? 12 : 6;
    double prev[12], delta[6];
    for (int k = 0; k < np; ++k) cur[k] = pose0[k];
    const int nh = nj * (nj + 1) / 2;
    if (int rc = pass_at(cur, S)) return rc;
    cost0 = S[nh + nj];
    st = 1; it = 0;
    bool again = false;                      // one more pass at the returned pose
    for (;;) {
        if (S[nh + nj + 1] < (double)o.min_inliers) {
            st = 2;
            if (it > 0) { for (int k = 0; k < np; ++k) cur[k] = prev[k]; again = true; }
            break;
        }
        if (it >= o.max_iters) { st = 1; break; }
        double Hf[36];
        for (int i = 0, c = 0; i < nj; ++i)
            for (int k = i; k < nj; ++k, ++c) Hf[i * nj + k] = Hf[k * nj + i] = S[c];
        if (!track_solve(nj, Hf, S + nh, o.damping, delta)) { st = 3; break; }
        for (int k = 0; k < np; ++k) prev[k] = cur[k];
        track_apply(dm, delta, cur);
        ++it;
        double nv = 0.0, nw = 0.0;
        for (int k = 0; k < nt; ++k) nv = nv + delta[k] * delta[k];
        for (int k = nt; k < nj; ++k) nw = nw + delta[k] * delta[k];
        if (std::sqrt(nv) < o.eps_t && std::sqrt(nw) < o.eps_r) { st = 0; again = true; break; }
        if (int rc = pass_at(cur, S)) return rc;
    }
    if (again)
        if (int rc = pass_at(cur, S)) return rc;
    return GPIS_OK;
}

// the result of a finished call (the residual image is written)
void Tracker::finish(int dm, long long n, const double* cur, const double* S, int st, int it) {
    const int nj = dm == 3 ? 6 : 3, np = dm == 3 ? 12 : 6, nh = nj * (nj + 1) / 2;
    for (int i = 0, c = 0; i < nj; ++i)
        for (int k = i; k < nj; ++k, ++c) H[i * nj + k] = H[k * nj + i] = S[c];
    for (int i = 0; i < nj; ++i) b[i] = S[nh + i];
    cost = S[nh + nj];
    inliers = S[nh + nj + 1];
    for (int k = 0; k < np; ++k) pose[k] = cur[k];
    status = st; iterations = it; dim = dm; pixels = n; valid = true;
}

int Tracker::track(MapQuery& mq, OnGPISStore& store, bool have_map, const TrackGeom& geo, const float* in, const double* cs, long long n,
                   const double* pose0, const TrackOpts& o, hipStream_t s) {
    if (int rc = setup(geo, in, cs, n, o, s)) return rc;
    const int dm = geo.dim;
    const long long m = points;
    const bool query = have_map && m > 0;
    if (query)
        if (int rc = mq.prepare(store, s)) return rc;
    double cur[12], S[kSums3] = {};
    int st = 1, it = 0;
    const PassFn pass_at = [&](const double* p, double* sums) { return pass(mq, store, query, geo, p, o, s, sums); };
    if (int rc = iterate(dm, pose0, o, pass_at, cur, S, st, it)) return rc;
    // the residual image of the final pass
    GPIS_HIP(hipMemsetD32Async((hipDeviceptr_t)d_resid, 0x7fc00000, (size_t)n, s));
    if (m > 0)
        hipLaunchKernelGGL(track_resid_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, dm, (const float4*)d_loc, d_rec, (int)m, o.level,
                           o.max_residual, o.max_var, d_resid);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    finish(dm, n, cur, S, st, it);
    return GPIS_OK;
}

int Tracker::track_field(const DistanceField& df, const TrackGeom& geo, const float* in, const double* cs, long long n,
                         const double* pose0, const TrackOpts& o, hipStream_t s) {
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != geo.dim) return GPIS_ERR_ARG;
    TrackOpts of = o;
    of.level = 0.f;                          // (not read: the field's level is zero by construction)
    of.max_var = INFINITY;                   // (not read: the field applied its gate when it was built)
    if (int rc = setup(geo, in, cs, n, of, s)) return rc;
    const int dm = geo.dim;
    const long long m = points;
    double cur[12], S[kSums3] = {};
    int st = 1, it = 0;
    const PassFn pass_at = [&](const double* p, double* sums) { return field_pass(df, dm, p, of, s, sums); };
    if (int rc = iterate(dm, pose0, of, pass_at, cur, S, st, it)) return rc;
    // the residual image of the final pass: its points sampled again at the returned pose
    GPIS_HIP(hipMemsetD32Async((hipDeviceptr_t)d_resid, 0x7fc00000, (size_t)n, s));
    if (m > 0) {
        const PassPose P = pass_pose(dm, cur);
        if (dm == 3)
            hipLaunchKernelGGL(track_field_resid_kernel<3>, dim3(grid_for(m)), dim3(kBlock), 0, s, P, (const float4*)d_loc, (int)m, df.d_dist,
                               df.lattice(), of.max_residual, d_resid);
        else
            hipLaunchKernelGGL(track_field_resid_kernel<2>, dim3(grid_for(m)), dim3(kBlock), 0, s, P, (const float4*)d_loc, (int)m, df.d_dist,
                               df.lattice(), of.max_residual, d_resid);
    }
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    finish(dm, n, cur, S, st, it);
    return GPIS_OK;
}

}  // namespace gpis
