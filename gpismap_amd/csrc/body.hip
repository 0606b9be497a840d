// The robot's footprint (body.h): host state, the upload of its device table, and the batch query of states
// against a distance field.  The query is two launches: a thread per state applies the body rule and every workgroup leaves its
// integer counts and its least (D, index); one workgroup then combines the blocks' partials.  Integer sums and minima of doubles
// that are never NaN where they are taken: order-free, no atomics.  The rollouts that read the table are the controller's
// (mppi.hip), the trajectory check is traj.hip's.
#include <cmath>
#include <cstring>
#include <vector>
#include "body.h"
#include "dfield.h"
#include "block_ops.h"

namespace gpis {

namespace {

constexpr int kBlock = Footprint::kBlock;

// the block's (or the grid's) least D by (D, index): the least D first, then the least index among the threads that hold it
__device__ __forceinline__ void least_of(double d, int idx, double* shd, int* shi, double* least, int* at) {
    const double m = block_reduce(d, OpMin(), shd, kBlock, (double)INFINITY);
    if (threadIdx.x == 0) shd[0] = m;
    __syncthreads();
    const double lo = shd[0];
    const int key = idx >= 0 && d == lo ? idx : 0x7fffffff;
    const int k = block_reduce(key, OpMin(), shi, kBlock, 0x7fffffff);
    *least = lo;
    *at = k;
}

template <int D>
__global__ void __launch_bounds__(kBlock) body_clearance_kernel(const float* __restrict__ F, DfLattice L, BodyArgs bd,
                                                                const double* __restrict__ states, int n, double clr,
                                                                double* __restrict__ Dout, int* __restrict__ ball, int nb,
                                                                double* __restrict__ bmin, int* __restrict__ bint) {
    constexpr int NS = D + 2;
    __shared__ double shd[kBlock / kWave];
    __shared__ int shi[kBlock / kWave];
    DfLattice Lc = L;
    Lc.dim = D;
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    double d = INFINITY;
    int idx = -1, below = 0, off = 0;
    if (i < n) {
        const double* __restrict__ S = states + (size_t)i * NS;
        double p[3] = {S[0], S[1], D == 3 ? S[2] : 0.0};
        int jm;
        const double v = body_clearance_at<D>(F, Lc, bd.tab, bd.m, p, S[D], S[D + 1], &jm);
        Dout[i] = v;
        ball[i] = jm;
        if (v != v) off = 1;
        else { d = v; idx = i; below = v < clr ? 1 : 0; }
    }
    double least;
    int at;
    least_of(d, idx, shd, shi, &least, &at);
    const int nbelow = block_reduce(below, OpAdd(), shi, kBlock, 0);
    const int noff = block_reduce(off, OpAdd(), shi, kBlock, 0);
    if (threadIdx.x == 0) {
        bmin[blockIdx.x] = least;
        bint[blockIdx.x] = nbelow; bint[(size_t)nb + blockIdx.x] = noff; bint[2 * (size_t)nb + blockIdx.x] = at == 0x7fffffff ? -1 : at;
    }
}

__global__ void __launch_bounds__(kBlock) body_clearance_top_kernel(int nb, const double* __restrict__ bmin, const int* __restrict__ bint,
                                                                    int* __restrict__ counts) {
    __shared__ double shd[kBlock / kWave];
    __shared__ int shi[kBlock / kWave];
    double d = INFINITY;
    int idx = -1, below = 0, off = 0;
    // a thread meets its blocks in ascending order: a strict comparison keeps the lowest index
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        below += bint[b]; off += bint[(size_t)nb + b];
        const int at = bint[2 * (size_t)nb + b];
        if (at >= 0 && (idx < 0 || bmin[b] < d)) { d = bmin[b]; idx = at; }
    }
    double least;
    int at;
    least_of(d, idx, shd, shi, &least, &at);
    below = block_reduce(below, OpAdd(), shi, kBlock, 0);
    off = block_reduce(off, OpAdd(), shi, kBlock, 0);
    if (threadIdx.x == 0) { counts[0] = below; counts[1] = off; counts[2] = at == 0x7fffffff ? -1 : at; }
}

}  // namespace

Footprint::Footprint() {
    std::memset(b, 0, sizeof(b)); std::memset(rho, 0, sizeof(rho));
    if (hipGetDevice(&device) != hipSuccess) { device = -1; return; }
    if (hipMalloc((void**)&d_tab, sizeof(double) * kMax * kRow) != hipSuccess) d_tab = nullptr;
}

Footprint::~Footprint() {
    if (!d_tab) return;
    DeviceScope ds(device);
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)d_tab, (void*)d_states, (void*)d_D, (void*)d_ball, (void*)d_bmin, (void*)d_bint, (void*)d_counts}) (void)hipFree(p);
}

int Footprint::set(int dm, int cnt, const double* offset, const double* radius) {
    double tab[kMax][kRow];
    for (int j = 0; j < cnt; ++j) {
        for (int a = 0; a < 3; ++a) tab[j][a] = a < dm ? offset[(size_t)j * dm + a] : 0.0;
        tab[j][3] = radius[j];
    }
    if (cnt > 0) {
        DeviceScope ds(device);
        GPIS_HIP(hipMemcpy(d_tab, tab, sizeof(double) * (size_t)cnt * kRow, hipMemcpyHostToDevice));      // (returns when it is there)
    }
    for (int j = 0; j < cnt; ++j) {
        for (int a = 0; a < 3; ++a) b[j][a] = tab[j][a];
        rho[j] = tab[j][3];
    }
    dim = dm; m = cnt; inited = true;
    return GPIS_OK;
}

int Footprint::clearance(const DistanceField& df, const double* states, long long n, double clr, double* D_out, int* ball_out,
                         int* counts, hipStream_t s) {
    const size_t ns = (size_t)(dim + 2), nn = (size_t)n;
    const int nb = (int)((n + kBlock - 1) / kBlock);
    if (int rc = grow(d_states, cap_states, nn * ns)) return rc;
    if (nn > cap_n) {
        (void)hipFree(d_D); (void)hipFree(d_ball);
        d_D = nullptr; d_ball = nullptr; cap_n = 0;
        GPIS_HIP(hipMalloc((void**)&d_D, sizeof(double) * nn));
        GPIS_HIP(hipMalloc((void**)&d_ball, sizeof(int) * nn));
        cap_n = nn;
    }
    if ((size_t)nb > cap_b) {
        (void)hipFree(d_bmin); (void)hipFree(d_bint);
        d_bmin = nullptr; d_bint = nullptr; cap_b = 0;
        GPIS_HIP(hipMalloc((void**)&d_bmin, sizeof(double) * (size_t)nb));
        GPIS_HIP(hipMalloc((void**)&d_bint, sizeof(int) * 3 * (size_t)nb));
        cap_b = (size_t)nb;
    }
    if (!d_counts) GPIS_HIP(hipMalloc((void**)&d_counts, sizeof(int) * 3));
    GPIS_HIP(hipMemcpyAsync(d_states, states, sizeof(double) * nn * ns, hipMemcpyHostToDevice, s));
    const BodyArgs bd{d_tab, m};
    const DfLattice L = df.lattice();
    const float* F = (const float*)df.d_dist;
    if (dim == 3)
        hipLaunchKernelGGL(body_clearance_kernel<3>, dim3((unsigned)nb), dim3(kBlock), 0, s, F, L, bd, (const double*)d_states, (int)n, clr, d_D,
                           d_ball, nb, d_bmin, d_bint);
    else
        hipLaunchKernelGGL(body_clearance_kernel<2>, dim3((unsigned)nb), dim3(kBlock), 0, s, F, L, bd, (const double*)d_states, (int)n, clr, d_D,
                           d_ball, nb, d_bmin, d_bint);
    hipLaunchKernelGGL(body_clearance_top_kernel, dim3(1), dim3(kBlock), 0, s, nb, (const double*)d_bmin, (const int*)d_bint, d_counts);
    GPIS_HIP(hipGetLastError());
    if (D_out) GPIS_HIP(hipMemcpyAsync(D_out, d_D, sizeof(double) * nn, hipMemcpyDeviceToHost, s));
    if (ball_out) GPIS_HIP(hipMemcpyAsync(ball_out, d_ball, sizeof(int) * nn, hipMemcpyDeviceToHost, s));
    if (counts) GPIS_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int) * 3, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}

}  // namespace gpis
