// Device pieces shared by the path planner (plan.hip) and the pose planner (pplan.hip): the lattice descriptor, the snap of a
// world point to its lattice point, the relaxed agent-scope cost accesses of the tile kernels, and the one-workgroup scan of
// the path lengths.  Each including file gets its own copy of the scan kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace gpis {
namespace plan_dev {

struct PlanLat {
    int dim, nx, ny, nz;
    float ox, oy, oz, step;
};

__device__ __forceinline__ float ld_cost(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_cost(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lattice point of a world point: i = (int)floorf(u + 0.5f), u = (x - origin) / step; false outside the lattice or non-finite
__device__ __forceinline__ bool snap(const PlanLat& L, const float* x, int* ijk) {
    const float o[3] = {L.ox, L.oy, L.oz};
    const int n[3] = {L.nx, L.ny, L.nz};
    ijk[2] = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a < L.dim) {
            const float xa = x[a];
            const float f = floorf((xa - o[a]) / L.step + 0.5f);
            const bool in = isfinite(xa) && f >= 0.f && f <= (float)(n[a] - 1);
            ijk[a] = in ? (int)f : 0;
            ok = ok && in;
        }
    }
    return ok;
}

// in place: off[0..m) = exclusive scan of the counts, off[m] = their sum.  One workgroup.
static __global__ void __launch_bounds__(1024) plan_scan_kernel(long long* __restrict__ off, int m) {
    __shared__ long long s[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < m; base += 1024) {
        const int idx = base + tid;
        const long long v = idx < m ? off[idx] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long t = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        if (idx < m) off[idx] = s[tid] - v + carry;
        __syncthreads();
        if (tid == 1023) carry += s[1023];
        __syncthreads();
    }
    if (tid == 0) off[m] = carry;
}

}  // namespace plan_dev
}  // namespace gpis
