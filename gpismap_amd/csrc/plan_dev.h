// The device side of the solver's rule, defined once for the path planner (plan.hip) and the pose planner (pplan.hip): the
// lattice descriptor PlanLat and snap(); point_cost(); the 27 offsets off_dx() .. off_nnz(); the statistics words kStat*; the
// relaxed agent-scope cost accesses ld_cost() / st_cost(); tile_begin() / note_border() / tile_finish(), the flag protocol around
// a tile kernel's own relaxation loop; better_move(), the policy's choice and tie-break; counts_begin() / commit_counts(), the
// counts of a policy kernel; and plan_scan_kernel, the one-workgroup scan of the path lengths (launched by plan_host.h; each
// including file gets its own copy).  The tiles, the move sets and the relaxation loops are the planners' own.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "plan.h"

namespace gpis {
namespace plan_dev {

struct PlanLat {
    int dim, nx, ny, nz;
    float ox, oy, oz, step;
};

// words of a handle's d_stat; kStatFree2 .. kStatMax2 are the pose planner's projection; one raised word per round of a batch
enum { kStatKept = 0, kStatLaunch, kStatFree, kStatReach, kStatMax, kStatFree2, kStatReach2, kStatMax2, kStatRaised,
       kStatWords = kStatRaised + PlanSchedule::kMaxBatch };

// direction index of the offset (dx, dy, dz): ((dz + 1) 3 + (dy + 1)) 3 + (dx + 1); 13 is "stay", 9 .. 17 have dz = 0
constexpr int off_dx(int k) { return k % 3 - 1; }
constexpr int off_dy(int k) { return (k / 3) % 3 - 1; }
constexpr int off_dz(int k) { return k / 9 - 1; }
constexpr int off_nnz(int k) { return (off_dx(k) != 0) + (off_dy(k) != 0) + (off_dz(k) != 0); }

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

// the point cost of the distance d: 0 = not free (d < clearance or NaN), else 1 + gain t^2 with t falling from 1 to 0 over margin
__device__ __forceinline__ float point_cost(float d, float clearance, float margin, float gain) {
    float cc = 0.f;
    if (d >= clearance) {
        cc = 1.f;
        if (margin > 0.f) {
            const float t = fmaxf(0.f, margin - (d - clearance)) / margin;
            cc = 1.f + gain * (t * t);
        }
    }
    return cc;
}

// the policy's choice among the open moves: the smaller value v, then the smaller cost cq of the move's end, then (the callers
// offer the moves by rising code) the smaller code
__device__ __forceinline__ void better_move(float v, float cq, int code, float& best, float& bestq, unsigned char& pol) {
    if (v < best || (v == best && cq < bestq)) { best = v; bestq = cq; pol = (unsigned char)code; }
}

// The counts of a policy kernel.  counts_begin() opens the kernel: thread 0 zeroes the block's three LDS words, then a barrier.
// commit_counts() closes it: the block's sums of nf and nr are added to stat3[0] and stat3[1], the largest mx is maxed into
// stat3[2] (the bits of a non-negative float order as the float does).
__device__ __forceinline__ void counts_begin(unsigned* s3) {
    if (threadIdx.x == 0) { s3[0] = 0; s3[1] = 0; s3[2] = 0; }
    __syncthreads();
}
__device__ __forceinline__ void commit_counts(unsigned* s3, unsigned nf, unsigned nr, unsigned mx, unsigned long long* stat3) {
    atomicAdd(&s3[0], nf);
    atomicAdd(&s3[1], nr);
    atomicMax(&s3[2], mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&stat3[0], (unsigned long long)s3[0]);
        atomicAdd(&stat3[1], (unsigned long long)s3[1]);
        atomicMax(&stat3[2], (unsigned long long)s3[2]);
    }
}

// Start of a tile kernel: thread 0 takes and clears the tile's flag of this round; false: the tile is idle, the workgroup leaves
__device__ __forceinline__ bool tile_begin(int* flags_cur, int tile, int& s_act, unsigned& s_nbr) {
    if (threadIdx.x == 0) {
        s_act = flags_cur[tile];
        if (s_act) flags_cur[tile] = 0;
        s_nbr = 0;
    }
    __syncthreads();
    return s_act != 0;
}

// A thread that lowered a point on the tile's border notes the neighbour tiles whose halo holds it: mx / my / mz have bit 1
// set, bit 0 at the tile's low border along that axis and bit 2 at its high border (mz = 2: no z neighbours); s_nbr gets the bit
// of every offset towards such a tile
__device__ __forceinline__ void note_border(unsigned& s_nbr, int li, int lj, int lk, int t, int tz) {
    const unsigned mx = 2u | (li == 0 ? 1u : 0u) | (li == t - 1 ? 4u : 0u);
    const unsigned my = 2u | (lj == 0 ? 1u : 0u) | (lj == t - 1 ? 4u : 0u);
    const unsigned mz = tz == 0 ? 2u : (2u | (lk == 0 ? 1u : 0u) | (lk == tz - 1 ? 4u : 0u));
    if ((mx | my | mz) != 2u) {
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < 27; ++k)
            if (k != 13 && ((mx >> (k % 3)) & (my >> ((k / 3) % 3)) & (mz >> (k / 9)) & 1u)) bits |= 1u << k;
        atomicOr(&s_nbr, bits);
    }
}

// End of a tile kernel, after the lowered points are stored and noted.  Raises the NEXT round's flag of every neighbour tile
// noted that lies in the tile lattice (all_dirs = false: only across a face) and the tile's own at the cap, counts the flags
// raised in *raised and the launch in stat.
__device__ __forceinline__ void tile_finish(const unsigned& s_nbr, bool capped, bool all_dirs, int tile, int ti, int tj, int tk, int tnx,
                                            int tny, int tnz, int* flags_next, unsigned long long* stat, unsigned long long* raised) {
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 27 && tid != 13 && ((s_nbr >> tid) & 1u) && (all_dirs || off_nnz(tid) == 1)) {
        const int ni = ti + off_dx(tid), nj = tj + off_dy(tid), nk = tk + off_dz(tid);
        if (ni >= 0 && ni < tnx && nj >= 0 && nj < tny && nk >= 0 && nk < tnz) {
            flags_next[(nk * tny + nj) * tnx + ni] = 1;
            atomicAdd(raised, 1ull);
        }
    }
    if (tid == 32) {
        if (capped) { flags_next[tile] = 1; atomicAdd(raised, 1ull); }
        atomicAdd(&stat[kStatLaunch], 1ull);
    }
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
