// The fixed-order reductions and scans of a workgroup (64-lane wavefronts), device only and stateless.  This header is the one
// statement of "the order of a block sum" and "how a block scans": the tracker's sums, the filter's estimate and the locator's
// cost are pinned bit for bit by their tests, and they share the orders written here.  The library builds with
// -ffp-contract=off, so every caller gets the same operations and the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace gpis {

constexpr int kWave = 64;

struct OpMin { template <class T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct OpAdd { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <class T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };

// v[k] = op(v[k], v[k + h]), h = 32 .. 1 through lane shuffles; lane 0 holds the wavefront's result
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int h = kWave / 2; h >= 1; h >>= 1) v = op(v, __shfl_down(v, h, kWave));
    return v;
}

// the value of every thread of the block combined: wave_reduce per wavefront, then wave_reduce over the wavefronts' results in
// wave 0; valid in thread 0.  sh: one slot per wavefront.  nt: the block's threads
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* sh, int nt, T neutral) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave, nw = nt / kWave;
    v = wave_reduce(v, op);
    __syncthreads();                       // (sh of the previous reduction is read)
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    if (wv == 0) v = wave_reduce(lane < nw ? sh[lane] : neutral, op);
    return v;
}

// inclusive scan of one value per thread over the block of NT threads: a __shfl_up ladder per wavefront, then the sums of the
// wavefronts before the own one, in ascending order; returns it, *total = the block's sum.  sh: one slot per wavefront, free
// again on return
template <int NT, class T>
__device__ __forceinline__ T block_incl_scan(T v, T* sh, T* total) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int o = 1; o < kWave; o <<= 1) {
        const T y = __shfl_up(v, o, kWave);
        if (lane >= o) v += y;
    }
    if (lane == kWave - 1) sh[w] = v;
    __syncthreads();
    T before = 0, all = 0;
    for (int q = 0; q < NT / kWave; ++q) { if (q < w) before += sh[q]; all += sh[q]; }
    __syncthreads();
    *total = all;
    return before + v;
}

// an integer max-scan of flags: the largest thread index <= the own one whose flag is set (-1: none), *first = the smallest
// index with a set flag in the block (-1: none).  A wavefront's ballot, then the wavefronts before (after) the own one through
// sh; integers, so there is no order to fix.  sh: two slots per wavefront, free again on return.  nt: the block's threads
__device__ __forceinline__ int block_latest_flag(bool flag, int* sh, int nt, int* first) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave, nw = nt / kWave;
    const unsigned long long mask = __ballot(flag);
    const unsigned long long upto = mask & (~0ull >> (kWave - 1 - lane));
    if (lane == 0) {
        sh[2 * w] = mask ? w * kWave + (kWave - 1 - __clzll((long long)mask)) : -1;      // the wavefront's last
        sh[2 * w + 1] = mask ? w * kWave + (__ffsll((unsigned long long)mask) - 1) : -1;  // and first
    }
    __syncthreads();
    int latest = upto ? w * kWave + (kWave - 1 - __clzll((long long)upto)) : -1, fst = -1;
    for (int q = 0; q < nw && fst < 0; ++q) fst = sh[2 * q + 1];
    for (int q = w - 1; q >= 0 && latest < 0; --q) latest = sh[2 * q];
    __syncthreads();
    *first = fst;
    return latest;
}

// the halving tree a[i] += a[i + s], s = NT / 2 .. 1 over the block's NT = 256 threads -- LDS for s = 128, 64, lane shuffles of
// wave 0 below -- into part[c * P + seg]
template <int NS, int NT>
__device__ __forceinline__ void segment_reduce(double* __restrict__ a, double (*sh)[NT / 2], int tid, int seg, int nseg_pow2,
                                               double* __restrict__ part) {
    static_assert(NT == 4 * kWave, "two LDS steps, then one wavefront");
    __syncthreads();                       // (sh of the previous segment is read)
    if (tid >= NT / 2)
        for (int c = 0; c < NS; ++c) sh[c][tid - NT / 2] = a[c];
    __syncthreads();
    if (tid < NT / 2)
        for (int c = 0; c < NS; ++c) a[c] = a[c] + sh[c][tid];
    __syncthreads();
    if (tid >= NT / 4 && tid < NT / 2)
        for (int c = 0; c < NS; ++c) sh[c][tid - NT / 4] = a[c];
    __syncthreads();
    if (tid < NT / 4) {
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            double v = a[c] + sh[c][tid];
            for (int s = kWave / 2; s >= 1; s >>= 1) v = v + __shfl_down(v, s, kWave);
            if (tid == 0) part[(size_t)c * nseg_pow2 + seg] = v;
        }
    }
}

// The segment partials of ns sums reduced by the same halving tree: part[c * P + i] += part[c * P + i + s], s = P / 2 .. 1 (P a
// power of two, in place); part[c * P] = the result.  One block: every level is finished (__syncthreads) before the next
// reads it.
__device__ __forceinline__ void tree_top(int ns, int P, double* __restrict__ part) {
    for (int s = P / 2; s >= 1; s >>= 1) {
        for (int e = threadIdx.x; e < ns * s; e += blockDim.x) {
            const int c = e / s, i = e - c * s;
            double* col = part + (size_t)c * P;
            col[i] = col[i] + col[i + s];
        }
        __syncthreads();
    }
}

}  // namespace gpis
