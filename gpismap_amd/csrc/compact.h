// Order-keeping compaction of the elements of [0, n) that pass a predicate: count, scan, write over chunks of kCompactChunk
// elements (the passing elements come out ascending), no atomics.  Device templates and their host driver, used by the coverage's
// frontier points (cover.hip), the detector's foreign samples (detect.hip), the view scorer's targets (view.hip) and the roots of
// the labels (components.h).  A predicate is a device functor bool(int); its type belongs to the including file, so every file
// instantiates kernels of its own, and a file that compacts nothing gets none: every kernel here is a template.
#pragma once
#include "dev_common.h"
#include "block_ops.h"

namespace gpis {

constexpr int kCompactBlock = 256;           // threads of the three kernels, and the width of both scans
constexpr int kCompactItems = 8;             // elements per thread
constexpr int kCompactChunk = kCompactBlock * kCompactItems;

template <class Pred>
__global__ void __launch_bounds__(kCompactBlock) compact_count_kernel(Pred pred, int n, int* __restrict__ bcount) {
    const int base = blockIdx.x * kCompactChunk;
    int cnt = 0;
    for (int it = 0; it < kCompactItems; ++it) {
        const int p = base + it * kCompactBlock + threadIdx.x;
        cnt += __syncthreads_count(p < n && pred(p));
    }
    if (threadIdx.x == 0) bcount[blockIdx.x] = cnt;
}

// in place: b[0..nb) = exclusive scan of the counts, b[nb] = their sum.  One workgroup.
namespace {
template <class T>
__global__ void __launch_bounds__(kCompactBlock) compact_offsets_kernel(T* __restrict__ b, int nb) {
    __shared__ T sh[kCompactBlock / kWave];
    T carry = 0;
    for (int base = 0; base < nb; base += kCompactBlock) {
        const int idx = base + threadIdx.x;
        const T v = idx < nb ? b[idx] : 0;
        T total;
        const T incl = block_incl_scan<kCompactBlock, T>(v, sh, &total);
        if (idx < nb) b[idx] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) b[nb] = carry;
}
}  // namespace

// list[off ..] = the elements of this chunk that pass, ascending; rank[p] = the position of p in the list, -1 if it fails
// (rank may be null: the list alone)
template <class Pred>
__global__ void __launch_bounds__(kCompactBlock) compact_write_kernel(Pred pred, int n, const int* __restrict__ boff, int* __restrict__ list,
                                                                    int* __restrict__ rank) {
    __shared__ int sh[kCompactBlock / kWave];
    const int base = blockIdx.x * kCompactChunk;
    int off = boff[blockIdx.x];
    for (int it = 0; it < kCompactItems; ++it) {
        const int p = base + it * kCompactBlock + threadIdx.x;
        const int f = (p < n && pred(p)) ? 1 : 0;
        int total;
        const int incl = block_incl_scan<kCompactBlock, int>(f, sh, &total);
        if (p < n) {
            const int r = off + incl - 1;
            if (f) list[r] = p;
            if (rank) rank[p] = f ? r : -1;
        }
        off += total;
    }
}

// count, scan, write of the elements of [0, n) that pass pred: *total of them, ascending in d_list (grow_lists(total) makes room
// once the count is known), their positions in d_rank (null: not kept); d_bcount: ceil(n / kCompactChunk) + 1 ints; h_word: one
// page-locked int; synchronises `s` after the scan.  n = 0: nothing is launched, *total = 0
template <class Pred, class Grow>
int compact_run(Pred pred, int n, int* d_bcount, int* h_word, int* total, int*& d_list, int*& d_rank, hipStream_t s, const Grow& grow_lists) {
    *total = 0;
    if (n <= 0) return grow_lists(0);
    const int nb = (n + kCompactChunk - 1) / kCompactChunk;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(compact_count_kernel<Pred>), dim3(nb), dim3(kCompactBlock), 0, s, pred, n, d_bcount);
    GPIS_HIP(hipGetLastError());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(compact_offsets_kernel<int>), dim3(1), dim3(kCompactBlock), 0, s, d_bcount, nb);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(h_word, d_bcount + nb, sizeof(int), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    *total = h_word[0];
    if (int rc = grow_lists(*total)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(compact_write_kernel<Pred>), dim3(nb), dim3(kCompactBlock), 0, s, pred, n, d_bcount, d_list, d_rank);
    GPIS_HIP(hipGetLastError());
    return GPIS_OK;
}

}  // namespace gpis
