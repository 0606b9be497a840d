// Connected components over a compacted list of m elements: labels by min-label propagation with pointer jumping,
// the roots compacted into component indices, and the buffers of a table of 64-bit words and a box per component.  Shared by the
// coverage's frontiers (cover.hip: lattice neighbours through the rank grid) and the detector's foreign samples (detect.hip: grid
// neighbours within `link`).  "Who is my neighbour" is a device functor, int Links(int r, int best, const int* label): the least of
// `best` and ld_label over r's linked neighbours; its type belongs to the including file, as compact.h's predicates do.  Thread r
// alone writes label[r] and values only fall, so the fixed point does not depend on the schedule; the number of rounds does.
// Everything that launches is a template, and the device side sits in an unnamed namespace: a file that only holds a Components
// (through cover.h or detect.h) gets no kernel, and the two that label get kernels of their own.
#pragma once
#include <algorithm>
#include "compact.h"

namespace gpis {

constexpr int kCompMaxBatch = 64;            // labelling rounds per read-back (check_every) at most
constexpr int kCompTabWords = 8;             // 64-bit words per component of the table (their meaning is the caller's)

namespace {

__device__ __forceinline__ int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_label(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class T>
__global__ void __launch_bounds__(kCompactBlock) label_iota_kernel(T* __restrict__ label, int m) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) label[r] = r;
}

// One round: label[r] = the smallest label among r and its linked neighbours, followed down its chain of labels (a label is the
// rank of a member of the same component and never exceeds the own rank, so the chain falls and ends).
template <class Links>
__global__ void __launch_bounds__(kCompactBlock) label_round_kernel(Links links, int m, int* label, int* changed) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) {
        const int old = ld_label(label + r);
        int best = links(r, old, label);
        for (;;) {
            const int t = ld_label(label + best);
            if (t >= best) break;
            best = t;
        }
        if (best < old) { st_label(label + r, best); *changed = 1; }
    }
}

// a root of the converged labels
struct RootPred {
    const int* label;
    __device__ bool operator()(int r) const { return label[r] == r; }
};

}  // namespace

// The buffers both callers need over the m listed elements and the nc components, grow-only, with the steps that fill them.  Box:
// the 32-bit word of the per-component box (int lattice indices in cover.hip, unsigned keys of floats in detect.hip).
template <class Box>
struct Components {
    int check_every = 4;                         // schedule (the results do not depend on it)

    int* d_bcount = nullptr;   size_t cap_blocks = 0;   // per-chunk counts, then their exclusive scan and the total
    int* d_list = nullptr;                               // per listed element: its index, ascending, ...
    int* d_label = nullptr;                              // ... label as a rank, ...
    int* d_cidx = nullptr;                               // ... component index of a root (-1 elsewhere), ...
    int* d_roots = nullptr;    size_t cap_m = 0;         // ... and the roots' ranks, ascending
    unsigned long long* d_tab = nullptr;                 // kCompTabWords words per component
    Box* d_box = nullptr;      size_t cap_c = 0;         // 6 words per component: least (3), greatest (3)
    int* d_word = nullptr;                               // [0]: a labelling round changed something
    // page-locked staging of what comes back
    int* h_word = nullptr;
    unsigned long long* h_tab = nullptr;  size_t cap_htab = 0;   // nc * kCompTabWords words, then nc * 6 of box

    // the words, and the chunk counts of a compaction over n elements
    int reserve(long long n) {
        if (!d_word) GPIS_HIP(hipMalloc((void**)&d_word, sizeof(int) * 4));
        if (!h_word) GPIS_HIP(hipHostMalloc((void**)&h_word, sizeof(int) * 4));
        return grow(d_bcount, cap_blocks, (size_t)((n + kCompactChunk - 1) / kCompactChunk) + 1);
    }

    // compact_run's Grow: the per-element lists grow together, once the count is known (they are at least one element long)
    int grow_lists(int m) {
        const size_t need = (size_t)std::max(1, m);
        if (need <= cap_m) return GPIS_OK;
        for (int** p : {&d_list, &d_label, &d_cidx, &d_roots}) { (void)hipFree(*p); *p = nullptr; }
        cap_m = 0;
        for (int** p : {&d_list, &d_label, &d_cidx, &d_roots}) GPIS_HIP(hipMalloc((void**)p, sizeof(int) * need));
        cap_m = need;
        return GPIS_OK;
    }

    // label[r] = r, then rounds in batches of check_every with one read-back of d_word each, until a batch's last round changes
    // nothing.  Returns the rounds done, GPIS_ERR_LIMIT after max_rounds of them (0: m + 1), or GPIS_ERR_HIP.  Synchronises `s`.
    template <class Links>
    long long label(Links links, int m, int max_rounds, hipStream_t s) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(label_iota_kernel<int>), dim3(grid_for(m, kCompactBlock)), dim3(kCompactBlock), 0, s, d_label, m);
        GPIS_HIP(hipGetLastError());
        const long long cap = max_rounds > 0 ? (long long)max_rounds : (long long)m + 1;
        const int every = std::max(1, std::min(check_every, kCompMaxBatch));
        for (long long round = 0; round < cap;) {
            const int nbatch = (int)std::min((long long)every, cap - round);
            for (int b = 0; b < nbatch; ++b) {
                if (b == nbatch - 1) GPIS_HIP(hipMemsetAsync(d_word, 0, sizeof(int), s));   // (the batch's last round decides)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(label_round_kernel<Links>), dim3(grid_for(m, kCompactBlock)), dim3(kCompactBlock), 0, s, links,
                                   m, d_label, d_word);
                GPIS_HIP(hipGetLastError());
            }
            GPIS_HIP(hipMemcpyAsync(h_word, d_word, sizeof(int), hipMemcpyDeviceToHost, s));
            GPIS_HIP(hipStreamSynchronize(s));
            round += nbatch;
            if (h_word[0] == 0) return round;
        }
        return GPIS_ERR_LIMIT;
    }

    // the roots, ascending, into d_roots and their positions into d_cidx: component c = the c-th smallest label; *nc of them
    // (at most m: d_roots holds them, and d_bcount the chunks of m <= reserve()'s n).  Synchronises `s` (compact_run).
    int roots(int m, int* nc, hipStream_t s) {
        auto no_grow = [](int) -> int { return GPIS_OK; };
        return compact_run(RootPred{d_label}, m, d_bcount, h_word, nc, d_roots, d_cidx, s, no_grow);
    }

    int grow_table(int nc) {
        if ((size_t)nc > cap_c) {
            (void)hipFree(d_tab); (void)hipFree(d_box); d_tab = nullptr; d_box = nullptr; cap_c = 0;
            GPIS_HIP(hipMalloc((void**)&d_tab, sizeof(unsigned long long) * kCompTabWords * (size_t)nc));
            GPIS_HIP(hipMalloc((void**)&d_box, sizeof(Box) * 6 * (size_t)nc));
            cap_c = (size_t)nc;
        }
        const size_t hneed = (size_t)nc * (kCompTabWords + 3);
        if (hneed > cap_htab) {
            if (h_tab) (void)hipHostFree(h_tab);
            h_tab = nullptr; cap_htab = 0;
            GPIS_HIP(hipHostMalloc((void**)&h_tab, sizeof(unsigned long long) * hneed));
            cap_htab = hneed;
        }
        return GPIS_OK;
    }

    // d_tab into h_tab and d_box behind it (*h_box); synchronises `s`
    int fetch_table(int nc, const Box** h_box, hipStream_t s) {
        *h_box = (const Box*)(h_tab + (size_t)nc * kCompTabWords);
        GPIS_HIP(hipMemcpyAsync(h_tab, d_tab, sizeof(unsigned long long) * kCompTabWords * (size_t)nc, hipMemcpyDeviceToHost, s));
        GPIS_HIP(hipMemcpyAsync((void*)*h_box, d_box, sizeof(Box) * 6 * (size_t)nc, hipMemcpyDeviceToHost, s));
        GPIS_HIP(hipStreamSynchronize(s));
        return GPIS_OK;
    }

    // frees everything under the current device; the schedule stays
    void release() {
        for (void* p : {(void*)d_bcount, (void*)d_list, (void*)d_label, (void*)d_cidx, (void*)d_roots, (void*)d_tab, (void*)d_box, (void*)d_word})
            (void)hipFree(p);
        if (h_word) (void)hipHostFree(h_word);
        if (h_tab) (void)hipHostFree(h_tab);
        const int every = check_every;
        *this = Components();
        check_every = every;
    }
};

}  // namespace gpis
