// K5 + test() driver: per-query cluster lookup, device-side binning of queries by
// cluster, the evaluation passes through K4 (map_query.hip) and the variance-weighted blend.
// Reference: GPisMap3::test_kernel cpp/src/GPisMap3.cpp:794-902 and
// GPisMap::test_kernel cpp/src/GPisMap.cpp:665-763.
#pragma once
#include <vector>
#include "ongpis.h"

namespace gpis {

struct ClusterEntry {  // host description of one non-empty cluster cell (tree traversal order)
    float c[3];
    float lo[3], hi[3];
    int model;         // store slot or -1
    int parent;        // index into the ancestor table or -1
};

// Internal tree node above the cluster level.  The reference reaches a cluster cell only through
// a top-down walk that prunes on EVERY ancestor's box (octree.cpp:864-866); ancestor and child
// bounds are rounded independently, so for queries aligned with cell boundaries the ancestor test
// can fail where the cell's own test passes.  The lookup kernel therefore re-checks the chain.
struct AncestorEntry {
    float lo[3], hi[3];
    int parent;        // next ancestor or -1 (root)
};

struct ClusterTableView {
    int n;
    const float4* c;   // centre
    const float4* lo;
    const float4* hi;
    const int* model;
    const int* parent; // [n] first ancestor (index into anc_*) or -1
    const float4* anc_lo;
    const float4* anc_hi;
    const int* anc_parent;
    const int* grid;   // dense lattice: cell -> table index or -1
    int gx, gy, gz;
    double ox, oy, oz; // lattice origin (lower corner of cell 0)
    double pitch;      // cluster cell size
};

class MapQuery {
public:
    MapQuery(int dim, float search_half, float var_thre, float prior_var);
    ~MapQuery();
    // Rebuild the cluster table + lattice from the host tree (after every update()).
    int set_clusters(const std::vector<ClusterEntry>& cl, const std::vector<AncestorEntry>& anc, double pitch, hipStream_t s);
    // test(): x device [n][dim] interleaved, res device [n][2(1+dim)]; only the entries the
    // reference writes are touched.
    int run(OnGPISStore& store, const float* d_x, int n, float* d_res, hipStream_t s);
    // run() in two halves for callers that query the same models many times in a row (the renderer's march passes): prepare()
    // does run()'s per-call host work once (lazy inverses, model sync, the per-class LDS sizing); run_prepared() is every
    // pass after it and must not be separated from prepare() by a change of the models.  run() = prepare() + run_prepared().
    int prepare(OnGPISStore& store, hipStream_t s);
    int run_prepared(OnGPISStore& store, const float* d_x, int n, float* d_res, hipStream_t s);
    // box of all cluster cells of the table (lo[0..2], hi[0..2]); false when the table is empty
    bool cluster_box(float* lo, float* hi) const;
    float search_half() const { return search_half_; }
    int num_clusters() const { return ncl_; }
    // the lookup's result of the last chunk run (test probe, read-only): ncand [cap], cand [3][cap] device arrays
    void last_candidates(const int** ncand, const int** cand, int* cap) const { *ncand = d_ncand_; *cand = d_cand_; *cap = cap_n_; }
    // statistics of the last run
    long long last_evals = 0, last_flops = 0, last_touched = 0;
    // (last_flops counts the columns computed: with a prediction that includes the gradient columns of a mispredicted record,
    // which nobody reads)
    // Evaluations of the last run by kind, in every pass2_mode: pass 1; two-candidate queries' candidate 2 in full; value columns of
    // candidates 2 and 3 of three-candidate queries behind the gate; the records among those that the blend reads in full --
    // whichever pass and layout computed them
    long long last_pass_jobs[4] = {0, 0, 0, 0};
    // How pass 2 of three-candidate queries went: jobs of pass 2F with a predicted candidate, of pass 2V, of pass 2G; records pass
    // 2F computed in full that the blend did not read; predictions made (both candidates have a model), predictions read
    long long last_pass_detail[6] = {0, 0, 0, 0, 0, 0};
    float last_pick_ms = 0.f;   // time in pick_kernel (profile on)
    // the six counts, last_pick_ms and pass2_mode (the *_pass_detail entries of the C API)
    void pass_detail(double* out8) const {
        for (int k = 0; k < 6; ++k) out8[k] = (double)last_pass_detail[k];
        out8[6] = (double)last_pick_ms; out8[7] = (double)pass2_mode;
    }
    // 0 = value columns of both, then the gradient columns the blend reads (no prediction); 1 = the predicted candidate in full
    // (default); 2 / 3 = always candidate 2 / 3 in full; 4 = the prediction inverted.  Same results in every mode.  GPIS_PASS2 in
    // the environment sets the initial value.  May change between runs.
    int pass2_mode = 1;
    int last_launches = 0;      // K4 launches of the last run
    float last_eval_ms = 0.f;   // time inside the K4 launches (hipEvents on the stream)
    // queries per pass of the chunk loop; 0 = automatic (chunk_for: the whole call where the device has the memory, 2^22 under
    // k4_schedule 0).  The results do not depend on it.
    int chunk = 0;
    int last_chunk_len = 0;     // the chunk length of the last run
    // How an automatic chunk is chosen: 0 = 2^22 queries whatever the call; 1 (default) = the chunk follows the call and the
    // device's free memory, so that a pass is one K4 launch per size class over the whole call where that fits.  Same results in
    // both.  GPIS_K4_SCHEDULE in the environment sets the initial value.  May change between runs.
    int k4_schedule = 1;
    bool profile = false;
    static constexpr int kMinChunk = 1 << 22, kMaxChunk = 1 << 28;
    static size_t scratch_bytes(int n);

private:
    int chunk_for(int n);
    int ensure_scratch(int n, int nmodels);
    int run_chunk(OnGPISStore& store, const float* d_x, int n, float* d_res, hipStream_t s);
    int eval_pass(OnGPISStore& store, int njobs, int shift, int rec_base, int nmodels, hipStream_t s, int layout, int pass);
    int dim_;
    float search_half_, var_thre_, prior_var_;
    int ncl_ = 0;
    ClusterTableView tv_{};
    float box_lo_[3] = {0.f, 0.f, 0.f}, box_hi_[3] = {0.f, 0.f, 0.f};
    void* d_tab_ = nullptr; size_t cap_tab_ = 0;
    int* d_grid_ = nullptr; size_t cap_grid_ = 0;
    // per-chunk scratch
    int cap_n_ = 0, cap_models_ = 0;
    float4* d_xq_ = nullptr;
    int* d_cand_ = nullptr;     // [3][cap]
    int* d_ncand_ = nullptr;    // [cap]
    int* d_pick_ = nullptr;     // [cap] pass 2F's candidate of a three-candidate query behind the gate: 1 or 2, else 0
    int h_stat_[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the job kernels' counters of the chunk (d_tot_ + 20), as of the last binning round
    hipEvent_t evp0_ = nullptr, evp1_ = nullptr;
    int* d_jm_ = nullptr;       // [2*cap] job -> model (-1 inactive)
    int* d_jq_ = nullptr;       // [2*cap] sorted query index
    int* d_jo_ = nullptr;       // [2*cap] sorted output record
    float* d_out_ = nullptr;    // [3*cap][8]
    int* d_cnt_ = nullptr;      // [models] job count
    int* d_base_ = nullptr;     // [models]
    int* d_cursor_ = nullptr;   // [models]
    int* d_tbase_ = nullptr;    // [models]
    int* d_tile_ = nullptr;     // [3][tile_cap]
    int tile_cap_ = 0;
    int* d_tot_ = nullptr;      // [32] totals of a binning round [0..17], counters of the chunk [20..27]
    int* d_tie_ = nullptr;      // [1] queries with an exact distance tie among their nearest candidates (list: d_jq_, free at that time)
    std::vector<int> h_maxN_, h_maxLd_;   // per class: largest N and ld (LDS sizing of K4)
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    // K4 launches of one pass (one per size class, disjoint tiles and outputs) run beside each other: the first on the caller's
    // stream, the rest on side streams forked from and joined to it
    static constexpr int kSide = 3;
    hipStream_t side_[kSide] = {nullptr, nullptr, nullptr};
    hipEvent_t evfork_ = nullptr, evjoin_[kSide] = {nullptr, nullptr, nullptr};
    bool side_off_ = false;
};

}  // namespace gpis
