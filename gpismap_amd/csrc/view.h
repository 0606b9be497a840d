// Candidate viewpoints scored by the unseen space they would reveal.  For a batch of m poses: the measurement a
// sensor at each pose would make of a distance field (render.h's march through the field, one thread per ray over m x rays), the
// unseen lattice points of a coverage mask compacted into a target list (compact.h), and one gather over (target x pose) that
// applies the coverage's integration rule (cover.h) and counts.  Every result is an integer; the counts are summed by integer
// atomics, so the schedule does not reach the bits: those of tests/view_ref.py on every run, for a pose alone and in any batch.
#pragma once
#include <vector>
#include "dev_common.h"
#include "frame.h"
#include "render.h"
#include "view_host.h"

namespace gpis {

struct DistanceField;
struct Coverage;

struct ViewScorer {
    static constexpr int kBlock = 256;           // threads of every kernel
    static constexpr int kPoints = 4;            // gather: target points per thread, kBlock * kPoints per workgroup
    static constexpr int kPoseTile = 64;         // gather: poses staged in LDS at a time

    int device = -1;
    hipStream_t own = nullptr;

    // grow-only device buffers
    float* d_pose = nullptr;                size_t cap_pose = 0;     // the poses [m][12 / 6]
    int* d_hits = nullptr;                                           // per pose: rays of status 0, ...
    unsigned* d_dmax = nullptr;                                      // ... the largest valid d' (its bits), ...
    int* d_nvalid = nullptr;                                         // ... 2-D: the valid beams, ...
    double* d_lim2 = nullptr;                                        // ... 2-D: the largest lim^2 of a sector, ...
    unsigned long long* d_gain = nullptr;   size_t cap_m = 0;        // ... and the gain; [m]: the samples of the march
    float* d_pred = nullptr;                size_t cap_pred = 0;     // d' [m][rays]
    double* d_csq = nullptr;                                         // 2-D: (c, s) of every beam [2 n], then their q [n]
    int* d_ord = nullptr;                   size_t cap_beams = 0;    // 2-D: the beams ordered by q
    int* d_sel = nullptr;                                            // 2-D, per pose: its valid beams in that order, ...
    double* d_sector = nullptr;             size_t cap_sector = 0;   // ... q [m][rays], then lim_eff [m][rays]
    int* d_bcount = nullptr;                size_t cap_blocks = 0;   // target compaction: chunk counts / offsets
    int* d_list = nullptr;                  size_t cap_list = 0;     // the targets' lattice indices, ascending
    // page-locked staging
    float* h_pose = nullptr;                size_t cap_hpose = 0;
    char* h_out = nullptr;                  size_t cap_hout = 0;     // gain [m] (and the samples), then hits [m]
    int* h_word = nullptr;

    // the last result
    bool valid = false;
    int dim = 0;
    long long poses = 0, rays = 0, targets = 0, samples = 0;
    double predict_ms = 0.0, table_ms = 0.0, target_ms = 0.0, gather_ms = 0.0;
    std::vector<long long> gain;
    std::vector<int> hits;

    ViewScorer();
    ~ViewScorer();
    void clear_result() { valid = false; dim = 0; poses = rays = targets = samples = 0; predict_ms = table_ms = target_ms = gather_ms = 0.0; gain.clear(); hits.clear(); }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // The whole call; synchronises `s`.  pose: m x 12 / 6 floats (host).  Arguments are checked by the caller (view_check_tail,
    // render_field_check_opts, view_check_batch, finite poses); field and coverage share a lattice on this device.  On an error
    // the holder holds no result.
    int score(const DistanceField& df, const Coverage& cv, const SensorFrame& f, const float* pose, int m, const gpis_view_opts& o,
              hipStream_t s);
    int predicted(int k, float* out);            // d' of pose k of the held result (host [rays])
};

}  // namespace gpis
