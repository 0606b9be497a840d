// Coverage of a sensor's view on a field's lattice: one byte per lattice point, set once some integrated depth frame
// or laser scan has seen the point as free space; the frontiers of the seen space (flag, compaction, connected components by
// min-label propagation with pointer jumping, a summary table by integer atomics); and a copy of a field restricted to seen space.
// Integration gathers: one thread per lattice point reads its own byte and writes its own byte.  Every result is an integer or a
// double computed in one fixed order, so the bits are those of tests/cover_ref.py on every run.
#pragma once
#include <cstdint>
#include <vector>
#include "dev_common.h"
#include "components.h"
#include "cover_host.h"
#include "dfield_sample.h"
#include "frame.h"

namespace gpis {

struct DistanceField;

struct Coverage {
    static constexpr int kBlock = 256;           // threads of every kernel

    int device = -1;
    hipStream_t own = nullptr;

    // grow-only device buffers
    unsigned char* d_seen = nullptr;  size_t cap_n = 0;         // 1 B per lattice point
    int* d_rank = nullptr;            size_t cap_rank = 0;      // frontiers: the rank grid, 4 B per lattice point
    // the frontier points (comp.d_list: lattice indices), their components, and the table (components.h), per component the words
    // count, sums (3), d2 bits, rep, label, unused and the integer box
    Components<int> comp;
    int* d_plabel = nullptr;          size_t cap_plabel = 0;    // per frontier point: its label as a lattice index
    double* d_sector = nullptr;       size_t cap_beams = 0;     // q [m], then lim_eff [m]
    float* d_depth = nullptr;         size_t cap_pix = 0;

    // the lattice (after reset) and the last frontiers
    int dim = 0;
    int n[3] = {1, 1, 1};
    float origin[3] = {0.f, 0.f, 0.f};
    float step = 0.f;
    long long ngrid = 0;
    bool has_lattice = false, frontiers_valid = false;
    long long frames = 0, npoints = 0, ncomponents = 0, rounds = 0;
    double integrate_ms = 0.0, frontiers_ms = 0.0;
    std::vector<int> label, count, box, rep;     // the table: clusters of at least min_size points, ordered by label
    std::vector<long long> sums;

    Coverage();
    ~Coverage();
    void clear_frontiers() { frontiers_valid = false; npoints = ncomponents = rounds = 0; label.clear(); count.clear(); box.clear(); rep.clear(); sums.clear(); }
    int bind(int dev);
    DfLattice lattice() const { return DfLattice{dim, n[0], n[1], n[2], origin[0], origin[1], origin[2], step}; }
    bool same_lattice(const DistanceField& df) const;
    int reset(const DistanceField& df);                          // the field's lattice, seen = 0; moves to the field's device
    int set(const unsigned char* seen);                          // host [ngrid]; non-zero = seen
    int get(unsigned char* seen);
    // the frame's gather; in: depth [W*H] / ranges [n] (host); pose: 12 / 6 floats; synchronises `s`
    int integrate(const SensorFrame& f, const float* in, const float* pose, const CoverOpts& o, hipStream_t s);
    // GPIS_ERR_LIMIT: max_rounds exceeded (no frontiers are held then); synchronises `s`
    int frontiers(const DistanceField& df, const CoverOpts& o, hipStream_t s);
    int restrict_field(const DistanceField& in, DistanceField& out, float unseen_dist, hipStream_t s);
};

}  // namespace gpis
