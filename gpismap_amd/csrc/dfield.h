// Signed Euclidean distance field of the map on the device: the map's f on a lattice of cubic cells (the mesh's
// lattice), sites = lattice points with an axis edge crossing the level, an exact Euclidean distance transform by three separable
// lower-envelope passes (x, y, z), and the distance to the anchor -- a mesh vertex -- of each point's nearest site.  Sampling:
// the trilinear (2-D: bilinear) interpolant of the lattice distances and its gradient.  No atomics; the same bits on every run.
// The sign is only as good as f: unknown space (f NaN, or gated by max_var) counts as outside.
#pragma once
#include <cstdint>
#include "dev_common.h"
#include "dfield_sample.h"

namespace gpis {

class MapQuery;
class OnGPISStore;
struct Coverage;

struct DistanceField {
    static constexpr long long kMaxLattice = 1ll << 28;   // lattice points per field
    static constexpr int kMaxAxis = 16384;                // per-axis size: 3 x 16383^2 stays in int32

    int device = -1;             // buffers live here (the device current at creation; rebound to a map's device on use)
    hipStream_t own = nullptr;   // stream of the kernel-level entries when the caller passes none
    int chunk = 1 << 22;         // lattice points per test() pass (MapQuery::chunk)

    // grow-only device buffers, about 28 B per lattice point
    float* d_val = nullptr;      // f (map level)
    int* d_feat[2] = {nullptr, nullptr};  // ping-pong nearest-feature indices; the last pass's is the result's `site`
    float* d_dist = nullptr;
    int* d_ws = nullptr;         // envelope stacks of the passes: 3 ints per lattice point, slot-major over the lines
    size_t cap_n = 0;
    float* d_x = nullptr;    size_t cap_x = 0;            // per-chunk staging: lattice positions ...
    float* d_rec = nullptr;  size_t cap_rec = 0;          // ... and their test() records

    // the last result
    int dim = 0;
    int n[3] = {1, 1, 1};
    float origin[3] = {0.f, 0.f, 0.f};
    float step = 0.f;
    long long ngrid = 0;
    int site_buf = 0;            // d_feat[site_buf] holds `site`
    bool valid = false;
    bool f_valid = false;        // d_val holds the f grid (map level only)

    DistanceField();
    ~DistanceField();
    void clear_result() { valid = f_valid = false; dim = 0; ngrid = 0; }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // sites, passes and output from a device f grid (x fastest); synchronises `s`
    int from_grid(const float* d_values, int dim, const int* n, const float* origin, const float* step, float level, hipStream_t s);
    // the map-level pipeline: lattice chunks through mq into d_val (gated by max_var), then from_grid
    int from_map(MapQuery& mq, OnGPISStore& store, int dim, const int* n, const float* origin, const float* step, float level,
                 float max_var, hipStream_t s);
    // d_out[m][1 + dim] = interpolated distance and gradient at the points d_x[m][dim]; synchronises `s`
    int sample(const float* d_x, long long m, float* d_out, hipStream_t s);

    const int* d_site() const { return valid ? d_feat[site_buf] : nullptr; }
    DfLattice lattice() const { return DfLattice{dim, n[0], n[1], n[2], origin[0], origin[1], origin[2], step}; }

private:
    friend struct Coverage;      // (cover.h: the restricted copy of a field fills another field's buffers)
    int ensure(long long n);
};

// Argument check shared by the C-ABI entries: mesh_check_lattice's (GPIS_ERR_ARG / GPIS_ERR_LIMIT above 2^28 points), then a
// step that differs between axes -> GPIS_ERR_ARG, an axis above kMaxAxis -> GPIS_ERR_LIMIT.
int dfield_check_lattice(int dim, const int* n, const float* origin, const float* step, long long* npts);

}  // namespace gpis
