// Zero-level surface extraction on the device (DESIGN.md "Surface extraction"): the map's test() on a lattice, marching
// tetrahedra on the Freudenthal split of every cell, a second test() on the vertices.  Every output position comes from an
// exclusive scan of per-point / per-cell counts (no atomics), so the result is the same bits on every run.
#pragma once
#include <cstdint>
#include "dev_common.h"

namespace gpis {

class MapQuery;
class OnGPISStore;

struct MeshExtractor {
    static constexpr long long kMaxLattice = 1ll << 28;     // lattice points per extraction
    static constexpr long long kMaxCount = (1ll << 31) - 1; // vertices / primitives (int32 indices)

    int device = -1;             // buffers live here (the device current at creation; rebound to a map's device on use)
    hipStream_t own = nullptr;   // stream of the kernel-level entry when the caller passes none
    int chunk = 1 << 22;         // lattice points per test() pass (MapQuery::chunk)

    // grow-only device buffers
    float* d_val = nullptr;  uint8_t* d_mask = nullptr;  int* d_vbase = nullptr;  int* d_tbase = nullptr;  size_t cap_n = 0;
    float* d_x = nullptr;    size_t cap_x = 0;           // per-chunk staging: lattice positions ...
    float* d_rec = nullptr;  size_t cap_rec = 0;         // ... and their test() records
    long long* d_part = nullptr;                         // scan: per-block partial sums (2 x (kScanBlocks + 1))
    long long* h_tot = nullptr;                          // page-locked: [0] vertices, [1] primitives
    float* d_verts = nullptr; size_t cap_verts = 0;
    int* d_prims = nullptr;   size_t cap_prims = 0;
    float* d_vrec = nullptr;  size_t cap_vrec = 0;

    // the last result
    int dim = 0;
    long long nvert = 0, nprim = 0, ngrid = 0;
    bool grid_valid = false;     // d_val holds the lattice values of the last extraction (map level only)
    bool rec_valid = false;      // d_vrec holds the vertices' test() records (map level only)

    MeshExtractor();
    ~MeshExtractor();
    void clear_result() { nvert = nprim = ngrid = 0; grid_valid = rec_valid = false; }
    int bind(int dev);           // move to `dev` (frees the buffers of another device); GPIS_OK / GPIS_ERR_HIP
    // classification, scans, limits, vertex and primitive emission from a device value grid (x fastest); synchronises `s`
    int from_grid(const float* d_values, int dim, const int* n, const float* origin, const float* step, float level, hipStream_t s);
    // the map-level pipeline: lattice chunks through mq.run into d_val, from_grid, mq.run on the vertices into d_vrec
    int from_map(MapQuery& mq, OnGPISStore& store, int dim, const int* n, const float* origin, const float* step, float level,
                 hipStream_t s);

private:
    int ensure_grid(long long n, bool values);
    int scan(int* d, long long n, long long* part, hipStream_t s);
};

// Argument check shared by the C-ABI entries: GPIS_OK, GPIS_ERR_ARG (dim, sizes < 2, bad origin / step) or GPIS_ERR_LIMIT
// (more than kMaxLattice points).  *npts receives the lattice size.
int mesh_check_lattice(int dim, const int* n, const float* origin, const float* step, long long* npts);

// The map's f on a lattice (shared by the mesh and the distance field): chunks of at most `chunk` lattice points through
// mq.run_prepared (one mq.prepare per call) into zero-prefilled records staged in d_x / d_rec (grown here), slot 0 of each
// record into d_val[np].  A point whose var_f (record slot 1 + dim) is above max_var gets NaN (+inf: no gate).  Enqueued on `s`.
int lattice_values(MapQuery& mq, OnGPISStore& store, int dim, const int* n, const float* origin, const float* step, long long np,
                   int chunk, float max_var, float*& d_x, size_t& cap_x, float*& d_rec, size_t& cap_rec, float* d_val, hipStream_t s);

}  // namespace gpis
