// Zero-level surface extraction (mesh.h; DESIGN.md "Surface extraction").  Memory-bound passes of a few bytes per lattice
// point: grid-stride loops over at most kGridCap blocks of 256 threads (cdna_hip_programming.md Guideline 11), the scans read
// and write 16 B per lane (Guideline 13).
//
// Lattice point (i, j, k): index p = (k ny + j) nx + i, coordinates o + (float)i * s per axis (no FMA: -ffp-contract=off).
// Inside iff f < level.  Edges of the Freudenthal split run from p to p + d, d a non-zero 0/1 vector numbered x + 2y + 4z;
// crossed iff both ends are finite and exactly one is inside.  mask[p] bit d-1 = edge (p, d) crossed; vertex of that edge =
// vbase[p] + popcount(mask[p] & ((1 << (d-1)) - 1)), vbase the exclusive scan of popcount(mask).  Primitive positions: the
// exclusive scan of the per-cell counts.
#include <algorithm>
#include <cmath>
#include "map_query.h"
#include "mesh.h"
#include "block_ops.h"

namespace gpis {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlocks = 2048;     // partial sums per scan
constexpr int kTile = kBlock * 4;     // scan elements per block iteration (one int4 per lane)

// Kuhn tetrahedra 0 -> e_a -> e_a + e_b -> (1,1,1) as corner bit sets (bit a = +e_a), axis orders xyz, xzy, yxz, yzx, zxy, zyx,
// and the sign of each order as a permutation (= the sign of the tetrahedron's volume).
__constant__ unsigned char c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ signed char c_tet_sign[6] = {1, -1, -1, 1, 1, -1};
// the two triangles of a square: 0 -> e_x -> (1,1) (positive), 0 -> e_y -> (1,1) (negative)
__constant__ unsigned char c_tri[2][3] = {{0, 1, 3}, {0, 2, 3}};
__constant__ signed char c_tri_sign[2] = {1, -1};

__device__ __forceinline__ long long corner_off(int cb, int nx, long long nxy) {
    return (long long)(cb & 1) + ((cb >> 1) & 1) * (long long)nx + ((cb >> 2) & 1) * nxy;
}

// finite / inside bits of the 2^dim corners of the cell at (i, j, k); corners outside the lattice are neither
__device__ __forceinline__ void corner_flags(const float* __restrict__ val, long long p, int i, int j, int k, int dim, int nx, int ny,
                                             int nz, long long nxy, float level, unsigned& fin, unsigned& ins) {
    fin = 0; ins = 0;
    const int nc = 1 << dim;
    for (int c = 0; c < nc; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
        if (i + dx >= nx || j + dy >= ny || k + dz >= nz) continue;
        const float f = val[p + corner_off(c, nx, nxy)];
        if (isfinite(f)) { fin |= 1u << c; if (f < level) ins |= 1u << c; }
    }
}

__global__ void __launch_bounds__(kBlock) mesh_lattice_kernel(long long off, int len, int dim, int nx, int ny, float ox, float oy,
                                                              float oz, float sx, float sy, float sz, float* __restrict__ x) {
    const long long nxy = (long long)nx * ny;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < len; q += gridDim.x * blockDim.x) {
        const long long p = off + q;
        const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / nxy);
        float* o = x + (size_t)q * dim;
        o[0] = ox + (float)i * sx;
        o[1] = oy + (float)j * sy;
        if (dim == 3) o[2] = oz + (float)k * sz;
    }
}

// slot 0 (f) of a chunk's test() records into the value grid; NaN where var_f (slot vs) is above max_var
__global__ void __launch_bounds__(kBlock) mesh_fcol_kernel(const float* __restrict__ rec, int nc, int vs, float max_var, int len,
                                                           float* __restrict__ val) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < len; q += gridDim.x * blockDim.x) {
        const float* r = rec + (size_t)q * nc;
        val[q] = r[vs] > max_var ? __int_as_float(0x7fc00000) : r[0];
    }
}

// crossing mask and vertex count per point, primitive count per cell
__global__ void __launch_bounds__(kBlock) mesh_classify_kernel(const float* __restrict__ val, int dim, int nx, int ny, int nz,
                                                               float level, uint8_t* __restrict__ mask, int* __restrict__ vcnt,
                                                               int* __restrict__ tcnt) {
    const long long nxy = (long long)nx * ny, n = nxy * nz;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / nxy);
        unsigned fin, ins;
        corner_flags(val, p, i, j, k, dim, nx, ny, nz, nxy, level, fin, ins);
        unsigned m = 0;
        if (fin & 1u) {
            const int nd = (1 << dim) - 1;
            for (int d = 1; d <= nd; ++d)
                if (((fin >> d) & 1u) && (((ins >> d) ^ ins) & 1u)) m |= 1u << (d - 1);
        }
        int t = 0;
        if (i < nx - 1 && j < ny - 1 && (dim == 2 || k < nz - 1)) {
            if (dim == 3) {
                for (int s = 0; s < 6; ++s) {
                    const unsigned cm = (1u << c_tet[s][0]) | (1u << c_tet[s][1]) | (1u << c_tet[s][2]) | (1u << c_tet[s][3]);
                    if ((fin & cm) != cm) continue;
                    const int nin = __popc(ins & cm);
                    t += (nin == 2) ? 2 : ((nin & 1) ? 1 : 0);
                }
            } else {
                for (int s = 0; s < 2; ++s) {
                    const unsigned cm = (1u << c_tri[s][0]) | (1u << c_tri[s][1]) | (1u << c_tri[s][2]);
                    if ((fin & cm) != cm) continue;
                    const int nin = __popc(ins & cm);
                    t += (nin == 1 || nin == 2) ? 1 : 0;
                }
            }
        }
        mask[p] = (uint8_t)m;
        vcnt[p] = __popc(m);
        tcnt[p] = t;
    }
}

// ---- deterministic exclusive scan: per-block sums, one block over the sums, per-block rescan ----------------------------------
// Block b owns elements [b * seg, min(n, (b + 1) * seg)), seg a multiple of kTile; the block walks its range in tiles of kTile;
// a tile is scanned by block_ops.h: block_incl_scan.
__device__ __forceinline__ int4 load4(const int* __restrict__ a, long long e, long long n) {
    if (e + 4 <= n) return *reinterpret_cast<const int4*>(a + e);
    int4 v = make_int4(0, 0, 0, 0);
    if (e < n) v.x = a[e];
    if (e + 1 < n) v.y = a[e + 1];
    if (e + 2 < n) v.z = a[e + 2];
    return v;
}

__global__ void __launch_bounds__(kBlock) mesh_scan_partial_kernel(const int* __restrict__ a, long long n, long long seg,
                                                              long long* __restrict__ part) {
    __shared__ long long sh[kBlock / 64];
    const long long lo = (long long)blockIdx.x * seg, hi = std::min(n, lo + seg);
    long long acc = 0;
    for (long long t = lo; t < hi; t += kTile) {
        const int4 v = load4(a, t + 4ll * threadIdx.x, hi);
        acc += (long long)v.x + v.y + v.z + v.w;
    }
    long long tot;
    (void)block_incl_scan<kBlock>(acc, sh, &tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// exclusive prefix of the nb (<= 2 * 1024) partial sums in place; part[nb] = the grand total
__global__ void __launch_bounds__(1024) mesh_scan_top_kernel(long long* __restrict__ part, int nb) {
    __shared__ long long sh[1024 / 64];
    const int e = 2 * threadIdx.x;
    const long long a = e < nb ? part[e] : 0, b = e + 1 < nb ? part[e + 1] : 0;
    long long tot;
    const long long inc = block_incl_scan<1024>(a + b, sh, &tot);
    if (e < nb) part[e] = inc - a - b;
    if (e + 1 < nb) part[e + 1] = inc - b;
    if (threadIdx.x == 0) part[nb] = tot;
}

__global__ void __launch_bounds__(kBlock) mesh_scan_apply_kernel(int* __restrict__ a, long long n, long long seg,
                                                            const long long* __restrict__ part) {
    __shared__ long long sh[kBlock / 64];
    const long long lo = (long long)blockIdx.x * seg, hi = std::min(n, lo + seg);
    long long carry = part[blockIdx.x];
    for (long long t = lo; t < hi; t += kTile) {
        const long long e = t + 4ll * threadIdx.x;
        const int4 v = load4(a, e, hi);
        const long long s4 = (long long)v.x + v.y + v.z + v.w;
        long long tot;
        const long long ex = carry + block_incl_scan<kBlock>(s4, sh, &tot) - s4;
        // (values past 2^31 - 1 wrap: the host refuses such totals before anything reads them)
        const int4 o = make_int4((int)ex, (int)(ex + v.x), (int)(ex + v.x + v.y), (int)(ex + v.x + v.y + v.z));
        if (e + 4 <= hi) {
            *reinterpret_cast<int4*>(a + e) = o;
        } else {
            if (e < hi) a[e] = o.x;
            if (e + 1 < hi) a[e + 1] = o.y;
            if (e + 2 < hi) a[e + 2] = o.z;
        }
        carry += tot;
    }
}

// ---- emission ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_vertex_kernel(const float* __restrict__ val, int dim, int nx, int ny, int nz,
                                                             float ox, float oy, float oz, float sx, float sy, float sz, float level,
                                                             const uint8_t* __restrict__ mask, const int* __restrict__ vbase,
                                                             float* __restrict__ verts) {
    const long long nxy = (long long)nx * ny, n = nxy * nz;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const unsigned m = mask[p];
        if (!m) continue;
        const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / nxy);
        const float fa = val[p];
        const float ax = ox + (float)i * sx, ay = oy + (float)j * sy, az = oz + (float)k * sz;
        long long v = vbase[p];
        for (int d = 1; d < 8; ++d) {
            if (!((m >> (d - 1)) & 1u)) continue;
            const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            const float fb = val[p + corner_off(d, nx, nxy)];
            const float t = (level - fa) / (fb - fa);
            const float bx = ox + (float)(i + dx) * sx, by = oy + (float)(j + dy) * sy;
            float* o = verts + (size_t)v * dim;
            o[0] = ax + t * (bx - ax);
            o[1] = ay + t * (by - ay);
            if (dim == 3) {
                const float bz = oz + (float)(k + dz) * sz;
                o[2] = az + t * (bz - az);
            }
            ++v;
        }
    }
}

// vertex index of the simplex edge between corners u and w (bit sets, one a subset of the other) of the cell at p
__device__ __forceinline__ int edge_vertex(int u, int w, long long p, int nx, long long nxy, const uint8_t* __restrict__ mask,
                                           const int* __restrict__ vbase) {
    const int lo = u & w, d = u ^ w;
    const long long q = p + corner_off(lo, nx, nxy);
    return vbase[q] + __popc((unsigned)mask[q] & ((1u << (d - 1)) - 1u));
}

__device__ __forceinline__ void put_tri(int* __restrict__ prims, long long& slot, int a, int b, int c) {
    // rotated so that the smallest index comes first (keeps the winding)
    int r0 = a, r1 = b, r2 = c;
    if (b < a && b < c) { r0 = b; r1 = c; r2 = a; }
    else if (c < a && c < b) { r0 = c; r1 = a; r2 = b; }
    int* o = prims + (size_t)slot * 3;
    o[0] = r0; o[1] = r1; o[2] = r2;
    ++slot;
}

// Winding from the simplex's sign and the permutation parity: for a positively oriented tetrahedron (c0, c1, c2, c3), the
// triangle on the edges (L, j1), (L, j2), (L, j3) (j ascending) faces away from corner L iff (-1)^L > 0, and the quad
// (i1,o1), (i1,o2), (i2,o2), (i2,o1) faces from {i1, i2} to {o1, o2} iff the permutation (i1, i2, o1, o2) is even.
__global__ void __launch_bounds__(kBlock) mesh_prim_kernel(const float* __restrict__ val, int dim, int nx, int ny, int nz, float level,
                                                           const uint8_t* __restrict__ mask, const int* __restrict__ vbase,
                                                           const int* __restrict__ tbase, int* __restrict__ prims) {
    const long long nxy = (long long)nx * ny, n = nxy * nz;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p + 1 < n; p += (long long)gridDim.x * blockDim.x) {
        long long slot = tbase[p];
        if (tbase[p + 1] == slot) continue;           // (the last point is never a cell)
        const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / nxy);
        unsigned fin, ins;
        corner_flags(val, p, i, j, k, dim, nx, ny, nz, nxy, level, fin, ins);
        if (dim == 2) {
            for (int s = 0; s < 2; ++s) {
                const int c[3] = {c_tri[s][0], c_tri[s][1], c_tri[s][2]};
                if (((fin >> c[0]) & (fin >> c[1]) & (fin >> c[2]) & 1u) == 0) continue;
                const int in[3] = {(int)((ins >> c[0]) & 1u), (int)((ins >> c[1]) & 1u), (int)((ins >> c[2]) & 1u)};
                const int nin = in[0] + in[1] + in[2];
                if (nin == 0 || nin == 3) continue;
                int L = 0;
                for (int q = 0; q < 3; ++q) if (in[q] == (nin == 1)) L = q;
                const int j1 = L == 0 ? 1 : 0, j2 = L == 2 ? 1 : 2;
                const int par = (L & 1) ? -1 : 1;
                const bool fwd = (nin == 1) ? (c_tri_sign[s] * par > 0) : (c_tri_sign[s] * par < 0);
                const int va = edge_vertex(c[L], c[j1], p, nx, nxy, mask, vbase);
                const int vb = edge_vertex(c[L], c[j2], p, nx, nxy, mask, vbase);
                int* o = prims + (size_t)slot * 2;
                o[0] = fwd ? va : vb; o[1] = fwd ? vb : va;
                ++slot;
            }
            continue;
        }
        for (int s = 0; s < 6; ++s) {
            const int c[4] = {c_tet[s][0], c_tet[s][1], c_tet[s][2], c_tet[s][3]};
            if (((fin >> c[0]) & (fin >> c[1]) & (fin >> c[2]) & (fin >> c[3]) & 1u) == 0) continue;
            int code = 0;
            for (int q = 0; q < 4; ++q) code |= (int)((ins >> c[q]) & 1u) << q;
            const int nin = __popc((unsigned)code);
            if (nin == 0 || nin == 4) continue;
            const int sg = c_tet_sign[s];
            if (nin != 2) {
                int L = 0;
                for (int q = 0; q < 4; ++q) if (((code >> q) & 1) == (nin == 1)) L = q;
                int jj[3], r = 0;
                for (int q = 0; q < 4; ++q) if (q != L) jj[r++] = q;
                const int par = (L & 1) ? -1 : 1;
                const bool fwd = (nin == 1) ? (sg * par > 0) : (sg * par < 0);
                const int v0 = edge_vertex(c[L], c[jj[0]], p, nx, nxy, mask, vbase);
                const int v1 = edge_vertex(c[L], c[jj[1]], p, nx, nxy, mask, vbase);
                const int v2 = edge_vertex(c[L], c[jj[2]], p, nx, nxy, mask, vbase);
                if (fwd) put_tri(prims, slot, v0, v1, v2);
                else put_tri(prims, slot, v0, v2, v1);
            } else {
                int I[2], O[2], a = 0, b = 0;
                for (int q = 0; q < 4; ++q) { if ((code >> q) & 1) I[a++] = q; else O[b++] = q; }
                // parity of (i1, i2, o1, o2): odd for the inside pairs {0,2} and {1,3}
                const int par = ((I[0] == 0 && I[1] == 2) || (I[0] == 1 && I[1] == 3)) ? -1 : 1;
                int q4[4] = {edge_vertex(c[I[0]], c[O[0]], p, nx, nxy, mask, vbase), edge_vertex(c[I[0]], c[O[1]], p, nx, nxy, mask, vbase),
                             edge_vertex(c[I[1]], c[O[1]], p, nx, nxy, mask, vbase), edge_vertex(c[I[1]], c[O[0]], p, nx, nxy, mask, vbase)};
                if (sg * par < 0) { const int t = q4[1]; q4[1] = q4[3]; q4[3] = t; }     // reversed cycle
                int m0 = 0;
                for (int q = 1; q < 4; ++q) if (q4[q] < q4[m0]) m0 = q;
                const int a0 = q4[m0], a1 = q4[(m0 + 1) & 3], a2 = q4[(m0 + 2) & 3], a3 = q4[(m0 + 3) & 3];
                // diagonal through the smallest index; the two triangles in lexicographic order
                if (a1 < a2) { put_tri(prims, slot, a0, a1, a2); put_tri(prims, slot, a0, a2, a3); }
                else { put_tri(prims, slot, a0, a2, a3); put_tri(prims, slot, a0, a1, a2); }
            }
        }
    }
}

}  // namespace

int mesh_check_lattice(int dim, const int* n, const float* origin, const float* step, long long* npts) {
    if ((dim != 2 && dim != 3) || !n || !origin || !step) return GPIS_ERR_ARG;
    long long tot = 1;
    bool big = false;
    for (int a = 0; a < dim; ++a) {
        if (n[a] < 2 || !std::isfinite(origin[a]) || !std::isfinite(step[a]) || !(step[a] > 0.f)) return GPIS_ERR_ARG;
        if (tot > MeshExtractor::kMaxLattice / n[a]) big = true;
        else tot *= n[a];
    }
    if (big || tot > MeshExtractor::kMaxLattice) return GPIS_ERR_LIMIT;
    if (npts) *npts = tot;
    return GPIS_OK;
}

int lattice_values(MapQuery& mq, OnGPISStore& store, int dm, const int* n, const float* origin, const float* step, long long np,
                   int chunk, float max_var, float*& d_x, size_t& cap_x, float*& d_rec, size_t& cap_rec, float* d_val, hipStream_t s) {
    const int nc = 2 * (1 + dm);
    const int C = (int)std::min<long long>(std::max(1, chunk), np);
    if (int rc = grow(d_x, cap_x, (size_t)C * dm)) return rc;
    if (int rc = grow(d_rec, cap_rec, (size_t)C * nc)) return rc;
    if (int rc = mq.prepare(store, s)) return rc;
    const float oz = dm == 3 ? origin[2] : 0.f, sz = dm == 3 ? step[2] : 0.f;
    for (long long off = 0; off < np; off += C) {
        const int len = (int)std::min<long long>(C, np - off);
        hipLaunchKernelGGL(mesh_lattice_kernel, dim3(grid_for(len)), dim3(kBlock), 0, s, off, len, dm, n[0], n[1], origin[0], origin[1], oz,
                           step[0], step[1], sz, d_x);
        GPIS_HIP(hipGetLastError());
        GPIS_HIP(hipMemsetAsync(d_rec, 0, sizeof(float) * (size_t)len * nc, s));   // (the mex gateway's zero pre-fill)
        if (int rc = mq.run_prepared(store, d_x, len, d_rec, s)) return rc;
        hipLaunchKernelGGL(mesh_fcol_kernel, dim3(grid_for(len)), dim3(kBlock), 0, s, d_rec, nc, 1 + dm, max_var, len, d_val + off);
        GPIS_HIP(hipGetLastError());
    }
    return GPIS_OK;
}

MeshExtractor::MeshExtractor() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

MeshExtractor::~MeshExtractor() { (void)bind(-1); }

int MeshExtractor::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_val, (void*)d_mask, (void*)d_vbase, (void*)d_tbase, (void*)d_x, (void*)d_rec, (void*)d_part,
                        (void*)d_verts, (void*)d_prims, (void*)d_vrec})
            (void)hipFree(p);
        if (h_tot) (void)hipHostFree(h_tot);
        if (own) (void)hipStreamDestroy(own);
    }
    d_val = nullptr; d_mask = nullptr; d_vbase = nullptr; d_tbase = nullptr; d_x = nullptr; d_rec = nullptr; d_part = nullptr;
    d_verts = nullptr; d_prims = nullptr; d_vrec = nullptr; h_tot = nullptr; own = nullptr;
    cap_n = cap_x = cap_rec = cap_verts = cap_prims = cap_vrec = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int MeshExtractor::ensure_grid(long long n, bool values) {
    const size_t need = (size_t)((n + 3) & ~3ll);       // (whole int4 groups for the scans)
    if (need > cap_n || (values && !d_val)) {
        for (void* p : {(void*)d_val, (void*)d_mask, (void*)d_vbase, (void*)d_tbase}) (void)hipFree(p);
        d_val = nullptr; d_mask = nullptr; d_vbase = nullptr; d_tbase = nullptr; cap_n = 0;
        const size_t c = std::max(need, cap_n);
        if (values) GPIS_HIP(hipMalloc((void**)&d_val, sizeof(float) * c));
        GPIS_HIP(hipMalloc((void**)&d_mask, c));
        GPIS_HIP(hipMalloc((void**)&d_vbase, sizeof(int) * c));
        GPIS_HIP(hipMalloc((void**)&d_tbase, sizeof(int) * c));
        cap_n = c;
    }
    if (!d_part) GPIS_HIP(hipMalloc((void**)&d_part, sizeof(long long) * 2 * (kScanBlocks + 1)));
    if (!h_tot) GPIS_HIP(hipHostMalloc((void**)&h_tot, sizeof(long long) * 2));
    return GPIS_OK;
}

int MeshExtractor::scan(int* d, long long n, long long* part, hipStream_t s) {
    const long long per = (n + kScanBlocks - 1) / kScanBlocks;
    const long long seg = std::max((long long)kTile, (per + kTile - 1) / kTile * kTile);
    const int nb = (int)((n + seg - 1) / seg);
    hipLaunchKernelGGL(mesh_scan_partial_kernel, dim3(nb), dim3(kBlock), 0, s, d, n, seg, part);
    hipLaunchKernelGGL(mesh_scan_top_kernel, dim3(1), dim3(1024), 0, s, part, nb);
    hipLaunchKernelGGL(mesh_scan_apply_kernel, dim3(nb), dim3(kBlock), 0, s, d, n, seg, part);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipMemcpyAsync(part == d_part ? h_tot : h_tot + 1, part + nb, sizeof(long long), hipMemcpyDeviceToHost, s));
    return GPIS_OK;
}

int MeshExtractor::from_grid(const float* d_values, int dm, const int* n, const float* origin, const float* step, float level,
                             hipStream_t s) {
    long long np = 0;
    if (int rc = mesh_check_lattice(dm, n, origin, step, &np)) return rc;
    if (int rc = ensure_grid(np, false)) return rc;
    const int nx = n[0], ny = n[1], nz = dm == 3 ? n[2] : 1;
    const float ox = origin[0], oy = origin[1], oz = dm == 3 ? origin[2] : 0.f;
    const float sx = step[0], sy = step[1], sz = dm == 3 ? step[2] : 0.f;
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, d_values, dm, nx, ny, nz, level, d_mask, d_vbase,
                       d_tbase);
    GPIS_HIP(hipGetLastError());
    if (int rc = scan(d_vbase, np, d_part, s)) return rc;
    if (int rc = scan(d_tbase, np, d_part + kScanBlocks + 1, s)) return rc;
    GPIS_HIP(hipStreamSynchronize(s));
    const long long nv = h_tot[0], nt = h_tot[1];
    if (nv > kMaxCount || nt > kMaxCount) return GPIS_ERR_LIMIT;        // (before any output is allocated)
    if (int rc = grow(d_verts, cap_verts, (size_t)std::max(1ll, nv) * dm)) return rc;
    if (int rc = grow(d_prims, cap_prims, (size_t)std::max(1ll, nt) * dm)) return rc;
    if (nv > 0) {
        hipLaunchKernelGGL(mesh_vertex_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, d_values, dm, nx, ny, nz, ox, oy, oz, sx, sy, sz,
                           level, d_mask, d_vbase, d_verts);
        GPIS_HIP(hipGetLastError());
    }
    if (nt > 0) {
        hipLaunchKernelGGL(mesh_prim_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, d_values, dm, nx, ny, nz, level, d_mask, d_vbase,
                           d_tbase, d_prims);
        GPIS_HIP(hipGetLastError());
    }
    GPIS_HIP(hipStreamSynchronize(s));
    dim = dm; nvert = nv; nprim = nt; ngrid = np;
    return GPIS_OK;
}

int MeshExtractor::from_map(MapQuery& mq, OnGPISStore& store, int dm, const int* n, const float* origin, const float* step, float level,
                            hipStream_t s) {
    long long np = 0;
    if (int rc = mesh_check_lattice(dm, n, origin, step, &np)) return rc;
    if (int rc = ensure_grid(np, true)) return rc;
    const int nc = 2 * (1 + dm);
    if (int rc = lattice_values(mq, store, dm, n, origin, step, np, chunk, INFINITY, d_x, cap_x, d_rec, cap_rec, d_val, s)) return rc;
    if (int rc = from_grid(d_val, dm, n, origin, step, level, s)) return rc;
    grid_valid = true;
    if (int rc = grow(d_vrec, cap_vrec, (size_t)std::max(1ll, nvert) * nc)) return rc;
    if (nvert > 0) {
        GPIS_HIP(hipMemsetAsync(d_vrec, 0, sizeof(float) * (size_t)nvert * nc, s));
        if (int rc = mq.run(store, d_verts, (int)nvert, d_vrec, s)) return rc;
    }
    GPIS_HIP(hipStreamSynchronize(s));
    rec_valid = true;
    return GPIS_OK;
}

}  // namespace gpis
