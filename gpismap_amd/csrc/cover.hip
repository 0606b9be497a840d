// Coverage, frontiers and the field restricted to seen space (cover.h).
//
// Lattice point (i, j, k): index p = (k ny + j) nx + i, world point o + (float)i * s (no FMA: -ffp-contract=off).  Every double
// expression below is written in the order tests/cover_ref.py evaluates it; the build does not contract, so the bits agree.
//
// Integration: one thread per lattice point (grid stride) reads its own byte, leaves a seen point alone, else projects the point
// into the frame (3-D: the nearest pixel's depth; 2-D: a binary search of the sector table) and writes its own byte.
// Frontiers: count, scan, write over chunks of 2048 points (the lattice indices come out ascending) with the rank grid as a
// by-product; labels, roots and the table's buffers by components.h, the neighbours being the 8 / 26 of the lattice; the table by
// integer atomics.
#include <climits>
#include <cmath>
#include <cstring>
#include "cover.h"
#include "block_ops.h"
#include "dfield.h"

namespace gpis {

namespace {

constexpr int kBlock = Coverage::kBlock;
constexpr int kTabWords = kCompTabWords;

struct CovPose { float v[12]; };

// ---- integration ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) cover_depth_kernel(DfLattice L, int n, CovPose P, double fx, double fy, double cx, double cy, int W, int H,
                                                             const float* __restrict__ depth, double back_off,
                                                             unsigned char* __restrict__ seen) {
    const int nxy = L.nx * L.ny;
    const double t0 = (double)P.v[0], t1 = (double)P.v[1], t2 = (double)P.v[2];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        if (seen[p]) continue;
        const int i = p % L.nx, j = (p / L.nx) % L.ny, k = p / nxy;
        const float x0 = L.ox + (float)i * L.st, x1 = L.oy + (float)j * L.st, x2 = L.oz + (float)k * L.st;
        const double d0 = (double)x0 - t0, d1 = (double)x1 - t1, d2 = (double)x2 - t2;
        const double lx = (double)P.v[3] * d0 + (double)P.v[4] * d1 + (double)P.v[5] * d2;
        const double ly = (double)P.v[6] * d0 + (double)P.v[7] * d1 + (double)P.v[8] * d2;
        const double lz = (double)P.v[9] * d0 + (double)P.v[10] * d1 + (double)P.v[11] * d2;
        if (!(lz > 0.0)) continue;
        const double u = floor(fx * lx / lz + cx + 0.5), v = floor(fy * ly / lz + cy + 0.5);
        if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) continue;
        const double d = (double)depth[(int)u * H + (int)v];
        if (d > 0.4 && d < 4.0 && lz < d - back_off) seen[p] = 1;
    }
}

__global__ void __launch_bounds__(kBlock) cover_scan_kernel(DfLattice L, int n, CovPose P, double off0, double off1, const double* __restrict__ q,
                                                            const double* __restrict__ lim, int m, unsigned char* __restrict__ seen) {
    const double t0 = (double)P.v[0], t1 = (double)P.v[1];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        if (seen[p]) continue;
        const int i = p % L.nx, j = p / L.nx;
        const float x0 = L.ox + (float)i * L.st, x1 = L.oy + (float)j * L.st;
        const double d0 = (double)x0 - t0, d1 = (double)x1 - t1;
        const double lx = ((double)P.v[2] * d0 + (double)P.v[3] * d1) - off0;
        const double ly = ((double)P.v[4] * d0 + (double)P.v[5] * d1) - off1;
        const double ll = lx * lx + ly * ly;
        bool s = ll == 0.0;
        if (!s) {
            const double e = lim[sector_of(q, m, pseudo_angle(lx, ly))];
            s = ll < e * e;                       // (e = 0 where the sector is wide or ends at the sensor)
        }
        if (s) seen[p] = 1;
    }
}

__global__ void __launch_bounds__(kBlock) cover_binarise_kernel(unsigned char* __restrict__ seen, int n) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) seen[p] = seen[p] ? 1 : 0;
}

// ---- compaction (compact.h): the predicates ---------------------------------------------------------------------------------
// a frontier point: seen and traversable, with an unseen and traversable axis neighbour inside the lattice
struct FrontierPred {
    DfLattice L;
    const unsigned char* seen;
    const float* dist;
    float clearance;
    __device__ bool operator()(int p) const {
        if (!(seen[p] && dist[p] >= clearance)) return false;
        const int nxy = L.nx * L.ny;
        const int i = p % L.nx, j = (p / L.nx) % L.ny, k = p / nxy;
        bool f = false;
        if (i > 0) f = f || (!seen[p - 1] && dist[p - 1] >= clearance);
        if (i + 1 < L.nx) f = f || (!seen[p + 1] && dist[p + 1] >= clearance);
        if (j > 0) f = f || (!seen[p - L.nx] && dist[p - L.nx] >= clearance);
        if (j + 1 < L.ny) f = f || (!seen[p + L.nx] && dist[p + L.nx] >= clearance);
        if (k > 0) f = f || (!seen[p - nxy] && dist[p - nxy] >= clearance);
        if (k + 1 < L.nz) f = f || (!seen[p + nxy] && dist[p + nxy] >= clearance);
        return f;
    }
};

// ---- labels (components.h): the links ---------------------------------------------------------------------------------------
// the 8 / 26 neighbours of frontier point r, through the rank grid
struct LatticeLinks {
    DfLattice L;
    const int* __restrict__ list;
    const int* __restrict__ rank;
    __device__ int operator()(int r, int best, const int* label) const {
        const int nxy = L.nx * L.ny;
        const int p = list[r];
        const int i = p % L.nx, j = (p / L.nx) % L.ny, k = p / nxy;
        for (int dz = -1; dz <= 1; ++dz) {
            if (k + dz < 0 || k + dz >= L.nz) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                if (j + dy < 0 || j + dy >= L.ny) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    if (i + dx < 0 || i + dx >= L.nx) continue;
                    const int nr = rank[p + (dz * L.ny + dy) * L.nx + dx];
                    if (nr >= 0) best = min(best, ld_label(label + nr));
                }
            }
        }
        return best;
    }
};

// ---- the table ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) cover_tab_init_kernel(unsigned long long* __restrict__ tab, int* __restrict__ box, int nc) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
        unsigned long long* t = tab + (size_t)c * kTabWords;
        t[0] = t[1] = t[2] = t[3] = 0ull;
        t[4] = t[5] = ~0ull;
        t[6] = t[7] = 0ull;
        for (int a = 0; a < 3; ++a) { box[c * 6 + a] = INT_MAX; box[c * 6 + 3 + a] = -1; }
    }
}

// count, integer sums and box of each component; the points' labels as lattice indices.  The list ascends and components are
// compact, so the 64 points of a wavefront mostly share one component: such a wavefront reduces its integers through lane
// shuffles and sends one atomic per word instead of 64 to the same address (integers: the order changes nothing).
__global__ void __launch_bounds__(kBlock) cover_tab_sum_kernel(DfLattice L, const int* __restrict__ list, const int* __restrict__ label,
                                                               const int* __restrict__ cidx, int m, unsigned long long* tab, int* box,
                                                               int* __restrict__ plabel) {
    const int nxy = L.nx * L.ny;
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {
        const int r = r0 + threadIdx.x;
        const bool ok = r < m;
        int c = -1, ijk[3] = {0, 0, 0};
        if (ok) {
            const int p = list[r], root = label[r];
            c = cidx[root];
            ijk[0] = p % L.nx; ijk[1] = (p / L.nx) % L.ny; ijk[2] = p / nxy;
            plabel[r] = list[root];
        }
        const int c0 = __shfl(c, 0, kWave);                    // (lane 0 holds the wavefront's smallest r)
        if (c0 < 0) continue;                                  // the whole wavefront lies past the list
        if (__all(!ok || c == c0)) {
            const unsigned long long cnt = wave_reduce(ok ? 1ull : 0ull, OpAdd());
            unsigned long long sm[3];
            int lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sm[a] = wave_reduce(ok ? (unsigned long long)ijk[a] : 0ull, OpAdd());
                lo[a] = wave_reduce(ok ? ijk[a] : INT_MAX, OpMin());
                hi[a] = wave_reduce(ok ? ijk[a] : -1, OpMax());
            }
            if ((threadIdx.x & (kWave - 1)) == 0) {
                unsigned long long* t = tab + (size_t)c0 * kTabWords;
                atomicAdd(&t[0], cnt);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    atomicAdd(&t[1 + a], sm[a]);
                    atomicMin(&box[c0 * 6 + a], lo[a]);
                    atomicMax(&box[c0 * 6 + 3 + a], hi[a]);
                }
            }
        } else if (ok) {
            unsigned long long* t = tab + (size_t)c * kTabWords;
            atomicAdd(&t[0], 1ull);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicAdd(&t[1 + a], (unsigned long long)ijk[a]);
                atomicMin(&box[c * 6 + a], ijk[a]);
                atomicMax(&box[c * 6 + 3 + a], ijk[a]);
            }
        }
    }
}

// the squared distance of point r to its component's centroid, in double: (i - si / n)^2 + (j - sj / n)^2 (+ (k - sk / n)^2)
__device__ __forceinline__ double cover_d2(const DfLattice& L, int p, const unsigned long long* t) {
    const int nxy = L.nx * L.ny;
    const double cnt = (double)t[0];
    const double di = (double)(p % L.nx) - (double)t[1] / cnt, dj = (double)((p / L.nx) % L.ny) - (double)t[2] / cnt;
    double d2 = di * di + dj * dj;
    if (L.dim == 3) {
        const double dk = (double)(p / nxy) - (double)t[3] / cnt;
        d2 = d2 + dk * dk;
    }
    return d2;
}

// STAGE 0: t[4] = the smallest distance's bits (non-negative doubles order as their bits), one atomic per wavefront where its
// points share a component; STAGE 1: t[5] = the smallest rank among the points at that distance
template <int STAGE>
__global__ void __launch_bounds__(kBlock) cover_tab_rep_kernel(DfLattice L, const int* __restrict__ list, const int* __restrict__ label,
                                                               const int* __restrict__ cidx, int m, unsigned long long* tab) {
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {
        const int r = r0 + threadIdx.x;
        const bool ok = r < m;
        const int c = ok ? cidx[label[r]] : -1;
        unsigned long long b = ~0ull;
        if (ok) b = (unsigned long long)__double_as_longlong(cover_d2(L, list[r], tab + (size_t)c * kTabWords));
        if (STAGE == 1) {
            if (ok && b == tab[(size_t)c * kTabWords + 4]) atomicMin(&tab[(size_t)c * kTabWords + 5], (unsigned long long)r);
            continue;
        }
        const int c0 = __shfl(c, 0, kWave);
        if (c0 < 0) continue;
        if (__all(!ok || c == c0)) {
            const unsigned long long bm = wave_reduce(b, OpMin());
            if ((threadIdx.x & (kWave - 1)) == 0) atomicMin(&tab[(size_t)c0 * kTabWords + 4], bm);
        } else if (ok) {
            atomicMin(&tab[(size_t)c * kTabWords + 4], b);
        }
    }
}

// ranks to lattice indices: t[5] = the representative, t[6] = the label
__global__ void __launch_bounds__(kBlock) cover_tab_final_kernel(const int* __restrict__ list, const int* __restrict__ roots, int nc,
                                                                 unsigned long long* __restrict__ tab) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
        unsigned long long* t = tab + (size_t)c * kTabWords;
        t[5] = (unsigned long long)list[(int)t[5]];
        t[6] = (unsigned long long)list[roots[c]];
    }
}

// ---- the restricted field -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) cover_restrict_kernel(const unsigned char* __restrict__ seen, const float* __restrict__ dist,
                                                                const int* __restrict__ site, int n, float unseen, float* __restrict__ dist_out,
                                                                int* __restrict__ site_out) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        dist_out[p] = seen[p] ? dist[p] : unseen;
        site_out[p] = site[p];
    }
}

}  // namespace

Coverage::Coverage() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

Coverage::~Coverage() { (void)bind(-1); }

int Coverage::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_seen, (void*)d_rank, (void*)d_plabel, (void*)d_sector, (void*)d_depth}) (void)hipFree(p);
        comp.release();
        if (own) (void)hipStreamDestroy(own);
    }
    d_seen = nullptr; d_rank = d_plabel = nullptr; d_sector = nullptr; d_depth = nullptr; own = nullptr;
    cap_n = cap_rank = cap_plabel = cap_beams = cap_pix = 0;
    clear_frontiers();
    has_lattice = false; dim = 0; ngrid = 0; frames = 0;
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

bool Coverage::same_lattice(const DistanceField& df) const {
    if (!has_lattice || !df.valid || df.dim != dim || df.step != step || df.device != device) return false;
    for (int a = 0; a < dim; ++a)
        if (df.n[a] != n[a] || df.origin[a] != origin[a]) return false;
    return true;
}

int Coverage::reset(const DistanceField& df) {
    if (!df.valid) return GPIS_ERR_STATE;
    if (int rc = bind(df.device)) return rc;
    clear_frontiers();
    has_lattice = false;
    if (int rc = grow(d_seen, cap_n, (size_t)df.ngrid)) return rc;
    GPIS_HIP(hipMemsetAsync(d_seen, 0, (size_t)df.ngrid, own));
    GPIS_HIP(hipStreamSynchronize(own));
    dim = df.dim; ngrid = df.ngrid; step = df.step;
    for (int a = 0; a < 3; ++a) { n[a] = a < dim ? df.n[a] : 1; origin[a] = a < dim ? df.origin[a] : 0.f; }
    frames = 0;
    has_lattice = true;
    return GPIS_OK;
}

int Coverage::set(const unsigned char* seen) {
    if (!has_lattice) return GPIS_ERR_STATE;
    clear_frontiers();
    GPIS_HIP(hipMemcpyAsync(d_seen, seen, (size_t)ngrid, hipMemcpyHostToDevice, own));
    hipLaunchKernelGGL(cover_binarise_kernel, dim3(grid_for(ngrid)), dim3(kBlock), 0, own, d_seen, (int)ngrid);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(own));
    return GPIS_OK;
}

int Coverage::get(unsigned char* seen) {
    if (!has_lattice) return GPIS_ERR_STATE;
    GPIS_HIP(hipMemcpyAsync(seen, d_seen, (size_t)ngrid, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    return GPIS_OK;
}

int Coverage::integrate(const SensorFrame& f, const float* in, const float* pose, const CoverOpts& o, hipStream_t s) {
    if (!has_lattice) return GPIS_ERR_STATE;
    if (f.geo.dim != dim) return GPIS_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    clear_frontiers();
    const DfLattice L = lattice();
    CovPose P;
    for (int k = 0; k < 12; ++k) P.v[k] = k < (dim == 3 ? 12 : 6) ? pose[k] : 0.f;
    if (dim == 3) {
        if (int rc = grow(d_depth, cap_pix, (size_t)f.n)) return rc;
        GPIS_HIP(hipMemcpyAsync(d_depth, in, sizeof(float) * (size_t)f.n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(cover_depth_kernel, dim3(grid_for(ngrid)), dim3(kBlock), 0, s, L, (int)ngrid, P, (double)f.geo.fx, (double)f.geo.fy,
                           (double)f.geo.cx, (double)f.geo.cy, f.geo.width, f.geo.height, d_depth, (double)o.back_off, d_seen);
        GPIS_HIP(hipGetLastError());
        GPIS_HIP(hipStreamSynchronize(s));
    } else {
        SectorTable t;
        sector_table(f.cs.data(), in, f.n, o.back_off, o.max_gap, &t);
        const long long m = t.size();
        if (m >= 2) {                                           // (fewer than two valid beams: nothing is seen)
            if (int rc = grow(d_sector, cap_beams, (size_t)(2 * m))) return rc;
            GPIS_HIP(hipMemcpyAsync(d_sector, t.q.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
            GPIS_HIP(hipMemcpyAsync(d_sector + m, t.lim_eff.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(cover_scan_kernel, dim3(grid_for(ngrid)), dim3(kBlock), 0, s, L, (int)ngrid, P, (double)f.geo.off[0],
                               (double)f.geo.off[1], d_sector, d_sector + m, (int)m, d_seen);
            GPIS_HIP(hipGetLastError());
            GPIS_HIP(hipStreamSynchronize(s));                  // (the table lives until here)
        }
    }
    ++frames;
    integrate_ms = ms_since(t0);
    return GPIS_OK;
}

int Coverage::frontiers(const DistanceField& df, const CoverOpts& o, hipStream_t s) {
    if (!has_lattice || !df.valid) return GPIS_ERR_STATE;
    if (!same_lattice(df)) return GPIS_ERR_ARG;
    if (int rc = cover_check_opts(o)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    clear_frontiers();
    const DfLattice L = lattice();
    const int np = (int)ngrid;
    if (int rc = grow(d_rank, cap_rank, (size_t)np)) return rc;
    if (int rc = comp.reserve(np)) return rc;
    auto grow_lists = [&](int m) -> int {
        if (int rc = comp.grow_lists(m)) return rc;
        return grow(d_plabel, cap_plabel, (size_t)std::max(1, m));
    };
    int m = 0;
    const FrontierPred pred{L, d_seen, df.d_dist, o.clearance};
    if (int rc = compact_run(pred, np, comp.d_bcount, comp.h_word, &m, comp.d_list, d_rank, s, grow_lists)) return rc;

    long long done = 0;
    int nc = 0;
    if (m > 0) {
        done = comp.label(LatticeLinks{L, comp.d_list, d_rank}, m, o.max_rounds, s);
        if (done < 0) return (int)done;
        if (int rc = comp.roots(m, &nc, s)) return rc;
        if (int rc = comp.grow_table(nc)) return rc;
        int *const d_list = comp.d_list, *const d_label = comp.d_label, *const d_cidx = comp.d_cidx, *const d_box = comp.d_box;
        unsigned long long* const d_tab = comp.d_tab;
        hipLaunchKernelGGL(cover_tab_init_kernel, dim3(grid_for(nc)), dim3(kBlock), 0, s, d_tab, d_box, nc);
        GPIS_HIP(hipGetLastError());
        hipLaunchKernelGGL(cover_tab_sum_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, L, d_list, d_label, d_cidx, m, d_tab, d_box, d_plabel);
        GPIS_HIP(hipGetLastError());
        hipLaunchKernelGGL(cover_tab_rep_kernel<0>, dim3(grid_for(m)), dim3(kBlock), 0, s, L, d_list, d_label, d_cidx, m, d_tab);
        GPIS_HIP(hipGetLastError());
        hipLaunchKernelGGL(cover_tab_rep_kernel<1>, dim3(grid_for(m)), dim3(kBlock), 0, s, L, d_list, d_label, d_cidx, m, d_tab);
        GPIS_HIP(hipGetLastError());
        hipLaunchKernelGGL(cover_tab_final_kernel, dim3(grid_for(nc)), dim3(kBlock), 0, s, d_list, comp.d_roots, nc, d_tab);
        GPIS_HIP(hipGetLastError());
        const int* h_box;
        if (int rc = comp.fetch_table(nc, &h_box, s)) return rc;
        for (int c = 0; c < nc; ++c) {
            const unsigned long long* t = comp.h_tab + (size_t)c * kTabWords;
            if ((long long)t[0] < (long long)o.min_size) continue;
            label.push_back((int)t[6]); count.push_back((int)t[0]); rep.push_back((int)t[5]);
            for (int a = 0; a < 3; ++a) sums.push_back((long long)t[1 + a]);
            for (int a = 0; a < 6; ++a) box.push_back(h_box[c * 6 + a]);
        }
    } else {
        GPIS_HIP(hipStreamSynchronize(s));
    }
    npoints = m; ncomponents = nc; rounds = done;
    frontiers_ms = ms_since(t0);
    frontiers_valid = true;
    return GPIS_OK;
}

int Coverage::restrict_field(const DistanceField& in, DistanceField& out, float unseen_dist, hipStream_t s) {
    if (!has_lattice || !in.valid) return GPIS_ERR_STATE;
    if (&in == &out || !std::isfinite(unseen_dist) || !same_lattice(in)) return GPIS_ERR_ARG;
    if (int rc = out.bind(in.device)) return rc;
    out.clear_result();
    if (int rc = out.ensure(ngrid)) return rc;
    hipLaunchKernelGGL(cover_restrict_kernel, dim3(grid_for(ngrid)), dim3(kBlock), 0, s, d_seen, in.d_dist, in.d_site(), (int)ngrid, unseen_dist,
                       out.d_dist, out.d_feat[0]);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    out.dim = dim; out.ngrid = ngrid; out.site_buf = 0; out.step = step;
    for (int a = 0; a < 3; ++a) { out.n[a] = n[a]; out.origin[a] = origin[a]; }
    out.valid = true;
    return GPIS_OK;
}

}  // namespace gpis
