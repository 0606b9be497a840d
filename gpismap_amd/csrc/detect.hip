// Moving obstacles from a frame's residual against a distance field (detect.h).
//
// Sample grid: the beams of a scan (q = the beam), or the strided pixels of a depth frame, q = n * gh + m over gw x gh =
// W / stride x H / stride (column-major: the tracker's order).  Per valid sample (Tracker::setup's list): x = world_point<D> of
// its local point at the float pose, d = df_sample_at(dist, x)[0]; foreign iff d is finite and (double)d >= min_dist and, with a
// coverage mask, the byte of the lattice point nearest x -- per axis min((int)floorf((x - o) / step + 0.5f), n - 1), in float --
// is set.  Neighbours: beams q - 1, q + 1 (no wrap from the last beam to the first); in 3-D the 8 neighbours on the strided grid.
// Two neighbouring foreign samples are linked iff e_0 e_0 + e_1 e_1 (+ e_2 e_2) <= link * link with e_a = (double)x_a -
// (double)y_a, summed left to right.  Labels, roots and the table's buffers: components.h.  The table: a count (integer sum), per
// axis the least and greatest coordinate (integer min / max of an order-preserving key of the float), the centre 0.5 *
// ((double)lo + (double)hi), r2 = the greatest sum_a ((double)x_a - c_a)^2 (integer max on the bits of the non-negative double).
// No floating-point atomics.  Every double expression is written in the order tests/detect_ref.py evaluates it; the build does
// not contract, so the bits agree.
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include "detect.h"
#include "block_ops.h"
#include "cover.h"
#include "dfield.h"
#include "obst.h"
#include "world_point.h"

namespace gpis {

static_assert(kDetectMaxBalls == Obstacles::kMax, "detect_host.h's cap is the set's");

namespace {

constexpr int kBlock = Detector::kBlock;
constexpr int kTabWords = kCompTabWords;

struct DetPose { float R[9], t[3]; };
struct DetGrid { int g, gh, gw; };             // samples, rows and columns of the grid (2-D: gh = gw = 0)

// the order-preserving key of a float: a < b as floats (with -0 < +0) iff key(a) < key(b) as unsigned
__host__ __device__ inline unsigned det_key(unsigned b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__host__ __device__ inline unsigned det_unkey(unsigned k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

// ---- foreign samples ----------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kBlock) detect_flag_kernel(DetPose P, const float4* __restrict__ loc, const int* __restrict__ vlist, int m,
                                                             const float* __restrict__ F, DfLattice L, double min_dist,
                                                             const unsigned char* __restrict__ seen, float* __restrict__ x,
                                                             float* __restrict__ d, unsigned char* __restrict__ flag) {
    L.dim = D;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int q = vlist[j];
        float w[3] = {0.f, 0.f, 0.f}, o[1 + D];
        world_point<D>(P.R, P.t, loc[j], w);
        df_sample_at(F, L, w[0], w[1], w[2], o);
        const float dd = o[0];
        bool f = isfinite(dd) && (double)dd >= min_dist;
        if (f && seen) {
            const int i0 = min((int)floorf((w[0] - L.ox) / L.st + 0.5f), L.nx - 1);
            const int i1 = min((int)floorf((w[1] - L.oy) / L.st + 0.5f), L.ny - 1);
            const int i2 = D == 3 ? min((int)floorf((w[2] - L.oz) / L.st + 0.5f), L.nz - 1) : 0;
            f = seen[((size_t)i2 * L.ny + i1) * L.nx + i0] != 0;
        }
#pragma unroll
        for (int a = 0; a < D; ++a) x[(size_t)q * D + a] = w[a];
        d[q] = dd;
        flag[q] = f ? 1 : 0;
    }
}

struct ForeignPred {
    const unsigned char* flag;
    __device__ bool operator()(int q) const { return flag[q] != 0; }
};

// ---- labels (components.h): the links -------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ bool det_linked(const float* __restrict__ x, int q, int p, double link2) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double e = (double)x[(size_t)q * D + a] - (double)x[(size_t)p * D + a];
        s = s + e * e;
    }
    return s <= link2;
}

// the grid neighbours of foreign sample r (2-D: beams q - 1, q + 1; 3-D: the 8 of the strided grid) whose world points lie within link
template <int D>
struct GridLinks {
    DetGrid G;
    const int* __restrict__ list;
    const int* __restrict__ rank;
    const float* __restrict__ x;
    double link2;
    __device__ int operator()(int r, int best, const int* label) const {
        const int q = list[r];
        if (D == 2) {
            for (int dq = -1; dq <= 1; dq += 2) {
                const int p = q + dq;
                if (p < 0 || p >= G.g) continue;
                const int nr = rank[p];
                if (nr >= 0 && det_linked<D>(x, q, p, link2)) best = min(best, ld_label(label + nr));
            }
        } else {
            const int gn = q / G.gh, gm = q - gn * G.gh;
            for (int dn = -1; dn <= 1; ++dn) {
                if (gn + dn < 0 || gn + dn >= G.gw) continue;
                for (int dm = -1; dm <= 1; ++dm) {
                    if ((dn == 0 && dm == 0) || gm + dm < 0 || gm + dm >= G.gh) continue;
                    const int p = (gn + dn) * G.gh + gm + dm;
                    const int nr = rank[p];
                    if (nr >= 0 && det_linked<D>(x, q, p, link2)) best = min(best, ld_label(label + nr));
                }
            }
        }
        return best;
    }
};

// ---- the table ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) detect_tab_init_kernel(unsigned long long* __restrict__ tab, unsigned* __restrict__ box, int nc) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
        unsigned long long* t = tab + (size_t)c * kTabWords;
#pragma unroll
        for (int k = 0; k < kTabWords; ++k) t[k] = 0ull;
        for (int a = 0; a < 3; ++a) { box[c * 6 + a] = 0xffffffffu; box[c * 6 + 3 + a] = 0u; }
    }
}

// count and box of each component, and the label image.  The list ascends and a component is compact on the grid, so the 64
// samples of a wavefront mostly share one component: such a wavefront reduces through lane shuffles and sends one atomic per word.
template <int D>
__global__ void __launch_bounds__(kBlock) detect_tab_box_kernel(const int* __restrict__ list, const int* __restrict__ label,
                                                                const int* __restrict__ cidx, const float* __restrict__ x, int m,
                                                                unsigned long long* tab, unsigned* box, int* __restrict__ limg) {
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {
        const int r = r0 + threadIdx.x;
        const bool ok = r < m;
        int c = -1;
        unsigned k[D];
#pragma unroll
        for (int a = 0; a < D; ++a) k[a] = 0u;
        if (ok) {
            const int q = list[r], root = label[r];
            c = cidx[root];
            limg[q] = list[root];
#pragma unroll
            for (int a = 0; a < D; ++a) k[a] = det_key(__float_as_uint(x[(size_t)q * D + a]));
        }
        const int c0 = __shfl(c, 0, kWave);
        if (c0 < 0) continue;                                  // the whole wavefront lies past the list
        if (__all(!ok || c == c0)) {
            const unsigned long long cnt = wave_reduce(ok ? 1ull : 0ull, OpAdd());
            unsigned lo[D], hi[D];
#pragma unroll
            for (int a = 0; a < D; ++a) {
                lo[a] = wave_reduce(ok ? k[a] : 0xffffffffu, OpMin());
                hi[a] = wave_reduce(ok ? k[a] : 0u, OpMax());
            }
            if ((threadIdx.x & (kWave - 1)) == 0) {
                atomicAdd(&tab[(size_t)c0 * kTabWords], cnt);
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    atomicMin(&box[c0 * 6 + a], lo[a]);
                    atomicMax(&box[c0 * 6 + 3 + a], hi[a]);
                }
            }
        } else if (ok) {
            atomicAdd(&tab[(size_t)c * kTabWords], 1ull);
#pragma unroll
            for (int a = 0; a < D; ++a) {
                atomicMin(&box[c * 6 + a], k[a]);
                atomicMax(&box[c * 6 + 3 + a], k[a]);
            }
        }
    }
}

// one thread per component: the centre's bits into t[1 + a], the label (a grid index) into t[5]
template <int D>
__global__ void __launch_bounds__(kBlock) detect_tab_centre_kernel(const int* __restrict__ list, const int* __restrict__ roots,
                                                                   const unsigned* __restrict__ box, int nc, unsigned long long* __restrict__ tab) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
        unsigned long long* t = tab + (size_t)c * kTabWords;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const float lo = __uint_as_float(det_unkey(box[c * 6 + a])), hi = __uint_as_float(det_unkey(box[c * 6 + 3 + a]));
            t[1 + a] = (unsigned long long)__double_as_longlong(0.5 * ((double)lo + (double)hi));
        }
        t[5] = (unsigned long long)list[roots[c]];
    }
}

// t[4] = the bits of the greatest squared distance to the centre (non-negative doubles order as their bits)
template <int D>
__global__ void __launch_bounds__(kBlock) detect_tab_r2_kernel(const int* __restrict__ list, const int* __restrict__ label,
                                                               const int* __restrict__ cidx, const float* __restrict__ x, int m,
                                                               unsigned long long* tab) {
    for (int r0 = blockIdx.x * blockDim.x; r0 < m; r0 += gridDim.x * blockDim.x) {
        const int r = r0 + threadIdx.x;
        const bool ok = r < m;
        const int c = ok ? cidx[label[r]] : -1;
        unsigned long long b = 0ull;
        if (ok) {
            const int q = list[r];
            const unsigned long long* t = tab + (size_t)c * kTabWords;
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const double e = (double)x[(size_t)q * D + a] - __longlong_as_double((long long)t[1 + a]);
                s = s + e * e;
            }
            b = (unsigned long long)__double_as_longlong(s);
        }
        const int c0 = __shfl(c, 0, kWave);
        if (c0 < 0) continue;
        if (__all(!ok || c == c0)) {
            const unsigned long long bm = wave_reduce(b, OpMax());
            if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(&tab[(size_t)c0 * kTabWords + 4], bm);
        } else if (ok) {
            atomicMax(&tab[(size_t)c * kTabWords + 4], b);
        }
    }
}

}  // namespace

Detector::Detector() { (void)hipGetDevice(&device); }

Detector::~Detector() { (void)bind(-1); }

int Detector::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (trk.own) (void)hipStreamSynchronize(trk.own);
        for (void* p : {(void*)d_x, (void*)d_d, (void*)d_flag, (void*)d_rank, (void*)d_limg}) (void)hipFree(p);
        comp.release();
    }
    d_x = d_d = nullptr; d_flag = nullptr; d_rank = d_limg = nullptr;
    cap_g = 0;
    clear_result();
    tracks.reset();
    device = dev;
    return trk.bind(dev);
}

int Detector::check(const DistanceField& df, const Coverage* cover, const TrackGeom& geo, long long n, const double* pose,
                    const DetectOpts& o, double t) const {
    if (int rc = detect_check_opts(o)) return rc;
    if (geo.dim != 2 && geo.dim != 3) return GPIS_ERR_ARG;
    for (int k = 0; k < (geo.dim == 3 ? 12 : 6); ++k) if (!std::isfinite(pose[k])) return GPIS_ERR_ARG;
    if (!std::isfinite(t)) return GPIS_ERR_ARG;
    if (!df.valid) return GPIS_ERR_STATE;
    if (df.dim != geo.dim) return GPIS_ERR_ARG;
    if (n > kMaxFramePoints) return GPIS_ERR_LIMIT;
    if (cover && !cover->same_lattice(df)) return GPIS_ERR_STATE;
    if (tracks.held && !(t > tracks.t_prev)) return GPIS_ERR_ARG;
    return GPIS_OK;
}

int Detector::detect(const DistanceField& df, const Coverage* cover, const TrackGeom& geo, const float* in, const double* cs, long long n,
                     const double* pose, const DetectOpts& o, double t, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    auto mark = t0;
    auto lap = [&](double* acc) {
        if (profile) (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        *acc = std::chrono::duration<double, std::milli>(now - mark).count();
        mark = now;
    };
    clear_result();
    const int dm = geo.dim;
    // the tracker's set-up reads the stride alone; the rest are values its check accepts
    TrackOpts to{};
    to.huber = 1.0; to.max_var = INFINITY; to.stride = dm == 3 ? o.stride : 1;
    if (int rc = trk.setup(geo, in, cs, n, to, s)) return rc;
    const long long m = trk.points;
    const int ghh = dm == 3 ? geo.height / to.stride : 0, gww = dm == 3 ? geo.width / to.stride : 0;
    const long long G = dm == 3 ? (long long)gww * ghh : n;
    lap(&setup_ms);

    const size_t ng = (size_t)std::max(1ll, G);
    if (ng > cap_g) {
        for (void* p : {(void*)d_x, (void*)d_d, (void*)d_flag, (void*)d_rank, (void*)d_limg}) (void)hipFree(p);
        d_x = d_d = nullptr; d_flag = nullptr; d_rank = d_limg = nullptr; cap_g = 0;
        GPIS_HIP(hipMalloc((void**)&d_x, sizeof(float) * 3 * ng));
        GPIS_HIP(hipMalloc((void**)&d_d, sizeof(float) * ng));
        GPIS_HIP(hipMalloc((void**)&d_flag, ng));
        GPIS_HIP(hipMalloc((void**)&d_rank, sizeof(int) * ng));
        GPIS_HIP(hipMalloc((void**)&d_limg, sizeof(int) * ng));
        cap_g = ng;
    }
    if (int rc = comp.reserve(G)) return rc;

    GPIS_HIP(hipMemsetAsync(d_x, 0, sizeof(float) * (size_t)dm * ng, s));
    GPIS_HIP(hipMemsetD32Async((hipDeviceptr_t)d_d, 0x7fc00000, ng, s));
    GPIS_HIP(hipMemsetAsync(d_flag, 0, ng, s));
    GPIS_HIP(hipMemsetAsync(d_limg, 0xff, sizeof(int) * ng, s));
    DetPose P{};
    for (int k = 0; k < dm; ++k) P.t[k] = (float)pose[k];
    for (int k = 0; k < dm * dm; ++k) P.R[k] = (float)pose[dm + k];
    const unsigned char* seen = cover ? cover->d_seen : nullptr;
    if (m > 0) {
        if (dm == 3)
            hipLaunchKernelGGL(detect_flag_kernel<3>, dim3(grid_for(m)), dim3(kBlock), 0, s, P, (const float4*)trk.d_loc, trk.d_list, (int)m,
                               (const float*)df.d_dist, df.lattice(), o.min_dist, seen, d_x, d_d, d_flag);
        else
            hipLaunchKernelGGL(detect_flag_kernel<2>, dim3(grid_for(m)), dim3(kBlock), 0, s, P, (const float4*)trk.d_loc, trk.d_list, (int)m,
                               (const float*)df.d_dist, df.lattice(), o.min_dist, seen, d_x, d_d, d_flag);
        GPIS_HIP(hipGetLastError());
    }
    lap(&flag_ms);

    auto grow_lists = [&](int mm) -> int { return comp.grow_lists(mm); };
    int mf = 0;
    if (int rc = compact_run(ForeignPred{d_flag}, (int)G, comp.d_bcount, comp.h_word, &mf, comp.d_list, d_rank, s, grow_lists)) return rc;
    lap(&compact_ms);

    const DetGrid GG{(int)G, ghh, gww};
    const double link2 = o.link * o.link;
    long long done = 0;
    int nc = 0;
    if (mf > 0) {
        int *const d_list = comp.d_list, *const d_label = comp.d_label, *const d_cidx = comp.d_cidx, *const d_roots = comp.d_roots;
        done = dm == 3 ? comp.label(GridLinks<3>{GG, d_list, d_rank, d_x, link2}, mf, o.max_rounds, s)
                       : comp.label(GridLinks<2>{GG, d_list, d_rank, d_x, link2}, mf, o.max_rounds, s);
        if (done < 0) return (int)done;
        lap(&label_ms);

        if (int rc = comp.roots(mf, &nc, s)) return rc;
        if (int rc = comp.grow_table(nc)) return rc;
        unsigned long long* const d_tab = comp.d_tab;
        unsigned* const d_box = comp.d_box;
        hipLaunchKernelGGL(detect_tab_init_kernel, dim3(grid_for(nc)), dim3(kBlock), 0, s, d_tab, d_box, nc);
        GPIS_HIP(hipGetLastError());
        if (dm == 3) {
            hipLaunchKernelGGL(detect_tab_box_kernel<3>, dim3(grid_for(mf)), dim3(kBlock), 0, s, d_list, d_label, d_cidx, d_x, mf, d_tab, d_box, d_limg);
            hipLaunchKernelGGL(detect_tab_centre_kernel<3>, dim3(grid_for(nc)), dim3(kBlock), 0, s, d_list, d_roots, d_box, nc, d_tab);
            hipLaunchKernelGGL(detect_tab_r2_kernel<3>, dim3(grid_for(mf)), dim3(kBlock), 0, s, d_list, d_label, d_cidx, d_x, mf, d_tab);
        } else {
            hipLaunchKernelGGL(detect_tab_box_kernel<2>, dim3(grid_for(mf)), dim3(kBlock), 0, s, d_list, d_label, d_cidx, d_x, mf, d_tab, d_box, d_limg);
            hipLaunchKernelGGL(detect_tab_centre_kernel<2>, dim3(grid_for(nc)), dim3(kBlock), 0, s, d_list, d_roots, d_box, nc, d_tab);
            hipLaunchKernelGGL(detect_tab_r2_kernel<2>, dim3(grid_for(mf)), dim3(kBlock), 0, s, d_list, d_label, d_cidx, d_x, mf, d_tab);
        }
        GPIS_HIP(hipGetLastError());
        const unsigned* h_box;
        if (int rc = comp.fetch_table(nc, &h_box, s)) return rc;
        c_label.resize(nc); c_count.resize(nc); c_box.assign((size_t)nc * 6, 0.f); c_centre.assign((size_t)nc * 3, 0.0); c_r2.resize(nc);
        for (int c = 0; c < nc; ++c) {
            const unsigned long long* tt = comp.h_tab + (size_t)c * kTabWords;
            c_count[c] = (int)tt[0]; c_label[c] = (int)tt[5];
            std::memcpy(&c_r2[c], &tt[4], sizeof(double));
            for (int a = 0; a < dm; ++a) {
                std::memcpy(&c_centre[(size_t)c * 3 + a], &tt[1 + a], sizeof(double));
                const unsigned lo = det_unkey(h_box[c * 6 + a]), hi = det_unkey(h_box[c * 6 + 3 + a]);
                std::memcpy(&c_box[(size_t)c * 6 + a], &lo, sizeof(float));
                std::memcpy(&c_box[(size_t)c * 6 + 3 + a], &hi, sizeof(float));
            }
        }
        lap(&table_ms);
    } else {
        GPIS_HIP(hipStreamSynchronize(s));
        label_ms = table_ms = 0.0;
    }

    // the host half (detect_host.h): selection, then the tracks
    std::vector<int> sel;
    detect_select(nc, c_count.data(), c_r2.data(), o, &c_flag, &sel);
    std::vector<DetBall> det(sel.size());
    for (size_t k = 0; k < sel.size(); ++k) {
        const int c = sel[k];
        for (int a = 0; a < dm; ++a) det[k].c[a] = c_centre[(size_t)c * 3 + a];
        det[k].r = std::sqrt(c_r2[c]) + o.pad;
        det[k].comp = c;
    }
    for (int c = 0; c < nc; ++c) {
        noise += c_flag[c] == kDetNoise; large += c_flag[c] == kDetLarge; dropped += c_flag[c] == kDetDropped;
    }
    balls = detect_associate(dm, std::move(det), t, o, &tracks);
    dim = dm; grid = G; gw = gww; gh = ghh; samples = m; foreign = mf; ncomp = nc; rounds = done; t_last = t;
    ms = ms_since(t0);
    valid = true;
    return GPIS_OK;
}

int Detector::to_obstacles(Obstacles& ob) const {
    if (!valid) return GPIS_ERR_STATE;
    const int nbl = (int)balls.size();
    std::vector<double> c((size_t)std::max(1, nbl) * dim), v((size_t)std::max(1, nbl) * dim), r((size_t)std::max(1, nbl));
    for (int i = 0; i < nbl; ++i) {
        for (int a = 0; a < dim; ++a) { c[(size_t)i * dim + a] = balls[i].c[a]; v[(size_t)i * dim + a] = balls[i].v[a]; }
        r[i] = balls[i].r;
    }
    return ob.set(dim, nbl, c.data(), v.data(), r.data(), t_last);
}

}  // namespace gpis
