// Candidate viewpoints scored by the unseen space they would reveal (view.h).
//
// Prediction: one thread per ray over m x rays marches its ray through the field (field_march.h: the field renderer's march) and
// writes d' = hit ? depth : miss, 4 B per ray.  A wavefront belongs to one pose -- in 3-D it owns an 8 x 8 pixel tile of that
// pose's image -- so the pose is read through scalar loads and the hit count is one ballot and one integer atomic per wavefront.
// Sector tables (2-D): the host orders the beams by pseudo-angle once (view_host.h); one workgroup per pose compacts that pose's
// valid beams in this order (block_ops.h's scan) and writes q[] and the folded lim[] of cover_host.h's sector_table.
// Targets: compact.h's count / offsets / write with the predicate !seen && !(dist < min_dist).
// Gather: a workgroup owns kBlock * kPoints targets, decodes each once, and walks its pose tiles of kPoseTile through LDS; per pose it
// applies cover.hip's rule in its operation order (double, left to right; the build does not contract), counts by ballot and
// popcount into a per-wavefront LDS word and ends the tile with one integer atomic per pose.  Integer sums: the schedule does
// not reach the bits.  An exact early reject skips the divisions: l.z >= the pose's largest valid d' less back_off (3-D), l.l >=
// the pose's largest lim^2 (2-D); rounding is monotone, so no point the rule accepts is rejected.
#include <cmath>
#include <cstring>
#include "view.h"
#include "block_ops.h"
#include "compact.h"
#include "cover.h"
#include "dfield.h"
#include "field_march.h"

namespace gpis {

namespace {

constexpr int kBlock = ViewScorer::kBlock;
constexpr int kPoints = ViewScorer::kPoints;
constexpr int kPoseTile = ViewScorer::kPoseTile;
constexpr int kWaves = kBlock / kWave;
static_assert(kPoseTile <= kBlock, "one thread per pose of a tile stages its cut and sends its count");

// ---- prediction -------------------------------------------------------------------------------------------------------------
// wavefront w of the grid: pose w / wpp, and of that pose's rays tile w % wpp (3-D: the 8 x 8 pixel tile (t / tiles_r, t %
// tiles_r), lanes over it as the field renderer's; 2-D: 64 consecutive beams).  all[0] += the samples taken.
template <int D>
__global__ void __launch_bounds__(kBlock) view_predict_kernel(TrackGeom tg, const float* __restrict__ pose, int m, const double* __restrict__ cs,
                                                              int n, int wpp, RenderFieldOpts o, float lx, float ly, float lz, float hx,
                                                              float hy, float hz, const float* __restrict__ F, DfLattice Lrt, float miss,
                                                              float* __restrict__ pred, int* __restrict__ hits,
                                                              unsigned* __restrict__ dmax, unsigned long long* __restrict__ all) {
    constexpr int PN = D == 3 ? 12 : 6;
    const long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (kWave - 1);
    const int k = __builtin_amdgcn_readfirstlane((int)(w / wpp));
    if (k >= m) return;                          // (the whole wavefront; no barrier follows)
    const int t = __builtin_amdgcn_readfirstlane((int)(w - (long long)k * wpp));
    int i;
    if (D == 3) {
        const int tiles_r = (tg.height + 7) >> 3;
        const int col = (t / tiles_r) * 8 + (lane >> 3), row = (t % tiles_r) * 8 + (lane & 7);
        i = (col < tg.width && row < tg.height) ? col * tg.height + row : -1;
    } else {
        i = t * kWave + lane;
        if (i >= n) i = -1;
    }
    RayGeom g{D, tg.width, tg.height, tg.fx, tg.fy, tg.cx, tg.cy, {}, {}, {tg.off[0], tg.off[1]}};
    const float* P = pose + (size_t)k * PN;
#pragma unroll
    for (int a = 0; a < D; ++a) g.t[a] = P[a];
#pragma unroll
    for (int a = 0; a < D * D; ++a) g.R[a] = P[D + a];
    DfLattice L = Lrt;
    L.dim = D;
    int ns = 0;
    bool hit = false;
    float dp = miss;
    if (i >= 0) {
        const float lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
        float u, v, il, z, zend, q, smp[1 + D];
        double cd, sd;
        ray_setup(g, cs, i, o.tnear, o.tfar, lo, hi, u, v, il, cd, sd, z, zend);
        hit = field_march<D>(g, u, v, il, cd, sd, z, zend, o, F, L, q, smp, ns) == 0;
        dp = hit ? q : miss;
        pred[(size_t)k * n + i] = dp;
    }
    const unsigned long long hb = __ballot(hit);
    unsigned bits = 0u;                          // 3-D: the largest d' the coverage's window accepts (positive floats order as their bits)
    if (D == 3) {
        const double dd = (double)dp;
        bits = wave_reduce((i >= 0 && dd > 0.4 && dd < 4.0) ? __float_as_uint(dp) : 0u, OpMax());
    }
    const unsigned long long sn = wave_reduce((unsigned long long)ns, OpAdd());
    if (lane == 0) {
        if (hb) atomicAdd(&hits[k], __popcll(hb));
        if (bits) atomicMax(&dmax[k], bits);
        if (sn) atomicAdd(all, sn);
    }
}

// ---- the sector table of every pose (2-D) -------------------------------------------------------------------------------------
// Workgroup k: the valid beams of pose k (0.2 < (double)r' < 30) in the host's order into sel, then per sector e -> e + 1 (the last
// wraps) q and lim_eff, cover_host.h's sector_table expression for expression.  csq: (c, s) of beam b at [2 b], its q at [2 n + b].
__global__ void __launch_bounds__(kBlock) view_sector_kernel(const float* __restrict__ pred, const double* __restrict__ csq,
                                                             const int* __restrict__ ord, int n, double bo, double cg, int* sel,
                                                             double* __restrict__ q, double* __restrict__ lim, int* __restrict__ nvalid,
                                                             double* __restrict__ lim2) {
    __shared__ int sh[kWaves];
    __shared__ double shd[kWaves];
    const size_t row = (size_t)blockIdx.x * n;
    const float* r = pred + row;
    int* sl = sel + row;
    const double* qb = csq + 2 * (size_t)n;
    int carry = 0;
    for (int base = 0; base < n; base += kBlock) {
        const int j = base + threadIdx.x;
        int b = 0, f = 0;
        if (j < n) {
            b = ord[j];
            const double rr = (double)r[b];
            f = (rr > 0.2 && rr < 30.0) ? 1 : 0;
        }
        int total;
        const int incl = block_incl_scan<kBlock, int>(f, sh, &total);
        if (f) sl[carry + incl - 1] = b;
        carry += total;
    }
    const int mv = carry;
    __syncthreads();                             // (sel is read by other threads of this workgroup)
    double best = 0.0;
    for (int e = threadIdx.x; e < mv; e += kBlock) {
        const int a = sl[e], b = sl[e + 1 < mv ? e + 1 : 0];
        const double dq = e + 1 < mv ? qb[b] - qb[a] : (qb[b] + 4.0) - qb[a];
        const double dot = csq[2 * (size_t)a] * csq[2 * (size_t)b] + csq[2 * (size_t)a + 1] * csq[2 * (size_t)b + 1];
        const double ra = (double)r[a], rb = (double)r[b];
        const double l = (rb < ra ? rb : ra) - bo;
        const double le = (dq < 2.0 && dot >= cg && l > 0.0) ? l : 0.0;
        q[row + e] = qb[a];
        lim[row + e] = le;
        const double l2 = le * le;
        best = l2 > best ? l2 : best;
    }
    best = block_reduce(best, OpMax(), shd, kBlock, 0.0);
    if (threadIdx.x == 0) { nvalid[blockIdx.x] = mv; lim2[blockIdx.x] = best; }
}

// ---- targets ------------------------------------------------------------------------------------------------------------------
struct TargetPred {
    const unsigned char* seen;
    const float* dist;
    float min_dist;
    __device__ bool operator()(int p) const { return !seen[p] && !(dist[p] < min_dist); }
};

// ---- the gather ---------------------------------------------------------------------------------------------------------------
// the kPoints targets of this thread as doubles of their float32 lattice points; ok: the slot lies inside the list
__device__ __forceinline__ void view_decode(const DfLattice& L, const int* __restrict__ list, int T, double (*x)[3], bool* ok) {
    const int nxy = L.nx * L.ny;
    const int base = blockIdx.x * (kBlock * kPoints);
#pragma unroll
    for (int a = 0; a < kPoints; ++a) {
        const int r = base + a * kBlock + threadIdx.x;
        ok[a] = r < T;
        const int p = ok[a] ? list[r] : 0;
        const int i = p % L.nx, j = (p / L.nx) % L.ny, k = p / nxy;
        x[a][0] = (double)(L.ox + (float)i * L.st);
        x[a][1] = (double)(L.oy + (float)j * L.st);
        x[a][2] = (double)(L.oz + (float)k * L.st);
    }
}

// the tile's counts summed over the wavefronts: one integer atomic per pose
__device__ __forceinline__ void view_flush(const int (*cnt)[kPoseTile], int k0, int nk, unsigned long long* __restrict__ gain) {
    if ((int)threadIdx.x < nk) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += cnt[w][threadIdx.x];
        if (c) atomicAdd(&gain[k0 + threadIdx.x], (unsigned long long)c);
    }
}

__global__ void __launch_bounds__(kBlock) view_gather_depth_kernel(DfLattice L, const int* __restrict__ list, int T,
                                                                   const float* __restrict__ pose, int m, double fx, double fy, double cx,
                                                                   double cy, int W, int H, const float* __restrict__ pred,
                                                                   const unsigned* __restrict__ dmax, double back_off,
                                                                   unsigned long long* __restrict__ gain) {
    __shared__ double shp[kPoseTile][13];        // the pose as doubles, then the cut: l.z below it or nothing
    __shared__ int cnt[kWaves][kPoseTile];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    double x[kPoints][3];
    bool ok[kPoints];
    view_decode(L, list, T, x, ok);
    const size_t n = (size_t)W * H;
    for (int k0 = blockIdx.y * kPoseTile; k0 < m; k0 += gridDim.y * kPoseTile) {
        const int nk = min(kPoseTile, m - k0);
        __syncthreads();                         // (the previous tile is read)
        for (int e = threadIdx.x; e < nk * 12; e += kBlock) shp[e / 12][e % 12] = (double)pose[(size_t)k0 * 12 + e];
        if ((int)threadIdx.x < nk) {
            const unsigned b = dmax[k0 + threadIdx.x];
            shp[threadIdx.x][12] = b ? (double)__uint_as_float(b) - back_off : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < nk; ++kk) {
            const double* P = shp[kk];
            const double t0 = P[0], t1 = P[1], t2 = P[2], cut = P[12];
            const float* dk = pred + (size_t)(k0 + kk) * n;
            int c = 0;
#pragma unroll
            for (int a = 0; a < kPoints; ++a) {
                bool s = false;
                if (ok[a]) {
                    const double d0 = x[a][0] - t0, d1 = x[a][1] - t1, d2 = x[a][2] - t2;
                    const double lz = P[9] * d0 + P[10] * d1 + P[11] * d2;
                    if (lz > 0.0 && lz < cut) {
                        const double lx = P[3] * d0 + P[4] * d1 + P[5] * d2;
                        const double ly = P[6] * d0 + P[7] * d1 + P[8] * d2;
                        const double u = floor(fx * lx / lz + cx + 0.5), v = floor(fy * ly / lz + cy + 0.5);
                        if (u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H) {
                            const double d = (double)dk[(int)u * H + (int)v];
                            s = d > 0.4 && d < 4.0 && lz < d - back_off;
                        }
                    }
                }
                c += __popcll(__ballot(s));
            }
            if (lane == 0) cnt[wv][kk] = c;
        }
        __syncthreads();
        view_flush(cnt, k0, nk, gain);
    }
}

__global__ void __launch_bounds__(kBlock) view_gather_scan_kernel(DfLattice L, const int* __restrict__ list, int T,
                                                                  const float* __restrict__ pose, int m, double off0, double off1, int n,
                                                                  const double* __restrict__ q, const double* __restrict__ lim,
                                                                  const int* __restrict__ nvalid, const double* __restrict__ lim2,
                                                                  unsigned long long* __restrict__ gain) {
    __shared__ double shp[kPoseTile][7];         // the pose as doubles, then the largest lim^2 of its sectors
    __shared__ int shn[kPoseTile];
    __shared__ int cnt[kWaves][kPoseTile];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    double x[kPoints][3];
    bool ok[kPoints];
    view_decode(L, list, T, x, ok);
    for (int k0 = blockIdx.y * kPoseTile; k0 < m; k0 += gridDim.y * kPoseTile) {
        const int nk = min(kPoseTile, m - k0);
        __syncthreads();                         // (the previous tile is read)
        for (int e = threadIdx.x; e < nk * 6; e += kBlock) shp[e / 6][e % 6] = (double)pose[(size_t)k0 * 6 + e];
        if ((int)threadIdx.x < nk) { shp[threadIdx.x][6] = lim2[k0 + threadIdx.x]; shn[threadIdx.x] = nvalid[k0 + threadIdx.x]; }
        __syncthreads();
        for (int kk = 0; kk < nk; ++kk) {
            const double* P = shp[kk];
            const double t0 = P[0], t1 = P[1], l2max = P[6];
            const int mv = shn[kk];
            const double* qk = q + (size_t)(k0 + kk) * n;
            const double* lk = lim + (size_t)(k0 + kk) * n;
            int c = 0;
            if (mv >= 2) {                       // (fewer than two valid beams: nothing is seen; uniform over the workgroup)
#pragma unroll
                for (int a = 0; a < kPoints; ++a) {
                    bool s = false;
                    if (ok[a]) {
                        const double d0 = x[a][0] - t0, d1 = x[a][1] - t1;
                        const double lx = (P[2] * d0 + P[3] * d1) - off0;
                        const double ly = (P[4] * d0 + P[5] * d1) - off1;
                        const double ll = lx * lx + ly * ly;
                        s = ll == 0.0;
                        if (!s && ll < l2max) {
                            const double e = lk[sector_of(qk, mv, pseudo_angle(lx, ly))];
                            s = ll < e * e;
                        }
                    }
                    c += __popcll(__ballot(s));
                }
            }
            if (lane == 0) cnt[wv][kk] = c;
        }
        __syncthreads();
        view_flush(cnt, k0, nk, gain);
    }
}

}  // namespace

ViewScorer::ViewScorer() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

ViewScorer::~ViewScorer() { (void)bind(-1); }

int ViewScorer::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_pose, (void*)d_hits, (void*)d_dmax, (void*)d_nvalid, (void*)d_lim2, (void*)d_gain, (void*)d_pred,
                        (void*)d_csq, (void*)d_ord, (void*)d_sel, (void*)d_sector, (void*)d_bcount, (void*)d_list})
            (void)hipFree(p);
        if (h_pose) (void)hipHostFree(h_pose);
        if (h_out) (void)hipHostFree(h_out);
        if (h_word) (void)hipHostFree(h_word);
        if (own) (void)hipStreamDestroy(own);
    }
    d_pose = nullptr; d_hits = nullptr; d_dmax = nullptr; d_nvalid = nullptr; d_lim2 = nullptr; d_gain = nullptr; d_pred = nullptr;
    d_csq = nullptr; d_ord = nullptr; d_sel = nullptr; d_sector = nullptr; d_bcount = nullptr; d_list = nullptr;
    h_pose = nullptr; h_out = nullptr; h_word = nullptr; own = nullptr;
    cap_pose = cap_m = cap_pred = cap_beams = cap_sector = cap_blocks = cap_list = cap_hpose = cap_hout = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int ViewScorer::score(const DistanceField& df, const Coverage& cv, const SensorFrame& f, const float* pose, int m, const gpis_view_opts& vo,
                      hipStream_t s) {
    clear_result();
    const int dm = f.geo.dim, PN = dm == 3 ? 12 : 6;
    const size_t M = (size_t)m, n = (size_t)f.n;
    RenderFieldOpts o;
    o.tnear = vo.march.tnear; o.tfar = vo.march.tfar; o.min_step = vo.march.min_step; o.max_step = vo.march.max_step;
    o.slack = vo.march.slack; o.refine = vo.march.refine; o.max_steps = vo.march.max_steps;

    // the buffers
    if (int rc = grow(d_pose, cap_pose, M * PN)) return rc;
    if (M > cap_m) {
        for (void* p : {(void*)d_hits, (void*)d_dmax, (void*)d_nvalid, (void*)d_lim2, (void*)d_gain}) (void)hipFree(p);
        d_hits = nullptr; d_dmax = nullptr; d_nvalid = nullptr; d_lim2 = nullptr; d_gain = nullptr; cap_m = 0;
        GPIS_HIP(hipMalloc((void**)&d_hits, sizeof(int) * M));
        GPIS_HIP(hipMalloc((void**)&d_dmax, sizeof(unsigned) * M));
        GPIS_HIP(hipMalloc((void**)&d_nvalid, sizeof(int) * M));
        GPIS_HIP(hipMalloc((void**)&d_lim2, sizeof(double) * M));
        GPIS_HIP(hipMalloc((void**)&d_gain, sizeof(unsigned long long) * (M + 1)));
        cap_m = M;
    }
    if (int rc = grow(d_pred, cap_pred, M * n)) return rc;
    if (dm == 2) {
        if (n > cap_beams) {
            (void)hipFree(d_csq); (void)hipFree(d_ord); d_csq = nullptr; d_ord = nullptr; cap_beams = 0;
            GPIS_HIP(hipMalloc((void**)&d_csq, sizeof(double) * 3 * n));
            GPIS_HIP(hipMalloc((void**)&d_ord, sizeof(int) * n));
            cap_beams = n;
        }
        if (M * n > cap_sector) {
            (void)hipFree(d_sel); (void)hipFree(d_sector); d_sel = nullptr; d_sector = nullptr; cap_sector = 0;
            GPIS_HIP(hipMalloc((void**)&d_sel, sizeof(int) * M * n));
            GPIS_HIP(hipMalloc((void**)&d_sector, sizeof(double) * 2 * M * n));
            cap_sector = M * n;
        }
    }
    if (M * PN > cap_hpose) {
        if (h_pose) (void)hipHostFree(h_pose);
        h_pose = nullptr; cap_hpose = 0;
        GPIS_HIP(hipHostMalloc((void**)&h_pose, sizeof(float) * M * PN));
        cap_hpose = M * PN;
    }
    const size_t out_bytes = sizeof(unsigned long long) * (M + 1) + sizeof(int) * M;
    if (out_bytes > cap_hout) {
        if (h_out) (void)hipHostFree(h_out);
        h_out = nullptr; cap_hout = 0;
        GPIS_HIP(hipHostMalloc((void**)&h_out, out_bytes));
        cap_hout = out_bytes;
    }
    if (!h_word) GPIS_HIP(hipHostMalloc((void**)&h_word, sizeof(int)));

    // 1. the predicted measurements
    auto t0 = std::chrono::steady_clock::now();
    std::memcpy(h_pose, pose, sizeof(float) * M * PN);
    GPIS_HIP(hipMemcpyAsync(d_pose, h_pose, sizeof(float) * M * PN, hipMemcpyHostToDevice, s));
    GPIS_HIP(hipMemsetAsync(d_hits, 0, sizeof(int) * M, s));
    GPIS_HIP(hipMemsetAsync(d_dmax, 0, sizeof(unsigned) * M, s));
    GPIS_HIP(hipMemsetAsync(d_gain, 0, sizeof(unsigned long long) * (M + 1), s));
    std::vector<double> hq;
    std::vector<int> hord;
    if (dm == 2) {
        view_order_table(f.cs.data(), f.n, &hq, &hord);
        GPIS_HIP(hipMemcpyAsync(d_csq, f.cs.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        GPIS_HIP(hipMemcpyAsync(d_csq + 2 * n, hq.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
        GPIS_HIP(hipMemcpyAsync(d_ord, hord.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    }
    const DfLattice DL = df.lattice();
    float lo[3] = {DL.ox, DL.oy, DL.oz}, hi[3];
    const int ln[3] = {DL.nx, DL.ny, DL.nz};
    for (int a = 0; a < 3; ++a) hi[a] = lo[a] + (float)(ln[a] - 1) * DL.st;
    const long long wpp = dm == 3 ? (long long)((f.geo.width + 7) / 8) * ((f.geo.height + 7) / 8) : ((long long)n + kWave - 1) / kWave;
    const long long nbp = (wpp * m + kWaves - 1) / kWaves;
    if (dm == 3)
        hipLaunchKernelGGL(view_predict_kernel<3>, dim3((unsigned)nbp), dim3(kBlock), 0, s, f.geo, d_pose, m, (const double*)nullptr, (int)n,
                           (int)wpp, o, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], df.d_dist, DL, vo.miss, d_pred, d_hits, d_dmax, d_gain + M);
    else
        hipLaunchKernelGGL(view_predict_kernel<2>, dim3((unsigned)nbp), dim3(kBlock), 0, s, f.geo, d_pose, m, d_csq, (int)n, (int)wpp, o,
                           lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], df.d_dist, DL, vo.miss, d_pred, d_hits, d_dmax, d_gain + M);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));           // (the order table lives until here)
    predict_ms = ms_since(t0);

    // 2. the sector table of every pose
    if (dm == 2) {
        t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(view_sector_kernel, dim3(m), dim3(kBlock), 0, s, d_pred, d_csq, d_ord, (int)n, (double)vo.back_off,
                           std::cos((double)vo.max_gap), d_sel, d_sector, d_sector + M * n, d_nvalid, d_lim2);
        GPIS_HIP(hipGetLastError());
        GPIS_HIP(hipStreamSynchronize(s));
        table_ms = ms_since(t0);
    }

    // 3. the targets
    t0 = std::chrono::steady_clock::now();
    const int np = (int)cv.ngrid;
    if (int rc = grow(d_bcount, cap_blocks, (size_t)(np + kCompactChunk - 1) / kCompactChunk + 1)) return rc;
    auto grow_list = [&](int cnt) -> int { return grow(d_list, cap_list, (size_t)std::max(1, cnt)); };
    int T = 0;
    int* no_rank = nullptr;
    if (int rc = compact_run(TargetPred{cv.d_seen, df.d_dist, vo.min_dist}, np, d_bcount, h_word, &T, d_list, no_rank, s, grow_list)) return rc;
    GPIS_HIP(hipStreamSynchronize(s));
    target_ms = ms_since(t0);

    // 4. the gather (no target: nothing is launched, the gains stay zero)
    t0 = std::chrono::steady_clock::now();
    if (T > 0) {
        // blocks (x, y): chunk x of the targets against the pose tiles y, y + ny, ...; a short list spreads its tiles over more
        // workgroups (a pose still lies in one tile, so it still gets one atomic per workgroup that meets it)
        const int nbx = (T + kBlock * kPoints - 1) / (kBlock * kPoints), tiles = (m + kPoseTile - 1) / kPoseTile;
        const dim3 nb(nbx, std::max(1, std::min(tiles, kGridCap / nbx)));
        if (dm == 3)
            hipLaunchKernelGGL(view_gather_depth_kernel, nb, dim3(kBlock), 0, s, DL, d_list, T, d_pose, m, (double)f.geo.fx, (double)f.geo.fy,
                               (double)f.geo.cx, (double)f.geo.cy, f.geo.width, f.geo.height, d_pred, d_dmax, (double)vo.back_off, d_gain);
        else
            hipLaunchKernelGGL(view_gather_scan_kernel, nb, dim3(kBlock), 0, s, DL, d_list, T, d_pose, m, (double)f.geo.off[0],
                               (double)f.geo.off[1], (int)n, d_sector, d_sector + M * n, d_nvalid, d_lim2, d_gain);
        GPIS_HIP(hipGetLastError());
    }
    unsigned long long* hg = (unsigned long long*)h_out;
    int* hh = (int*)(h_out + sizeof(unsigned long long) * (M + 1));
    GPIS_HIP(hipMemcpyAsync(hg, d_gain, sizeof(unsigned long long) * (M + 1), hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipMemcpyAsync(hh, d_hits, sizeof(int) * M, hipMemcpyDeviceToHost, s));
    GPIS_HIP(hipStreamSynchronize(s));
    gather_ms = ms_since(t0);

    gain.resize(M); hits.resize(M);
    for (size_t k = 0; k < M; ++k) { gain[k] = (long long)hg[k]; hits[k] = hh[k]; }
    dim = dm; poses = m; rays = f.n; targets = T; samples = (long long)hg[M];
    valid = true;
    return GPIS_OK;
}

int ViewScorer::predicted(int k, float* out) {
    if (!valid || k < 0 || k >= poses) return GPIS_ERR_STATE;
    GPIS_HIP(hipMemcpyAsync(out, d_pred + (size_t)k * rays, sizeof(float) * (size_t)rays, hipMemcpyDeviceToHost, own));
    GPIS_HIP(hipStreamSynchronize(own));
    return GPIS_OK;
}

}  // namespace gpis
