// Signed Euclidean distance field (dfield.h).  Memory-bound passes: grid-stride loops over at most kGridCap blocks of
// 256 threads (cdna_hip_programming.md Guideline 11).
//
// Lattice point (i, j, k): index p = (k ny + j) nx + i, coordinates o + (float)i * s (no FMA: -ffp-contract=off).  Inside iff
// f < level; f NaN is outside.  Site: f finite and an axis neighbour with a finite f on the other side of the level.
//
// Distance transform: feat(p) = nearest feature so far (-1: none); the x pass starts from feat = p at sites.  Pass along axis a,
// one thread per line: new(p) = argmin over q on the line of (p_a - q_a)^2 + g(q), g(q) = |q - feat(q)|^2 (feat(q) shares q's
// coordinate a, so this is |p - feat(q)|^2), the smallest q_a on ties.  The lower envelope of these parabolas (Felzenszwalb /
// Meijster) in exact integers: for q < r, q wins at every integer p <= floor(S), S = ((g_r + r^2) - (g_q + q^2)) / (2 (r - q)),
// so r starts at floor(S) + 1.  Stack slot k of line t lives at ws[k L + t] (L lines), so that neighbouring lines' threads
// coalesce; a parabola that would start past the line's end is not pushed.
#include <algorithm>
#include <cmath>
#include "dfield.h"
#include "dfield_sample.h"
#include "map_query.h"
#include "mesh.h"

namespace gpis {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ bool crosses(float fa, float fb, float level) {
    return isfinite(fa) && isfinite(fb) && ((fa < level) != (fb < level));
}

// feat[p] = p at sites, -1 elsewhere
__global__ void __launch_bounds__(kBlock) df_site_kernel(const float* __restrict__ val, int dim, int nx, int ny, int nz, float level,
                                                         int* __restrict__ feat) {
    const int nxy = nx * ny, n = nxy * nz;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int i = p % nx, j = (p / nx) % ny, k = p / nxy;
        const float f = val[p];
        bool s = false;
        if (isfinite(f)) {
            s = (i > 0 && crosses(f, val[p - 1], level)) || (i < nx - 1 && crosses(f, val[p + 1], level)) ||
                (j > 0 && crosses(f, val[p - nx], level)) || (j < ny - 1 && crosses(f, val[p + nx], level));
            if (dim == 3) s = s || (k > 0 && crosses(f, val[p - nxy], level)) || (k < nz - 1 && crosses(f, val[p + nxy], level));
        }
        feat[p] = s ? p : -1;
    }
}

__device__ __forceinline__ int sq_dist(int p, int q, int nx, int ny) {
    const int nxy = nx * ny;
    const int di = p % nx - q % nx, dj = (p / nx) % ny - (q / nx) % ny, dk = p / nxy - q / nxy;
    return di * di + dj * dj + dk * dk;
}

__device__ __forceinline__ int floor_div(int a, int b) {     // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// One envelope pass along axis `ax` (0 x, 1 y, 2 z) over all lines: in -> out.
__global__ void __launch_bounds__(kBlock) df_pass_kernel(const int* __restrict__ in, int* __restrict__ out, int* __restrict__ ws, int ax,
                                                         int nx, int ny, int nz) {
    const int na = ax == 0 ? nx : (ax == 1 ? ny : nz);
    const int nlines = nx * ny * nz / na;
    const int stride = ax == 0 ? 1 : (ax == 1 ? nx : nx * ny);
    const size_t L = (size_t)nlines;
    int* __restrict__ V = ws;
    int* __restrict__ G = ws + L * na;
    int* __restrict__ Z = ws + 2 * L * na;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nlines; t += gridDim.x * blockDim.x) {
        const int base = ax == 0 ? t * nx : (ax == 1 ? (t / nx) * nx * ny + t % nx : t);
        int k = -1;
        for (int q = 0; q < na; ++q) {
            const int p = base + q * stride;
            const int f = in[p];
            if (f < 0) continue;
            const int g = sq_dist(p, f, nx, ny);
            int s = 0;
            while (k >= 0) {
                const size_t sk = (size_t)k * L + t;
                const int v = V[sk];
                s = floor_div((g + q * q) - (G[sk] + v * v), 2 * (q - v)) + 1;
                if (s <= Z[sk]) --k;
                else break;
            }
            if (k < 0) {
                k = 0;
                V[t] = q; G[t] = g; Z[t] = 0;
            } else if (s < na) {
                ++k;
                const size_t sk = (size_t)k * L + t;
                V[sk] = q; G[sk] = g; Z[sk] = s;
            }
        }
        if (k < 0) {
            for (int q = 0; q < na; ++q) out[base + q * stride] = -1;
            continue;
        }
        int j = 0, next = k > 0 ? Z[L + t] : na;
        int vj = V[t];
        for (int q = 0; q < na; ++q) {
            while (next <= q) {
                ++j;
                vj = V[(size_t)j * L + t];
                next = j < k ? Z[(size_t)(j + 1) * L + t] : na;
            }
            out[base + q * stride] = in[base + vj * stride];
        }
    }
}

// dist from the anchor of each point's nearest site (recomputed from f around it: the mesh vertex of the crossed axis edge
// closest along its axis, ties to the first edge of -x, +x, -y, +y, -z, +z)
__global__ void __launch_bounds__(kBlock) df_output_kernel(const float* __restrict__ val, const int* __restrict__ feat, int dim, int nx,
                                                           int ny, int nz, float ox, float oy, float oz, float st, float level,
                                                           float* __restrict__ dist) {
    const int nxy = nx * ny, n = nxy * nz;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const float fp = val[p];
        const bool inside = fp < level;
        const int q = feat[p];
        if (q < 0) {
            dist[p] = inside ? -INFINITY : INFINITY;
            continue;
        }
        const int qi[3] = {q % nx, (q / nx) % ny, q / nxy};
        const int qs[3] = {1, nx, nxy};
        const int qn[3] = {nx, ny, nz};
        const float qo[3] = {ox, oy, oz};
        float c[3] = {ox + (float)qi[0] * st, oy + (float)qi[1] * st, oz + (float)qi[2] * st};
        const float fq = val[q];
        float best = INFINITY, cx = 0.f;
        int ba = -1;
        for (int a = 0; a < dim; ++a) {
            for (int sg = -1; sg <= 1; sg += 2) {
                const int ia = qi[a] + sg;
                if (ia < 0 || ia >= qn[a]) continue;
                const float fo = val[q + sg * qs[a]];
                if (!crosses(fq, fo, level)) continue;
                const int ilo = sg < 0 ? ia : qi[a];
                const float fa = sg < 0 ? fo : fq, fb = sg < 0 ? fq : fo;
                const float t = (level - fa) / (fb - fa);
                const float xa = qo[a] + (float)ilo * st, xb = qo[a] + (float)(ilo + 1) * st;
                const float x = xa + t * (xb - xa);
                const float d = fabsf(x - c[a]);
                if (d < best) { best = d; cx = x; ba = a; }
            }
        }
        if (ba == 0) c[0] = cx;
        else if (ba == 1) c[1] = cx;
        else if (ba == 2) c[2] = cx;
        const int pi = p % nx, pj = (p / nx) % ny, pk = p / nxy;
        const float dx = (ox + (float)pi * st) - c[0], dy = (oy + (float)pj * st) - c[1];
        float s2 = dx * dx + dy * dy;
        if (dim == 3) {
            const float dz = (oz + (float)pk * st) - c[2];
            s2 = s2 + dz * dz;
        }
        const float r = sqrtf(s2);
        dist[p] = inside ? -r : r;
    }
}

// out[q][0] = trilinear / bilinear interpolant, out[q][1 + a] = its derivative along axis a (df_sample_at)
__global__ void __launch_bounds__(kBlock) df_sample_kernel(const float* __restrict__ F, DfLattice L, const float* __restrict__ x, long long m,
                                                           float* __restrict__ out) {
    const int dim = L.dim;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (long long)gridDim.x * blockDim.x) {
        const float* xq = x + (size_t)q * dim;
        df_sample_at(F, L, xq[0], xq[1], dim == 3 ? xq[2] : 0.f, out + (size_t)q * (1 + dim));
    }
}

}  // namespace

int dfield_check_lattice(int dim, const int* n, const float* origin, const float* step, long long* npts) {
    const int rc = mesh_check_lattice(dim, n, origin, step, npts);
    if (rc == GPIS_ERR_ARG) return rc;
    for (int a = 1; a < dim; ++a)
        if (!(step[a] == step[0])) return GPIS_ERR_ARG;       // (cubic cells: exact integer distances)
    if (rc) return rc;
    for (int a = 0; a < dim; ++a)
        if (n[a] > DistanceField::kMaxAxis) return GPIS_ERR_LIMIT;
    return GPIS_OK;
}

DistanceField::DistanceField() {
    (void)hipGetDevice(&device);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
}

DistanceField::~DistanceField() { (void)bind(-1); }

int DistanceField::bind(int dev) {
    if (dev == device && dev >= 0) return GPIS_OK;
    {
        DeviceScope ds(device);
        if (own) (void)hipStreamSynchronize(own);
        for (void* p : {(void*)d_val, (void*)d_feat[0], (void*)d_feat[1], (void*)d_dist, (void*)d_ws, (void*)d_x, (void*)d_rec})
            (void)hipFree(p);
        if (own) (void)hipStreamDestroy(own);
    }
    d_val = nullptr; d_feat[0] = d_feat[1] = nullptr; d_dist = nullptr; d_ws = nullptr; d_x = nullptr; d_rec = nullptr; own = nullptr;
    cap_n = cap_x = cap_rec = 0;
    clear_result();
    device = dev;
    if (dev < 0) return GPIS_OK;
    DeviceScope ds(dev);
    GPIS_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    return GPIS_OK;
}

int DistanceField::ensure(long long np) {
    if ((size_t)np <= cap_n) return GPIS_OK;
    for (void* p : {(void*)d_val, (void*)d_feat[0], (void*)d_feat[1], (void*)d_dist, (void*)d_ws}) (void)hipFree(p);
    d_val = nullptr; d_feat[0] = d_feat[1] = nullptr; d_dist = nullptr; d_ws = nullptr; cap_n = 0;
    GPIS_HIP(hipMalloc((void**)&d_val, sizeof(float) * np));
    GPIS_HIP(hipMalloc((void**)&d_feat[0], sizeof(int) * np));
    GPIS_HIP(hipMalloc((void**)&d_feat[1], sizeof(int) * np));
    GPIS_HIP(hipMalloc((void**)&d_dist, sizeof(float) * np));
    GPIS_HIP(hipMalloc((void**)&d_ws, sizeof(int) * 3 * np));
    cap_n = (size_t)np;
    return GPIS_OK;
}

int DistanceField::from_grid(const float* d_values, int dm, const int* nn, const float* org, const float* stp, float level,
                             hipStream_t s) {
    long long np = 0;
    if (int rc = dfield_check_lattice(dm, nn, org, stp, &np)) return rc;
    if (int rc = ensure(np)) return rc;
    const int nx = nn[0], ny = nn[1], nz = dm == 3 ? nn[2] : 1;
    const float ox = org[0], oy = org[1], oz = dm == 3 ? org[2] : 0.f, st = stp[0];
    hipLaunchKernelGGL(df_site_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, d_values, dm, nx, ny, nz, level, d_feat[0]);
    GPIS_HIP(hipGetLastError());
    int cur = 0;
    for (int a = 0; a < dm; ++a) {
        const int na = a == 0 ? nx : (a == 1 ? ny : nz);
        hipLaunchKernelGGL(df_pass_kernel, dim3(grid_for(np / na)), dim3(kBlock), 0, s, d_feat[cur], d_feat[cur ^ 1], d_ws, a, nx, ny, nz);
        GPIS_HIP(hipGetLastError());
        cur ^= 1;
    }
    hipLaunchKernelGGL(df_output_kernel, dim3(grid_for(np)), dim3(kBlock), 0, s, d_values, d_feat[cur], dm, nx, ny, nz, ox, oy, oz, st,
                       level, d_dist);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    dim = dm; ngrid = np; site_buf = cur; step = st;
    for (int a = 0; a < 3; ++a) { n[a] = a < dm ? nn[a] : 1; origin[a] = a < dm ? org[a] : 0.f; }
    valid = true;
    return GPIS_OK;
}

int DistanceField::from_map(MapQuery& mq, OnGPISStore& store, int dm, const int* nn, const float* org, const float* stp, float level,
                            float max_var, hipStream_t s) {
    long long np = 0;
    if (int rc = dfield_check_lattice(dm, nn, org, stp, &np)) return rc;
    if (int rc = ensure(np)) return rc;
    if (int rc = lattice_values(mq, store, dm, nn, org, stp, np, chunk, max_var, d_x, cap_x, d_rec, cap_rec, d_val, s)) return rc;
    if (int rc = from_grid(d_val, dm, nn, org, stp, level, s)) return rc;
    f_valid = true;
    return GPIS_OK;
}

int DistanceField::sample(const float* d_xs, long long m, float* d_out, hipStream_t s) {
    if (!valid) return GPIS_ERR_STATE;
    if (m <= 0) return GPIS_OK;
    hipLaunchKernelGGL(df_sample_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, d_dist, lattice(), d_xs, m, d_out);
    GPIS_HIP(hipGetLastError());
    GPIS_HIP(hipStreamSynchronize(s));
    return GPIS_OK;
}

}  // namespace gpis
