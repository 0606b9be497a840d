// The distance field's sampler on the device, shared by gpis_dfield_sample (dfield.hip) and the field tracker
// (track.hip).  The library builds with -ffp-contract=off, so every caller gets the same operation order and the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace gpis {

// a field's lattice: dim, the point counts (nz = 1 in 2-D), the origin (oz = 0 in 2-D) and the step
struct DfLattice {
    int dim, nx, ny, nz;
    float ox, oy, oz, st;
};

__device__ __forceinline__ float df_lerp(float a, float b, float w) { return a + w * (b - a); }

// o[0] = trilinear / bilinear interpolant of the lattice values F at (x, y, z) (z unused in 2-D), o[1 + a] = its derivative
// along axis a; all NaN outside the lattice (DESIGN §7e's operation order)
__device__ __forceinline__ void df_sample_at(const float* __restrict__ F, const DfLattice& L, float x, float y, float z,
                                             float* __restrict__ o) {
    const int dim = L.dim, nx = L.nx, ny = L.ny, nz = L.nz;
    const float st = L.st;
    const long long nxy = (long long)nx * ny;
    const float ux = (x - L.ox) / st, uy = (y - L.oy) / st, uz = dim == 3 ? (z - L.oz) / st : 0.f;
    const bool in = (ux >= 0.f && ux <= (float)(nx - 1)) && (uy >= 0.f && uy <= (float)(ny - 1)) &&
                    (dim == 2 || (uz >= 0.f && uz <= (float)(nz - 1)));
    if (!in) {
        for (int a = 0; a <= dim; ++a) o[a] = __int_as_float(0x7fc00000);
        return;
    }
    const int i0 = min((int)floorf(ux), nx - 2), j0 = min((int)floorf(uy), ny - 2);
    const float wx = ux - (float)i0, wy = uy - (float)j0;
    const long long b = (long long)j0 * nx + i0;
    if (dim == 2) {
        const float c00 = F[b], c10 = F[b + 1], c01 = F[b + nx], c11 = F[b + nx + 1];
        const float e0 = df_lerp(c00, c10, wx), e1 = df_lerp(c01, c11, wx);
        o[0] = df_lerp(e0, e1, wy);
        o[1] = df_lerp(c10 - c00, c11 - c01, wy) / st;
        o[2] = (e1 - e0) / st;
        return;
    }
    const int k0 = min((int)floorf(uz), nz - 2);
    const float wz = uz - (float)k0;
    const long long b0 = b + k0 * nxy, b1 = b0 + nxy;
    const float c000 = F[b0], c100 = F[b0 + 1], c010 = F[b0 + nx], c110 = F[b0 + nx + 1];
    const float c001 = F[b1], c101 = F[b1 + 1], c011 = F[b1 + nx], c111 = F[b1 + nx + 1];
    // e_{dy dz}: x lerps; f_{dz}: y lerps
    const float e00 = df_lerp(c000, c100, wx), e10 = df_lerp(c010, c110, wx), e01 = df_lerp(c001, c101, wx),
                e11 = df_lerp(c011, c111, wx);
    const float f0 = df_lerp(e00, e10, wy), f1 = df_lerp(e01, e11, wy);
    o[0] = df_lerp(f0, f1, wz);
    const float hy0 = df_lerp(c100 - c000, c110 - c010, wy), hy1 = df_lerp(c101 - c001, c111 - c011, wy);
    o[1] = df_lerp(hy0, hy1, wz) / st;
    o[2] = df_lerp(e10 - e00, e11 - e01, wz) / st;
    o[3] = (f1 - f0) / st;
}

}  // namespace gpis
