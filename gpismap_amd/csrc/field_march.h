// The rays of a render and the sphere-tracing march of one ray through a distance field, device only: the
// set-up and world point of a ray, and the march itself.  render.hip's kernels and the batched prediction of view.hip include
// this header, so a ray takes the same samples in the same order wherever it is marched.  The library builds with
// -ffp-contract=off: every caller gets the same operations and the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "dfield_sample.h"
#include "render.h"

namespace gpis {

constexpr int kRayRunning = 255;      // status of a ray still marching

// the world point of parameter z on a ray: 3-D from its (u, v); 2-D from its host-double (c, s)
__device__ __forceinline__ void world_point_at(const RayGeom& g, float u, float v, double c, double s, float z, float& p0, float& p1,
                                               float& p2) {
    if (g.dim == 3) {
        const float xl = u * z, yl = v * z;
        p0 = g.R[0] * xl + g.R[3] * yl + g.R[6] * z + g.t[0];
        p1 = g.R[1] * xl + g.R[4] * yl + g.R[7] * z + g.t[1];
        p2 = g.R[2] * xl + g.R[5] * yl + g.R[8] * z + g.t[2];
    } else {
        const float xl = (float)((double)z * c) + g.off[0];
        const float yl = (float)((double)z * s) + g.off[1];
        p0 = g.R[0] * xl + g.R[2] * yl + g.t[0];
        p1 = g.R[1] * xl + g.R[3] * yl + g.t[1];
        p2 = 0.f;
    }
}

// Set-up of ray i: its direction terms (3-D: u, v, il = 1 / sqrt(u^2 + v^2 + 1); 2-D: c, s of the beam), then the slab clip of
// [tnear, tfar] against the box [lo, hi] (IEEE division; fmin / fmax drop the NaN of an axis the ray runs in the plane of)
// into [t0, t1].
__device__ __forceinline__ void ray_setup(const RayGeom& g, const double* __restrict__ cs, int i, float tnear, float tfar,
                                          const float* lo, const float* hi, float& u, float& v, float& il, double& cd, double& sd,
                                          float& t0, float& t1) {
    float o[3], d[3];
    if (g.dim == 3) {
        const int col = i / g.height, row = i - col * g.height;
        u = ((float)col - g.cx) / g.fx; v = ((float)row - g.cy) / g.fy;
        il = 1.0f / sqrtf(u * u + v * v + 1.0f);
        cd = sd = 0.0;
        for (int a = 0; a < 3; ++a) { o[a] = g.t[a]; d[a] = g.R[a] * u + g.R[3 + a] * v + g.R[6 + a]; }
    } else {
        cd = cs[2 * (size_t)i]; sd = cs[2 * (size_t)i + 1];
        u = v = 0.f; il = 1.0f;
        const float c = (float)cd, s = (float)sd;
        o[0] = g.R[0] * g.off[0] + g.R[2] * g.off[1] + g.t[0];
        o[1] = g.R[1] * g.off[0] + g.R[3] * g.off[1] + g.t[1];
        d[0] = g.R[0] * c + g.R[2] * s;
        d[1] = g.R[1] * c + g.R[3] * s;
    }
    t0 = tnear; t1 = tfar;
    for (int a = 0; a < g.dim; ++a) {
        const float ta = (lo[a] - o[a]) / d[a], tb = (hi[a] - o[a]) / d[a];
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    }
}

// One ray from the near end z of its clipped interval [z, zend] to its status: one loop whose every turn takes one sample of the
// field -- a march sample, a bisection midpoint or the final secant point, by the ray's phase -- so the lanes of a wavefront
// share one sampler whatever their phases.  Step, hit, refinement and status: tests/render_field_ref.py.  Returns the status
// (0 hit, 1 left the interval, 2 step limit); on a hit q is the reported parameter and smp the sample there.  ns: samples taken.
template <int D>
__device__ __forceinline__ int field_march(const RayGeom& g, float u, float v, float il, double cd, double sd, float z, float zend,
                                           const RenderFieldOpts& o, const float* __restrict__ F, const DfLattice& L, float& q,
                                           float* __restrict__ smp, int& ns) {
    const float sl = o.slack * L.st;
    float zlo = 0.f, glo = 0.f, ghi = 0.f;
    q = z;
    int st = (z <= zend) ? kRayRunning : 1;
    int phase = 0, nstep = 0, round = 0;     // phase 0 march, 1 bisection, 2 the final sample
    bool has = false;
    while (st == kRayRunning) {
        float p0, p1, p2;
        world_point_at(g, u, v, cd, sd, q, p0, p1, p2);
        df_sample_at(F, L, p0, p1, p2, smp);
        ++ns;
        const float d = smp[0];
        if (phase == 0) {
            if (has && d < 0.f && !(glo < 0.f)) {
                ghi = d;                     // bracket [zlo, z]
                phase = o.refine > 0 ? 1 : 2;
            } else {
                zlo = z; glo = d; has = true;
                if (++nstep >= o.max_steps) { st = 2; break; }
                const float ds = isnan(d) ? o.min_step : fminf(fmaxf(fabsf(d) - sl, o.min_step), o.max_step);
                const float zn = z + (D == 3 ? ds * il : ds);
                if (!(zn <= zend)) { st = 1; break; }
                z = zn; q = zn;
                continue;
            }
        } else if (phase == 1) {
            if (d < 0.f) { z = q; ghi = d; }
            else { zlo = q; glo = d; }
            if (++round >= o.refine) phase = 2;
        } else {
            st = 0;
            break;
        }
        if (phase == 1) {
            q = zlo + (z - zlo) * 0.5f;
        } else if (isnan(glo)) {
            q = z;
        } else {
            q = zlo + (z - zlo) * (glo / (glo - ghi));
            q = fminf(fmaxf(q, zlo), z);
        }
    }
    return st;
}

}  // namespace gpis
