"""Reference for rendering from a distance field (csrc/render.hip, gpis3_render_depth_field / gpis2_render_scan_field, DESIGN.md
§7g): a vectorised numpy float32 restatement of the sphere-tracing contract.  The rays, the parameter, the world point and the
slab clip are render_ref's (imported, not restated); the sample is dfield_ref.sample.  It imports nothing from gpismap_amd.

Contract (per ray, all float32, no fused multiply-add):
- clip [tnear, tfar] against the lattice box [o, o + f32(n - 1) * step] per axis; empty: status 1 without a sample;
- sample d and its gradient at the world point of the parameter; inside iff d < 0 (the field's level is zero); NaN (outside the
  lattice) counts as outside / unknown;
- hit: a sample with d < 0 whose previous sample was not inside (d >= 0 or NaN); the first sample of a ray is never a hit;
- otherwise the sample is counted; after max_steps counted samples the ray stops with status 2; else it advances by
  fmin(fmax(|d| - slack * step, min_step), max_step) of arc length (min_step where d is NaN; z steps are arc length times
  1 / sqrt(u^2 + v^2 + 1) in 3-D) and stops with status 1 once the parameter is not <= the end of its interval;
- a hit's bracket [lo, hi] is halved `refine` times at lo + (hi - lo) * 0.5 (d < 0 moves hi, anything else lo), then sampled once
  more at the secant point lo + (hi - lo) * (d_lo / (d_lo - d_hi)) clamped into the bracket (hi when d_lo is NaN): that parameter
  and that sample [d, grad] are the output.  No hit: NaN.
Counters: every sample taken (march, bisection, final), the hits, the largest number of samples a single ray took."""
import numpy as np

import dfield_ref
import render_ref

F32 = np.float32
NAN = F32(np.nan)


class Opts:
    """The march options of a field of lattice step `step` (gpis_render_field_default_opts)."""

    def __init__(self, dim, step, **kw):
        if dim == 3:
            d = dict(tnear=0.4, tfar=4.0, max_steps=512)
        else:
            d = dict(tnear=0.2, tfar=30.0, max_steps=1024)
        d.update(min_step=F32(step) * F32(0.5), max_step=np.inf, slack=3.0, refine=8)
        for k in kw:
            if k not in d:
                raise TypeError("unknown option %r" % k)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


def box(shape, origin, step):
    """(lo, hi) float32 of the lattice: [o, o + f32(n - 1) * step] per axis."""
    st = F32(step)
    lo = np.array([F32(v) for v in origin], F32)
    hi = np.array([F32(origin[a]) + F32(shape[a] - 1) * st for a in range(len(shape))], F32)
    return lo, hi


def march(sample_fn, dim, n, point_fn, il, t0, t1, go, step, o, trace=None):
    """sample_fn(x [m, dim] f32) -> [m, 1 + dim] f32; point_fn(idx, param) -> world points.  Returns (depth, rec, status, stats);
    stats also holds the per-ray sample counts ("per_ray") and the final brackets of the hits ("bracket": idx, lo, hi, d_lo,
    d_hi).  trace(idx, param, x, s, ds): called for every march pass with the unclamped step |d| - slack * step of its samples."""
    nc = 1 + dim
    mn, mx = F32(o.min_step), F32(o.max_step)
    sl = F32(o.slack) * F32(step)
    z, zend = t0.copy(), t1.copy()
    zlo = np.zeros(n, F32); glo = np.zeros(n, F32); ghi = np.zeros(n, F32)
    has = np.zeros(n, bool); nstep = np.zeros(n, np.int64); nsamp = np.zeros(n, np.int64)
    status = np.where(go, 255, 1).astype(np.uint8)
    depth = np.full(n, NAN, F32)
    rec = np.full((n, nc), NAN, F32)
    act = np.nonzero(go)[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while act.size:
            x = point_fn(act, z[act])
            r = sample_fn(x)
            nsamp[act] += 1
            g = r[:, 0]
            hit = has[act] & (g < 0) & ~(glo[act] < 0)
            ghi[act[hit]] = g[hit]
            status[act[hit]] = 0
            a, ga = act[~hit], g[~hit]
            zlo[a] = z[a]; glo[a] = ga; has[a] = True
            nstep[a] += 1
            lim = nstep[a] >= o.max_steps
            status[a[lim]] = 2
            a, ga = a[~lim], ga[~lim]
            raw = (np.abs(ga) - sl).astype(F32)
            if trace is not None:
                keep = ~hit
                keep[keep] = ~lim
                trace(a, z[a], x[keep], r[keep], raw)
            ds = np.where(np.isnan(ga), mn, np.fmin(np.fmax(raw, mn), mx)).astype(F32)
            zn = (z[a] + (ds * il[a] if dim == 3 else ds)).astype(F32)
            out = ~(zn <= zend[a])
            status[a[out]] = 1
            z[a[~out]] = zn[~out]
            act = a[~out]
        H = np.nonzero(status == 0)[0]
        if H.size:
            for _ in range(o.refine):
                q = (zlo[H] + (z[H] - zlo[H]) * F32(0.5)).astype(F32)
                g = sample_fn(point_fn(H, q))[:, 0]
                nsamp[H] += 1
                ins = g < 0
                z[H[ins]] = q[ins]; ghi[H[ins]] = g[ins]
                zlo[H[~ins]] = q[~ins]; glo[H[~ins]] = g[~ins]
            a, b, ga = zlo[H], z[H], glo[H]
            sec = np.fmin(np.fmax((a + (b - a) * (ga / (ga - ghi[H]))).astype(F32), a), b)
            q = np.where(np.isnan(ga), b, sec).astype(F32)
            r = sample_fn(point_fn(H, q))
            nsamp[H] += 1
            depth[H] = q
            rec[H] = r
    stats = dict(samples=int(nsamp.sum()), hits=int(H.size), max_samples=int(nsamp.max()) if n else 0, per_ray=nsamp,
                 bracket=(H, zlo[H], z[H], glo[H], ghi[H]))
    return depth, rec, status, stats


def _sampler(dist, shape, origin, step):
    return lambda x: dfield_ref.sample(dist, shape, origin, step, x)


def render_depth(dist, shape, origin, step, cam6, pose12, opts=None, trace=None, **kw):
    """dist: the lattice distances (dfield_ref.distance_field's or DistanceField.get()'s, x fastest).  Returns (depth [W*H], rec
    [W*H, 4], status, stats) in update()'s column-major layout."""
    o = opts if opts is not None else Opts(3, step, **kw)
    u, v, il, org, d = render_ref.rays3(cam6, pose12)
    lo, hi = box(shape, origin, step)
    t0, t1, go = render_ref.clip(org, d, lo, hi, o.tnear, o.tfar)
    return march(_sampler(dist, shape, origin, step), 3, u.shape[0], lambda idx, z: render_ref.points3(u, v, pose12, idx, z),
                 il, t0, t1, go, step, o, trace)


def render_scan(dist, shape, origin, step, thetas, pose6, off2, opts=None, trace=None, **kw):
    """Returns (range [n], rec [n, 3], status, stats)."""
    o = opts if opts is not None else Opts(2, step, **kw)
    c, s, org, d = render_ref.rays2(thetas, pose6, off2)
    lo, hi = box(shape, origin, step)
    t0, t1, go = render_ref.clip(org, d, lo, hi, o.tnear, o.tfar)
    return march(_sampler(dist, shape, origin, step), 2, c.shape[0],
                 lambda idx, r: render_ref.points2(c, s, off2, pose6, idx, r), None, t0, t1, go, step, o, trace)


__all__ = ["Opts", "box", "march", "render_depth", "render_scan"]
