"""Reference for the ray-marching renderer (csrc/render.hip): a vectorised numpy float32 restatement of the march
contract with the same ray layout, clip, steps, hit rule, refinement and output, written independently of the product (it imports
nothing from gpismap_amd).  The map enters only through `test_fn(points [m, dim] f32, res [m, 2(1+dim)] f32) -> res`, which
answers test() on pre-filled records (f = NaN, zeros elsewhere), and through the clip box (the cluster cells' box grown by the
search half-width, as the renderer reports it).  test()'s bits do not depend on the batch, so the order of the calls here is free.

3-D: ray k = pixel (col, row) = (k // H, k % H); u = (col - cx) / fx, v = (row - cy) / fy; parameter z; world point
R[i] (u z) + R[3+i] (v z) + R[6+i] z + t[i], left to right.  2-D: c, s = cos, sin of the beam angle in float64; local point
(f32(r c) + off0, f32(r s) + off1); world R local + t.  Arc-length steps become z steps through 1 / sqrt(u^2 + v^2 + 1)."""
import math

import numpy as np

F32 = np.float32
NAN = F32(np.nan)


class Opts:
    """The march options; None fields are resolved by the caller (far_step, level)."""

    def __init__(self, dim, **kw):
        if dim == 3:
            d = dict(tnear=0.4, tfar=4.0, min_step=1e-3, max_step=0.01, max_steps=512)
        else:
            d = dict(tnear=0.2, tfar=30.0, min_step=0.01, max_step=0.1, max_steps=1024)
        d.update(far_step=None, level=None, max_var=np.inf, refine=8)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


def rays3(cam6, pose12):
    """(u, v, inv_len, origin [3], direction [3][n]) of the W*H pixel rays, float32."""
    fx, fy, cx, cy = (F32(c) for c in cam6[:4])
    W, H = int(cam6[4]), int(cam6[5])
    k = np.arange(W * H)
    col, row = (k // H).astype(F32), (k % H).astype(F32)
    u = (col - cx) / fx
    v = (row - cy) / fy
    il = F32(1) / np.sqrt(u * u + v * v + F32(1))
    P = np.asarray(pose12, F32)
    R, t = P[3:], P[:3]
    d = [R[a] * u + R[3 + a] * v + R[6 + a] for a in range(3)]
    o = [np.full(u.shape, t[a], F32) for a in range(3)]
    return u, v, il, o, d


def rays2(thetas, pose6, off):
    """(c, s float64, origin [2], direction [2][n] float32) of the beams."""
    th = np.asarray(thetas, F32)
    c = np.array([math.cos(float(a)) for a in th], np.float64)
    s = np.array([math.sin(float(a)) for a in th], np.float64)
    P = np.asarray(pose6, F32)
    t, R = P[:2], P[2:]
    o0, o1 = F32(off[0]), F32(off[1])
    cf, sf = c.astype(F32), s.astype(F32)
    o = [np.full(th.shape, R[0] * o0 + R[2] * o1 + t[0], F32), np.full(th.shape, R[1] * o0 + R[3] * o1 + t[1], F32)]
    d = [R[0] * cf + R[2] * sf, R[1] * cf + R[3] * sf]
    return c, s, o, d


def clip(o, d, lo, hi, tnear, tfar):
    """Slab test of [tnear, tfar] against [lo, hi] (IEEE division; fmin / fmax drop NaN).  Returns (t0, t1, go)."""
    n = o[0].shape[0]
    t0 = np.full(n, F32(tnear), F32)
    t1 = np.full(n, F32(tfar), F32)
    if lo is None or np.any(np.isnan(np.asarray(lo[:len(o)], F32))):
        return t0, t1, np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(len(o)):
            ta = (F32(lo[a]) - o[a]) / d[a]
            tb = (F32(hi[a]) - o[a]) / d[a]
            t0 = np.fmax(t0, np.fmin(ta, tb))
            t1 = np.fmin(t1, np.fmax(ta, tb))
    return t0, t1, t0 <= t1


def points3(u, v, pose12, idx, z):
    P = np.asarray(pose12, F32)
    R, t = P[3:], P[:3]
    xl, yl = u[idx] * z, v[idx] * z
    return np.stack([R[a] * xl + R[3 + a] * yl + R[6 + a] * z + t[a] for a in range(3)], axis=1).astype(F32)


def points2(c, s, off, pose6, idx, r):
    P = np.asarray(pose6, F32)
    t, R = P[:2], P[2:]
    rd = r.astype(np.float64)
    xl = (rd * c[idx]).astype(F32) + F32(off[0])
    yl = (rd * s[idx]).astype(F32) + F32(off[1])
    return np.stack([R[0] * xl + R[2] * yl + t[0], R[1] * xl + R[3] * yl + t[1]], axis=1).astype(F32)


def _query(test_fn, x, nc):
    res = np.zeros((x.shape[0], nc), F32)
    res[:, 0] = NAN
    if x.shape[0] == 0:
        return res
    out = test_fn(np.ascontiguousarray(x, F32), res)
    return res if out is None else out


def march(test_fn, dim, n, point_fn, il, t0, t1, go, o):
    """The march, the refinement and the output.  point_fn(idx, param) -> world points.  Returns (depth, rec, status, stats)."""
    nc = 2 * (1 + dim)
    level, far_step = F32(o.level), F32(o.far_step)
    mn, mx, max_var = F32(o.min_step), F32(o.max_step), F32(o.max_var)
    z, zend = t0.copy(), t1.copy()
    zlo = np.zeros(n, F32); glo = np.zeros(n, F32); ghi = np.zeros(n, F32)
    has = np.zeros(n, bool); pok = np.zeros(n, bool); nstep = np.zeros(n, np.int64)
    status = np.where(go, 255, 1).astype(np.uint8)
    depth = np.full(n, NAN, F32)
    rec = np.full((n, nc), NAN, F32)
    stats = dict(passes=0, march_passes=0, samples=0)
    act = np.nonzero(go)[0]
    while act.size:
        r = _query(test_fn, point_fn(act, z[act]), nc)
        stats["passes"] += 1; stats["march_passes"] += 1; stats["samples"] += act.size
        g = r[:, 0] - level
        ok = r[:, 1 + dim] <= max_var
        with np.errstate(invalid="ignore"):
            hit = has[act] & pok[act] & ok & (g < 0) & ~(glo[act] < 0)
        ghi[act[hit]] = g[hit]
        status[act[hit]] = 0
        a, ga, oka = act[~hit], g[~hit], ok[~hit]
        zlo[a] = z[a]; glo[a] = ga; has[a] = True; pok[a] = oka
        nstep[a] += 1
        lim = nstep[a] >= o.max_steps
        status[a[lim]] = 2
        a, ga = a[~lim], ga[~lim]
        ds = np.where(np.isnan(ga), far_step, np.fmin(np.fmax(np.abs(ga), mn), mx)).astype(F32)
        zn = z[a] + (ds * il[a] if dim == 3 else ds)
        with np.errstate(invalid="ignore"):
            out = ~(zn <= zend[a])
        status[a[out]] = 1
        z[a[~out]] = zn[~out]
        act = a[~out]
    H = np.nonzero(status == 0)[0]
    if H.size:
        q = None
        for _ in range(o.refine):
            q = zlo[H] + (z[H] - zlo[H]) * F32(0.5)
            r = _query(test_fn, point_fn(H, q), nc)
            stats["passes"] += 1; stats["samples"] += H.size
            g = r[:, 0] - level
            with np.errstate(invalid="ignore"):
                ins = g < 0
            z[H[ins]] = q[ins]; ghi[H[ins]] = g[ins]
            zlo[H[~ins]] = q[~ins]; glo[H[~ins]] = g[~ins]
        a, b, ga = zlo[H], z[H], glo[H]
        with np.errstate(invalid="ignore", divide="ignore"):
            sec = np.fmin(np.fmax(a + (b - a) * (ga / (ga - ghi[H])), a), b)
        q = np.where(np.isnan(ga), b, sec).astype(F32)
        r = _query(test_fn, point_fn(H, q), nc)
        stats["passes"] += 1; stats["samples"] += H.size
        depth[H] = q
        rec[H] = r
    stats["hits"] = int(H.size)
    return depth, rec, status, stats


def render_depth(test_fn, cam6, pose12, box, opts):
    """box = (lo [3], hi [3]) as the renderer reports it (None / NaN: an empty map).  Returns (depth, rec, status, stats)."""
    u, v, il, o, d = rays3(cam6, pose12)
    lo, hi = (None, None) if box is None else box
    t0, t1, go = clip(o, d, lo, hi, opts.tnear, opts.tfar)
    n = u.shape[0]
    return march(test_fn, 3, n, lambda idx, z: points3(u, v, pose12, idx, z), il, t0, t1, go, opts)


def render_scan(test_fn, thetas, pose6, off, box, opts):
    c, s, o, d = rays2(thetas, pose6, off)
    lo, hi = (None, None) if box is None else box
    t0, t1, go = clip(o, d, lo, hi, opts.tnear, opts.tfar)
    return march(test_fn, 2, c.shape[0], lambda idx, r: points2(c, s, off, pose6, idx, r), None, t0, t1, go, opts)


__all__ = ["Opts", "rays3", "rays2", "clip", "points3", "points2", "march", "render_depth", "render_scan"]
