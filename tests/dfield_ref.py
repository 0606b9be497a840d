"""Reference for the signed Euclidean distance field (csrc/dfield.hip): a numpy restatement of the contract,
written independently of the product (it imports nothing from gpismap_amd; mesh_ref only for the lattice coordinates).

Lattice and f as mesh_ref: index p = (k ny + j) nx + i, coordinates o + float32(i) * s, one step s on every axis.  Inside iff
f < level; f NaN counts as outside.  A site is a point with a finite f that has an axis neighbour with a finite f on the other
side of the level.  The anchor of a site is the crossing of its crossed axis edges closest to it along the edge's axis (ties: the
first edge in the order -x, +x, -y, +y, -z, +z), computed as the mesh vertex of that edge: from the lower end a to the upper
end b, t = (level - f_a) / (f_b - f_a), x = a + t (b - a), float32.  Every point takes the site q* of the smallest integer
squared lattice distance (ties: the smallest linear index), found here by separable brute-force passes x, y, z.  |dist| =
sqrtf of the float32 squared distance to the anchor of q*, summed left to right; negative iff inside.  No site at all: +-inf,
site -1.

Sampling: u = (x - o) / s per axis, outside iff !(0 <= u <= n - 1) (all NaN); i0 = min(floor(u), n - 2), w = u - i0; lerps
a + w (b - a) along x, then y, then z; the gradient is the derivative of that interpolant, the x differences lerped along y
then z (y differences along z), divided by s."""
import numpy as np

import mesh_ref

F32 = np.float32
MAX_AXIS = 16384


def _coords(p, shape):
    """Integer lattice coordinates (i, j[, k]) of linear indices p (int64 arrays)."""
    out = []
    for a in range(len(shape)):
        out.append(p % shape[a])
        p = p // shape[a]
    return out


def sites(val, shape, level):
    """Boolean [n] site mask and inside mask (f < level; NaN is outside) of the f grid val (x fastest)."""
    dim = len(shape)
    V = np.asarray(val, F32).reshape(shape[::-1])
    fin = np.isfinite(V)
    with np.errstate(invalid="ignore"):
        ins = V < F32(level)
    site = np.zeros(V.shape, bool)
    for a in range(dim):
        ax = dim - 1 - a
        lo = [slice(None)] * dim
        hi = [slice(None)] * dim
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cr = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
        site[lo] |= cr
        site[hi] |= cr
    return site.ravel(), ins.ravel()


def anchors(val, shape, origin, step, level, idx):
    """Anchor coordinates [len(idx), dim] float32 of the sites idx."""
    dim = len(shape)
    v = np.asarray(val, F32).ravel()
    level = F32(level)
    ax = mesh_ref.axes(shape, origin, [step] * dim)
    idx = np.asarray(idx, np.int64)
    c = _coords(idx, shape)
    strides = [1, shape[0], shape[0] * (shape[1] if dim == 3 else 1)][:dim]
    pos = np.stack([ax[a][c[a]] for a in range(dim)], axis=1)
    out = pos.copy()
    best = np.full(idx.size, np.inf, F32)
    fp = v[idx]
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(dim):
            for sgn in (-1, 1):
                ok = (c[a] > 0) if sgn < 0 else (c[a] < shape[a] - 1)
                q = np.where(ok, idx + sgn * strides[a], idx)
                fq = v[q]
                cr = ok & np.isfinite(fp) & np.isfinite(fq) & ((fp < level) != (fq < level))
                lo = np.where(sgn < 0, q, idx)
                hi = np.where(sgn < 0, idx, q)
                fa, fb = v[lo], v[hi]
                t = (level - fa) / (fb - fa)
                xa = ax[a][np.where(sgn < 0, c[a] - 1, c[a]).clip(0, shape[a] - 1)]
                xb = ax[a][np.where(sgn < 0, c[a], c[a] + 1).clip(0, shape[a] - 1)]
                x = (xa + t * (xb - xa)).astype(F32)
                d = np.abs(x - pos[:, a]).astype(F32)
                take = cr & (d < best)
                best = np.where(take, d, best)
                out[take, a] = x[take]
                out[take, :a] = pos[take, :a]
                out[take, a + 1:] = pos[take, a + 1:]
    return out


def _d2(p, q, shape):
    """Integer squared lattice distance between index arrays p and q (q >= 0)."""
    cp, cq = _coords(p, shape), _coords(q, shape)
    return sum((cp[a] - cq[a]) ** 2 for a in range(len(shape)))


def edt_separable(site, shape, block=512):
    """Nearest site index [n] int64 (-1: none) by the passes x, y, z, each new(p) = argmin over q on p's line of
    |p - feat(q)|^2 (smallest q on ties), brute force over the line."""
    dim = len(shape)
    n = int(np.prod(shape))
    feat = np.where(np.asarray(site, bool).ravel(), np.arange(n, dtype=np.int64), -1)
    for a in range(dim):
        ax = dim - 1 - a
        F = np.moveaxis(feat.reshape(shape[::-1]), ax, -1)           # [..., n_a], a view of the line layout
        P = np.moveaxis(np.arange(n, dtype=np.int64).reshape(shape[::-1]), ax, -1)
        L = F.shape[-1]
        Fl, Pl = F.reshape(-1, L), P.reshape(-1, L)
        out = np.empty_like(Fl)
        block = max(1, min(block, (1 << 22) // (Fl.shape[0] * L)))
        for b0 in range(0, L, block):
            b1 = min(L, b0 + block)
            pp = Pl[:, b0:b1, None]                                    # [lines, B, 1]
            ff = Fl[:, None, :]                                        # [lines, 1, L]
            d = np.where(ff >= 0, _d2(pp, np.maximum(ff, 0), shape), np.iinfo(np.int64).max)
            k = np.argmin(d, axis=2)                                   # (first = smallest coordinate on ties)
            out[:, b0:b1] = np.take_along_axis(Fl, k, axis=1)
        feat = np.moveaxis(out.reshape(F.shape), -1, ax).reshape(n)
        feat = np.ascontiguousarray(feat)
    return feat


def edt_brute(site, shape):
    """The same by a brute force over all sites: smallest squared distance, then smallest index."""
    n = int(np.prod(shape))
    s = np.nonzero(np.asarray(site, bool).ravel())[0]
    if s.size == 0:
        return np.full(n, -1, np.int64)
    p = np.arange(n, dtype=np.int64)
    d = _d2(p[:, None], s[None, :], shape)
    return s[np.argmin(d, axis=1)]


def distance_field(val, shape, origin, step, level):
    """(dist [n] f32, site [n] i32) of the f grid val (x fastest), one step on every axis."""
    shape = tuple(int(v) for v in shape)
    dim = len(shape)
    assert dim in (2, 3) and max(shape) <= MAX_AXIS and min(shape) >= 2
    step = F32(step)
    site, ins = sites(val, shape, level)
    q = edt_separable(site, shape)
    n = q.size
    if not site.any():
        return np.where(ins, F32(-np.inf), F32(np.inf)).astype(F32), np.full(n, -1, np.int32)
    ax = mesh_ref.axes(shape, origin, [step] * dim)
    uq, inv = np.unique(q, return_inverse=True)
    c = anchors(val, shape, origin, step, level, uq)[inv.ravel()]
    cp = _coords(np.arange(n, dtype=np.int64), shape)
    s2 = F32(0)
    for a in range(dim):
        d = (ax[a][cp[a]] - c[:, a]).astype(F32)
        s2 = (s2 + d * d).astype(F32) if a else (d * d).astype(F32)
    dist = np.sqrt(s2).astype(F32)
    dist = np.where(ins, -dist, dist).astype(F32)
    return dist, q.astype(np.int32)


def sample(field, shape, origin, step, x):
    """[m, 1 + dim] float32: the interpolant of the lattice values field (x fastest) and its gradient at the points x."""
    shape = tuple(int(v) for v in shape)
    dim = len(shape)
    x = np.asarray(x, F32).reshape(-1, dim)
    m = x.shape[0]
    step = F32(step)
    F = np.asarray(field, F32).ravel()
    out = np.full((m, 1 + dim), np.nan, F32)
    u = [((x[:, a] - F32(origin[a])) / step).astype(F32) for a in range(dim)]
    ok = np.ones(m, bool)
    for a in range(dim):
        ok &= (u[a] >= 0) & (u[a] <= F32(shape[a] - 1))
    if not ok.any():
        return out
    i0 = [np.minimum(np.floor(u[a][ok]).astype(np.int64), shape[a] - 2) for a in range(dim)]
    w = [(u[a][ok] - i0[a].astype(F32)).astype(F32) for a in range(dim)]
    strides = [1, shape[0], shape[0] * (shape[1] if dim == 3 else 1)][:dim]
    base = sum(i0[a] * strides[a] for a in range(dim))

    def corner(dx, dy, dz=0):
        return F[base + dx + dy * strides[1] + (dz * strides[2] if dim == 3 else 0)]

    def lerp(a, b, t):
        return (a + t * (b - a)).astype(F32)

    with np.errstate(invalid="ignore", over="ignore"):
        if dim == 2:
            c00, c10, c01, c11 = corner(0, 0), corner(1, 0), corner(0, 1), corner(1, 1)
            e0, e1 = lerp(c00, c10, w[0]), lerp(c01, c11, w[0])
            val = lerp(e0, e1, w[1])
            gy = ((e1 - e0).astype(F32) / step).astype(F32)
            h0, h1 = (c10 - c00).astype(F32), (c11 - c01).astype(F32)
            gx = (lerp(h0, h1, w[1]) / step).astype(F32)
            out[ok] = np.stack([val, gx, gy], axis=1)
        else:
            c = {(dx, dy, dz): corner(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
            e = {(dy, dz): lerp(c[0, dy, dz], c[1, dy, dz], w[0]) for dy in (0, 1) for dz in (0, 1)}
            f0, f1 = lerp(e[0, 0], e[1, 0], w[1]), lerp(e[0, 1], e[1, 1], w[1])
            val = lerp(f0, f1, w[2])
            gz = ((f1 - f0).astype(F32) / step).astype(F32)
            g0, g1 = (e[1, 0] - e[0, 0]).astype(F32), (e[1, 1] - e[0, 1]).astype(F32)
            gy = (lerp(g0, g1, w[2]) / step).astype(F32)
            h = {(dy, dz): (c[1, dy, dz] - c[0, dy, dz]).astype(F32) for dy in (0, 1) for dz in (0, 1)}
            hy0, hy1 = lerp(h[0, 0], h[1, 0], w[1]), lerp(h[0, 1], h[1, 1], w[1])
            gx = (lerp(hy0, hy1, w[2]) / step).astype(F32)
            out[ok] = np.stack([val, gx, gy, gz], axis=1)
    return out


__all__ = ["sites", "anchors", "edt_separable", "edt_brute", "distance_field", "sample", "MAX_AXIS"]
