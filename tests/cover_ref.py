"""numpy reference of the coverage mask, its frontiers and the field restricted to seen space (csrc/cover.hip),
written from the definitions.  It imports nothing from gpismap_amd.  Every result is an integer or a double computed in one fixed
order without FMA, so the device's bits are these.

Lattice: shape = (nx, ny[, nz]), index p = (k ny + j) nx + i, world point origin + (float)i * step (mesh_ref.lattice).  `seen` is a
flat uint8 / bool array over it, x fastest.  Poses: float32, pose12 = [t(3), R(9)] and pose6 = [t(2), R(4)], R column-major (the
tracker's layouts); the local point of a world point x is l = R^T (x - t): l[c] = R[dim c] d[0] + R[dim c + 1] d[1] (+ R[dim c + 2]
d[2]), d = (double)x - (double)t, left to right in double.

3-D: seen iff l.z > 0, the nearest pixel (floor(fx l.x / l.z + cx + 0.5), floor(fy l.y / l.z + cy + 0.5)) lies inside the image,
its depth d is valid (0.4 < (double)d < 4) and l.z < d - back_off.  Every pixel counts.

2-D: the valid beams (0.2 < (double)r < 30) with their host-double directions (c, s), sorted stably by the diamond pseudo-angle
q(c, s) = 1 - c / (|c| + |s|) for s >= 0, else 3 + c / (|c| + |s|); sector k runs from sorted beam k to k + 1 (the last wraps to the
first), lim = min(r_k, r_k+1) - back_off, narrow = (dq < 2) and (c_k c_k+1 + s_k s_k+1 >= cos(max_gap)).  l = R^T (x - t) - off2;
its sector: the last k with q_k <= q(l), the wrapping one if there is none.  Seen iff that sector is narrow, lim > 0 and
l.l < lim^2.  Fewer than two valid beams: nothing; l.l == 0: seen when two or more valid beams exist."""
import math

import numpy as np

import mesh_ref

F32, F64 = np.float32, np.float64


# ---- options ------------------------------------------------------------------------------------------------------------------
def default_opts(dim, step):
    if dim not in (2, 3) or not (math.isfinite(step) and step > 0):
        raise ValueError("dim / step")
    return dict(back_off=float(F32(step)), max_gap=float(F32(2.0 * (math.pi / 180.0))), clearance=float(F32(3) * F32(step)),
                min_size=8, max_rounds=0)


def check_opts(o):
    """ValueError on what gpis_cover_* refuses with GPIS_ERR_ARG."""
    b, g, c = F32(o["back_off"]), F32(o["max_gap"]), F32(o["clearance"])
    if not (np.isfinite(b) and b >= 0):
        raise ValueError("back_off")
    if not (np.isfinite(g) and g > 0 and float(g) < math.pi / 2):
        raise ValueError("max_gap")
    if not (np.isfinite(c) and c > b):
        raise ValueError("clearance <= back_off: every surface would raise a frontier")
    if o["min_size"] < 1 or o["max_rounds"] < 0:
        raise ValueError("min_size / max_rounds")


def _n3(shape):
    return (shape[2] if len(shape) == 3 else 1, shape[1], shape[0])


def _local(shape, origin, step, pose):
    """[dim] arrays of doubles: R^T (x - t) of every lattice point."""
    dim = len(shape)
    x = mesh_ref.lattice(shape, origin, [step] * dim).astype(F64)
    P = np.ascontiguousarray(pose, F32).ravel().astype(F64)
    d = [x[:, a] - P[a] for a in range(dim)]
    R = P[dim:]
    out = []
    for c in range(dim):
        v = R[dim * c] * d[0] + R[dim * c + 1] * d[1]
        if dim == 3:
            v = v + R[dim * c + 2] * d[2]
        out.append(v)
    return out


# ---- integrating a frame --------------------------------------------------------------------------------------------------------
def depth_mask(shape, origin, step, depth, cam6, pose12, back_off):
    """bool [n]: the lattice points this depth frame sees as free space."""
    fx, fy, cx, cy = (F64(F32(c)) for c in cam6[:4])
    W, H = int(cam6[4]), int(cam6[5])
    z = np.ascontiguousarray(depth, F32).ravel()
    assert z.size == W * H
    lx, ly, lz = _local(shape, origin, step, pose12)
    with np.errstate(all="ignore"):
        u = np.floor(fx * lx / lz + cx + 0.5)
        v = np.floor(fy * ly / lz + cy + 0.5)
        ok = (lz > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        k = np.where(ok, u * H + v, 0).astype(np.int64)
        d = z[k].astype(F64)
        ok &= (d > 0.4) & (d < 4.0) & (lz < d - F64(F32(back_off)))
    return ok


def pseudo_angle(c, s):
    """The diamond angle of the direction (c, s), monotone in atan2 from 0 at (1, 0) through 1, 2, 3 towards 4: one division."""
    c, s = np.asarray(c, F64), np.asarray(s, F64)
    with np.errstate(all="ignore"):
        p = c / (np.abs(c) + np.abs(s))
    return np.where(s >= 0, 1.0 - p, 3.0 + p)


def sector_table(thetas, ranges, back_off, max_gap):
    """(q [m], lim [m], narrow [m] bool) of the m valid beams sorted by pseudo-angle; sector k: beam k -> k + 1, the last wraps."""
    th = np.ascontiguousarray(thetas, F32).ravel()
    r = np.ascontiguousarray(ranges, F32).ravel().astype(F64)
    keep = np.nonzero((r > 0.2) & (r < 30.0))[0]
    c = np.array([math.cos(float(a)) for a in th[keep]], F64)
    s = np.array([math.sin(float(a)) for a in th[keep]], F64)
    q = pseudo_angle(c, s)
    order = np.argsort(q, kind="stable")
    q, c, s, r = q[order], c[order], s[order], r[keep][order]
    m = q.size
    if m == 0:
        return q, np.zeros(0), np.zeros(0, bool)
    nxt = np.roll(np.arange(m), -1)
    dq = q[nxt] - q
    dq[m - 1] = (q[0] + 4.0) - q[m - 1]
    dot = c * c[nxt] + s * s[nxt]
    lim = np.minimum(r, r[nxt]) - F64(F32(back_off))
    narrow = (dq < 2.0) & (dot >= math.cos(float(F32(max_gap))))
    return q, lim, narrow


def scan_mask(shape, origin, step, thetas, ranges, pose6, off2, back_off, max_gap):
    """bool [n]: the lattice points this scan sees as free space."""
    q, lim, narrow = sector_table(thetas, ranges, back_off, max_gap)
    lx, ly = _local(shape, origin, step, pose6)
    lx = lx - F64(F32(off2[0]))
    ly = ly - F64(F32(off2[1]))
    m = q.size
    if m < 2:
        return np.zeros(lx.size, bool)
    ll = lx * lx + ly * ly
    k = np.searchsorted(q, pseudo_angle(lx, ly), side="right") - 1
    k[k < 0] = m - 1
    k[ll == 0] = 0                                              # (q is NaN there)
    return (ll == 0) | (narrow[k] & (lim[k] > 0) & (ll < lim[k] * lim[k]))


def integrate_depth(seen, shape, origin, step, depth, cam6, pose12, back_off):
    return (np.asarray(seen).ravel() != 0) | depth_mask(shape, origin, step, depth, cam6, pose12, back_off)


def integrate_scan(seen, shape, origin, step, thetas, ranges, pose6, off2, back_off, max_gap):
    return (np.asarray(seen).ravel() != 0) | scan_mask(shape, origin, step, thetas, ranges, pose6, off2, back_off, max_gap)


# ---- frontiers ------------------------------------------------------------------------------------------------------------------
def _shift(a, o, fill):
    dx, dy, dz = o
    nz, ny, nx = a.shape
    p = np.pad(a, 1, constant_values=fill)
    return p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def frontier_flags(seen, dist, shape, clearance):
    """bool [n]: seen and traversable, with an unseen and traversable axis neighbour inside the lattice.  float32 compares."""
    n3 = _n3(shape)
    s = (np.asarray(seen).ravel() != 0).reshape(n3)
    with np.errstate(all="ignore"):
        ok = np.ascontiguousarray(dist, F32).reshape(n3) >= F32(clearance)
    a, b = s & ok, ~s & ok
    nb = np.zeros(n3, bool)
    for o in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        if o[2] == 0 or len(shape) == 3:
            nb |= _shift(b, o, False)
    return (a & nb).ravel()


def components(points, shape):
    """Labels of the compacted frontier points (ascending lattice indices) under full connectivity: the smallest lattice index of
    each point's component."""
    pts = np.asarray(points, np.int64)
    m = pts.size
    if m == 0:
        return pts.copy()
    n3 = _n3(shape)
    rank = np.full(n3, -1, np.int64)
    rank.ravel()[pts] = np.arange(m)
    src, dst = [], []
    for k in range(27):
        o = (k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1)
        if o == (0, 0, 0) or (len(shape) == 2 and o[2] != 0):
            continue
        nb = _shift(rank, o, -1).ravel()[pts]
        has = nb >= 0
        src.append(np.flatnonzero(has))
        dst.append(nb[has])
    src, dst = np.concatenate(src), np.concatenate(dst)
    lab = np.arange(m)
    while True:
        new = lab.copy()
        np.minimum.at(new, src, lab[dst])
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return pts[lab]
        lab = new


def frontiers(seen, dist, shape, origin, step, clearance, min_size=8):
    """dict: points [m] (ascending lattice indices), point_label [m], clusters (all components; count), and per cluster of at least
    min_size points, ordered by label: label, count, sums [c, 3], box [c, 6] (min ijk, max ijk), rep (lattice index), centroid
    [c, dim] (world, double), rep_point [c, dim] (float32 lattice point)."""
    dim = len(shape)
    nx, ny = shape[0], shape[1]
    pts = np.flatnonzero(frontier_flags(seen, dist, shape, clearance)).astype(np.int64)
    lab = components(pts, shape)
    ijk = np.stack([pts % nx, (pts // nx) % ny, pts // (nx * ny)], axis=1)
    labels = np.unique(lab)
    out = dict(label=[], count=[], sums=[], box=[], rep=[])
    for L in labels:
        mem = np.flatnonzero(lab == L)
        if mem.size < min_size:
            continue
        c = ijk[mem]
        sums = c.sum(axis=0)
        cen = sums.astype(F64) / F64(mem.size)
        di, dj, dk = (c[:, a].astype(F64) - cen[a] for a in range(3))
        d2 = di * di + dj * dj
        if dim == 3:
            d2 = d2 + dk * dk
        out["label"].append(L)
        out["count"].append(mem.size)
        out["sums"].append(sums)
        out["box"].append(np.concatenate([c.min(axis=0), c.max(axis=0)]))
        out["rep"].append(pts[mem[np.argmin(d2)]])              # (the first minimum: the smallest index)
    nc = len(out["label"])
    res = dict(points=pts.astype(np.int32), point_label=lab.astype(np.int32), clusters=int(labels.size),
               label=np.array(out["label"], np.int32), count=np.array(out["count"], np.int32),
               sums=np.array(out["sums"], np.int64).reshape(nc, 3), box=np.array(out["box"], np.int32).reshape(nc, 6),
               rep=np.array(out["rep"], np.int32))
    o64 = np.array([F64(F32(v)) for v in origin])
    with np.errstate(all="ignore"):
        res["centroid"] = o64 + (res["sums"][:, :dim].astype(F64) / res["count"].astype(F64)[:, None]) * F64(F32(step))
    res["rep_point"] = lattice_points(res["rep"], shape, origin, step)
    return res


def lattice_points(idx, shape, origin, step):
    """float32 [m, dim]: origin + (float)i * step of the lattice indices."""
    idx = np.asarray(idx, np.int64)
    nx, ny = shape[0], shape[1]
    ijk = [idx % nx, (idx // nx) % ny, idx // (nx * ny)]
    return np.stack([F32(origin[a]) + ijk[a].astype(F32) * F32(step) for a in range(len(shape))], axis=1).astype(F32).reshape(-1, len(shape))


# ---- the field restricted to seen space, and the exploration step ---------------------------------------------------------------
def restrict(seen, dist, unseen_dist):
    assert math.isfinite(unseen_dist)
    return np.where(np.asarray(seen).ravel() != 0, np.ascontiguousarray(dist, F32).ravel(), F32(unseen_dist)).astype(F32)


def explore(seen, dist, shape, origin, step, start, clearance, min_size=8, unseen_dist=None, **plan):
    """(path [len, dim] f32, status, clusters): the frontiers, the planner's reference on the restricted field with the cluster
    representatives as goals, the path from `start`.  Status: the planner's, or 4 without a frontier."""
    import plan_ref
    fr = frontiers(seen, dist, shape, origin, step, clearance, min_size)
    if fr["label"].size == 0:
        return np.zeros((0, len(shape)), F32), 4, fr
    rd = restrict(seen, dist, -float(F32(step)) if unseen_dist is None else unseen_dist)
    pb = plan_ref.Problem(rd, shape, origin, step, fr["rep_point"], clearance=clearance, **plan)
    cost = plan_ref.solve_dijkstra(pb)
    pol = plan_ref.policy(pb, cost)
    npts = int(np.prod(shape))
    off, pts, sc, st = plan_ref.paths(pb, cost, pol, np.asarray(start, F32).reshape(1, -1), npts)
    return pts, int(st[0]), fr
