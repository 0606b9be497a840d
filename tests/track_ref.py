"""Reference for sensor tracking (csrc/track.hip): a numpy restatement of the tracking contract -- the points, the
records, the residual / Jacobian terms, the fixed reduction order, the host solve and the pose update -- written independently of
the product (it imports nothing from gpismap_amd).  The map enters only through `test_fn(points [m, dim] f32, res [m, 2(1+dim)]
f32) -> res`, which answers test() on pre-filled records (f = NaN, zeros elsewhere; None = no answer, the records stay as they
are).  test()'s bits do not depend on the batch, so one call per pass is free to stand for the device's chunks.

Contract:
- 3-D points: pixels (col, row) = (n stride, m stride), n < W // stride, m < H // stride, column-major (k = col H + row
  ascending); used iff 0.4 < (double)z < 4.  u = (col - cx) / fx, v = (row - cy) / fy in float32; local (u z, v z, z); world
  R[i] x + R[3+i] y + R[6+i] z + t[i] left to right in float32, R, t = the double pose cast to float32.
- 2-D points: beams with 0.2 < (double)r < 30 in input order; c, s = cos, sin of the float64 angle; local
  (f32(r c) + off0, f32(r s) + off1); world R local + t.
- r = f - level in float32; inlier iff f and the gradient are finite, (double)var_f <= max_var and
  |(double)r| <= max_residual; w = 1 if |r| <= huber else huber / |r| (double).
- J (double from the float32 values): 3-D [g ; (p - t) x g], 2-D [gx, gy, (px - tx) gy - (py - ty) gx].
- Terms per point (non-inliers +0): (w J_i) J_k for i <= k row by row, (w J_i) r, (w r) r, 1.
- Sum: segments of 256 consecutive points zero-padded, halving tree a[i] = a[i] + a[i + s] for s = 128 .. 1; the segment
  partials zero-padded to a power of two, the same tree.
- Step: (H + lambda diag(H)) delta = -b by the Cholesky of `solve`; pose <- (Exp(omega) R, t + v) by `apply`.
- Loop, statuses and the final pass: `track`."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
SEG = 256


class Opts:
    """The tracking options (the library's defaults); level None is resolved by the caller (-fbias of the map)."""

    def __init__(self, dim, **kw):
        if dim == 3:
            d = dict(max_residual=0.05, huber=0.01, min_inliers=100)
        else:
            d = dict(max_residual=0.5, huber=0.1, min_inliers=20)
        d.update(max_var=math.inf, damping=1e-4, eps_t=1e-5, eps_r=1e-5, level=None, stride=2, max_iters=20)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


# ---- points -------------------------------------------------------------------------------------------------------------
def points3(depth, cam6, stride):
    """(local points [m, 3] f32, pixel index [m]) of the valid samples of a depth image in update()'s column-major layout."""
    fx, fy, cx, cy = (F32(c) for c in cam6[:4])
    W, H = int(cam6[4]), int(cam6[5])
    depth = np.asarray(depth, F32).ravel()
    col = np.arange(W // stride) * stride
    row = np.arange(H // stride) * stride
    k = (col[:, None] * H + row[None, :]).ravel()
    zd = depth[k].astype(F64)
    k = k[(zd > 0.4) & (zd < 4.0)]
    z = depth[k]
    u = ((k // H).astype(F32) - cx) / fx
    v = ((k % H).astype(F32) - cy) / fy
    return np.stack([u * z, v * z, z], axis=1).astype(F32), k


def points2(thetas, ranges, off):
    """(local points [m, 2] f32, beam index [m]) of the valid beams."""
    th = np.asarray(thetas, F32).ravel()
    r = np.asarray(ranges, F32).ravel()
    rd = r.astype(F64)
    k = np.nonzero((rd > 0.2) & (rd < 30.0))[0]
    c = np.array([math.cos(float(a)) for a in th[k]], F64)
    s = np.array([math.sin(float(a)) for a in th[k]], F64)
    x = (rd[k] * c).astype(F32) + F32(off[0])
    y = (rd[k] * s).astype(F32) + F32(off[1])
    return np.stack([x, y], axis=1).astype(F32), k


def pass_pose(pose, dim):
    """(R f32, t f32) of a double pose (3-D [t(3), R(9)], 2-D [t(2), R(4)])."""
    P = np.asarray(pose, F64)
    return P[dim:].astype(F32), P[:dim].astype(F32)


def world(loc, pose, dim):
    R, t = pass_pose(pose, dim)
    if dim == 3:
        x, y, z = loc[:, 0], loc[:, 1], loc[:, 2]
        return np.stack([R[a] * x + R[3 + a] * y + R[6 + a] * z + t[a] for a in range(3)], axis=1).astype(F32)
    x, y = loc[:, 0], loc[:, 1]
    return np.stack([R[0] * x + R[2] * y + t[0], R[1] * x + R[3] * y + t[1]], axis=1).astype(F32)


def query(test_fn, x, dim):
    nc = 2 * (1 + dim)
    res = np.zeros((x.shape[0], nc), F32)
    res[:, 0] = np.nan
    if x.shape[0] == 0:
        return res
    out = test_fn(np.ascontiguousarray(x, F32), res)
    return res if out is None else out


# ---- terms and their sum --------------------------------------------------------------------------------------------------
def residual(rec, dim, o):
    """(r f32, inlier bool) of the records."""
    f = rec[:, 0]
    r = f - F32(o.level)
    with np.errstate(invalid="ignore"):
        inl = np.isfinite(f) & np.all(np.isfinite(rec[:, 1:1 + dim]), axis=1) & (rec[:, 1 + dim].astype(F64) <= o.max_var) \
            & (np.abs(r.astype(F64)) <= o.max_residual)
    return r, inl


def jacobian(x, g, t, dim):
    """J [m, 6 / 3] in double from the float32 world points x, gradients g and translation t."""
    g = g.astype(F64)
    d = x.astype(F64) - np.asarray(t, F32).astype(F64)
    if dim == 3:
        return np.stack([g[:, 0], g[:, 1], g[:, 2], d[:, 1] * g[:, 2] - d[:, 2] * g[:, 1], d[:, 2] * g[:, 0] - d[:, 0] * g[:, 2],
                         d[:, 0] * g[:, 1] - d[:, 1] * g[:, 0]], axis=1)
    return np.stack([g[:, 0], g[:, 1], d[:, 0] * g[:, 1] - d[:, 1] * g[:, 0]], axis=1)


def terms(x, rec, t, dim, o):
    """[m, NS] float64 terms: the upper triangle of w J J^T row by row, w J r, w r^2, 1 (all +0 for non-inliers)."""
    nj = 6 if dim == 3 else 3
    r, inl = residual(rec, dim, o)
    rr = r.astype(F64)
    ar = np.abs(rr)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(ar <= o.huber, 1.0, o.huber / ar)
    J = jacobian(x, rec[:, 1:1 + dim], t, dim)
    cols = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nj):
            wj = w * J[:, i]
            for k in range(i, nj):
                cols.append(wj * J[:, k])
        for i in range(nj):
            cols.append((w * J[:, i]) * rr)
        cols.append((w * rr) * rr)
    cols.append(np.ones(x.shape[0]))
    T = np.stack(cols, axis=1) if x.shape[0] else np.zeros((0, len(cols)))
    return np.where(inl[:, None], T, 0.0)


def halving(a):
    """The halving tree over axis 0 of a (its length a power of two): a[i] = a[i] + a[i + s], s = n/2 .. 1."""
    a = a.copy()
    s = a.shape[0] // 2
    while s >= 1:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


def tree_sum(T):
    """The device's reduction of the terms [m, NS]: 256-point segments, then the partials padded to a power of two."""
    m, ns = T.shape
    nseg = (m + SEG - 1) // SEG
    pad = np.zeros((nseg * SEG, ns))
    pad[:m] = T
    seg = pad.reshape(nseg, SEG, ns).transpose(1, 0, 2).copy()     # [256, nseg, ns]
    s = SEG // 2
    while s >= 1:
        seg[:s] = seg[:s] + seg[s:2 * s]
        s //= 2
    part = seg[0]                                                  # [nseg, ns]
    P = 1
    while P < nseg:
        P *= 2
    pp = np.zeros((P, ns))
    pp[:nseg] = part
    return halving(pp)


def normal_equations(S, dim):
    """(H [n, n], b [n], cost, inliers) of the sums."""
    nj = 6 if dim == 3 else 3
    H = np.zeros((nj, nj))
    c = 0
    for i in range(nj):
        for k in range(i, nj):
            H[i, k] = H[k, i] = S[c]
            c += 1
    nh = nj * (nj + 1) // 2
    return H, S[nh:nh + nj].copy(), float(S[nh + nj]), float(S[nh + nj + 1])


# ---- host step ------------------------------------------------------------------------------------------------------------
def solve(H, b, lam):
    """(H + lam diag(H)) x = -b by Cholesky in Python floats (the library's order); None on a non-positive pivot."""
    n = len(b)
    A = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    for i in range(n):
        A[i][i] = float(H[i][i]) + lam * float(H[i][i])
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * n
    for i in range(n):
        s = -float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def apply(pose, delta, dim):
    """pose (list of floats) <- (Exp(omega) R, t + v).  3-D Rodrigues; below |omega| = 1e-4 A = 1 - th^2/6, B = 1/2 - th^2/24."""
    p = [float(v) for v in pose]
    if dim == 3:
        w0, w1, w2 = delta[3], delta[4], delta[5]
        th2 = w0 * w0 + w1 * w1 + w2 * w2
        th = math.sqrt(th2)
        if th < 1e-4:
            A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
        else:
            A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
        K = [[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]]
        E = [[((1.0 if r == c else 0.0) + A * K[r][c]) + B * (K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c])
              for c in range(3)] for r in range(3)]
        R = [[E[r][0] * p[3 + 3 * c] + E[r][1] * p[4 + 3 * c] + E[r][2] * p[5 + 3 * c] for c in range(3)] for r in range(3)]
        for r in range(3):
            for c in range(3):
                p[3 + 3 * c + r] = R[r][c]
        for k in range(3):
            p[k] = p[k] + delta[k]
    else:
        c, s = math.cos(delta[2]), math.sin(delta[2])
        E = [[c, -s], [s, c]]
        R = [[E[r][0] * p[2 + 2 * k] + E[r][1] * p[3 + 2 * k] for k in range(2)] for r in range(2)]
        for r in range(2):
            for k in range(2):
                p[2 + 2 * k + r] = R[r][k]
        for k in range(2):
            p[k] = p[k] + delta[k]
    return p


# ---- the call -------------------------------------------------------------------------------------------------------------
def track(test_fn, dim, loc, pix, npix, pose0, o):
    """The whole call from the local points.  Returns a dict: pose (f32, the returned pose), status, iterations, passes, points,
    inliers, cost0, cost, H, b, resid [npix] f32, pose64 (the double pose)."""
    nj = 6 if dim == 3 else 3
    cur = [float(v) for v in np.asarray(pose0, F32).ravel()]
    prev = None
    stats = dict(passes=0)

    def run(pose):
        x = world(loc, pose, dim)
        rec = query(test_fn, x, dim)
        stats["passes"] += 1
        _, t = pass_pose(pose, dim)
        return tree_sum(terms(x, rec, t, dim, o)), rec

    S, rec = run(cur)
    cost0 = normal_equations(S, dim)[2]
    it, again = 0, False
    while True:
        H, b, _, cnt = normal_equations(S, dim)
        if cnt < o.min_inliers:
            status = 2
            if it > 0:
                cur, again = prev, True
            break
        if it >= o.max_iters:
            status = 1
            break
        delta = solve(H, b, o.damping)
        if delta is None:
            status = 3
            break
        prev = cur
        cur = apply(cur, delta, dim)
        it += 1
        nv = 0.0
        for k in range(dim):
            nv = nv + delta[k] * delta[k]
        nw = 0.0
        for k in range(dim, nj):
            nw = nw + delta[k] * delta[k]
        if math.sqrt(nv) < o.eps_t and math.sqrt(nw) < o.eps_r:
            status, again = 0, True
            break
        S, rec = run(cur)
    if again:
        S, rec = run(cur)
    H, b, cost, cnt = normal_equations(S, dim)
    r, inl = residual(rec, dim, o)
    resid = np.full(npix, np.nan, F32)
    resid[pix[inl]] = r[inl]
    return dict(pose=np.asarray(cur, F64).astype(F32), pose64=np.asarray(cur, F64), status=status, iterations=it,
                passes=stats["passes"], points=int(loc.shape[0]), inliers=cnt, cost0=cost0, cost=cost, H=H, b=b, resid=resid)


def track_depth(test_fn, depth, cam6, pose0, o):
    loc, pix = points3(depth, cam6, o.stride)
    return track(test_fn, 3, loc, pix, int(cam6[4]) * int(cam6[5]), pose0, o)


def track_scan(test_fn, thetas, ranges, pose0, off, o):
    loc, pix = points2(thetas, ranges, off)
    return track(test_fn, 2, loc, pix, np.asarray(ranges).size, pose0, o)


__all__ = ["Opts", "points3", "points2", "world", "query", "residual", "jacobian", "terms", "halving", "tree_sum",
           "normal_equations", "solve", "apply", "track", "track_depth", "track_scan"]
