"""Reference for scoring batches of pose hypotheses against a distance field (csrc/locate.hip, gpis3_locate_depth_field /
gpis2_locate_scan_field): a numpy restatement of the contract, written independently of the product (it imports
nothing from gpismap_amd).  The points and the world-point expression are the tracker's (tests/track_ref.py), the sample is the
field's (tests/dfield_ref.py); what is stated here is the truncated cost, its one summation order and the ranking.

Contract:
- Points: track_ref.points3(depth, cam6, stride) / track_ref.points2(thetas, ranges, off2): the tracker's validity windows, order
  and float32 local points; p of them.
- Poses: float32 [m, 12] = [t(3), R(9)] / [m, 6] = [t(2), R(4)].  World point of point i under pose P: track_ref.world's
  expression with R, t straight from the float32 pose: R[a] x + R[3+a] y + R[6+a] z + t[a], left to right, float32, no FMA.
- Per point: d = dfield_ref.sample(...)[:, 0] (NaN outside the lattice); e = |(double)d|; inlier iff d is finite and
  e <= max_residual; q = e for an inlier, else max_residual; the term is q * q in double, the count term 1 for an inlier.
- Per pose: slot l (0 <= l < 64) adds the terms of points l, l + 64, l + 128, ... in ascending order from 0.0; the 64 slots are
  reduced by the halving tree v[k] = v[k] + v[k + h], h = 32 .. 1.  The inlier count is an integer sum.  p = 0: cost 0.0.
- Ranking: the first min(top_k, m) pose indices by cost ascending, ties by lower index (stable); top_k = 0: all m.
- Poses are independent: a pose has the same bits alone, in any batch, at any batch position.

The `variant` argument of `score` builds the defective variants tests/test_locate_ref.py rejects; None is the contract."""
import numpy as np

import dfield_ref
import track_ref

F32 = np.float32
F64 = np.float64
SLOTS = 64
CHUNK = 1 << 16          # samples per dfield_ref.sample call (cache-sized; the poses are independent)


def default_opts(dim):
    """The library's defaults (gpis_locate_default_opts)."""
    return dict(max_residual=0.05, stride=8, top_k=16) if dim == 3 else dict(max_residual=0.5, stride=1, top_k=16)


def world_points(loc, poses, dim, variant=None):
    """[m, p, dim] float32 world points of the local points under every pose."""
    P = np.asarray(poses, F32).reshape(-1, 12 if dim == 3 else 6)
    if variant == "pose64":                # the world point from a float64 pose: every product and sum in double, one rounding
        P = P.astype(F64)
        loc = loc.astype(F64)
    R, t = P[:, dim:], P[:, :dim]
    c = [loc[None, :, a] for a in range(dim)]
    if dim == 3:
        cols = [R[:, a, None] * c[0] + R[:, 3 + a, None] * c[1] + R[:, 6 + a, None] * c[2] + t[:, a, None] for a in range(3)]
    else:
        cols = [R[:, 0, None] * c[0] + R[:, 2, None] * c[1] + t[:, 0, None], R[:, 1, None] * c[0] + R[:, 3, None] * c[1] + t[:, 1, None]]
    return np.stack(cols, axis=2).astype(F32)


def terms(d, max_residual, variant=None):
    """(term float64, inlier bool) of the sampled values d (any shape)."""
    e = np.abs(d.astype(F64))
    with np.errstate(invalid="ignore"):
        inl = np.isfinite(d) & (e <= max_residual)
    if variant == "min_after_square32":    # min(e, max_residual) applied after squaring, in float32
        with np.errstate(invalid="ignore", over="ignore"):
            sq = (d * d).astype(F32)
            cap = F32(max_residual) * F32(max_residual)
            return np.where(np.isfinite(d) & (sq <= cap), sq, cap).astype(F64), inl
    q = np.where(inl, e, max_residual)
    T = q * q
    if variant == "outliers_zero":         # non-inliers contributing 0
        T = np.where(inl, T, 0.0)
    return T, inl


def reduce_pose_terms(T, variant=None):
    """[m] float64: the contract's sum of the terms T [m, p] of every pose."""
    m, p = T.shape
    if variant == "np_sum":
        return np.sum(T, axis=1)
    slots = 256 if variant == "tree256" else SLOTS
    rounds = (p + slots - 1) // slots
    pad = np.zeros((m, rounds * slots))
    pad[:, :p] = T
    rows = pad.reshape(m, rounds, slots)
    acc = np.zeros((m, slots))
    for j in (range(rounds - 1, -1, -1) if variant == "descending" else range(rounds)):
        acc = acc + rows[:, j, :]
    return track_ref.halving(np.ascontiguousarray(acc.T))


def rank(cost, top_k):
    m = cost.shape[0]
    k = m if top_k == 0 else min(int(top_k), m)
    return np.argsort(cost, kind="stable")[:k].astype(np.int32)


def score(dist, shape, origin, step, loc, poses, max_residual, top_k=0, variant=None):
    """(cost [m] f64, inliers [m] i32, order) of the poses from the local points loc [p, dim] f32."""
    dim = len(shape)
    poses = np.asarray(poses, F32).reshape(-1, 12 if dim == 3 else 6)
    m, p = poses.shape[0], loc.shape[0]
    cost = np.zeros(m, F64)
    inliers = np.zeros(m, np.int32)
    if p > 0:
        per = max(1, CHUNK // p)
        for a in range(0, m, per):
            x = world_points(loc, poses[a:a + per], dim, variant)
            d = dfield_ref.sample(dist, shape, origin, step, x.reshape(-1, dim))[:, 0].reshape(x.shape[0], p)
            T, inl = terms(d, float(max_residual), variant)
            cost[a:a + per] = reduce_pose_terms(T, variant)
            inliers[a:a + per] = inl.sum(axis=1)
    return cost, inliers, rank(cost, top_k)


def score_depth(dist, shape, origin, step, depth, cam6, poses, max_residual=0.05, stride=8, top_k=16, variant=None):
    loc, _ = track_ref.points3(depth, cam6, stride)
    return score(dist, shape, origin, step, loc, poses, max_residual, top_k, variant)


def score_scan(dist, shape, origin, step, thetas, ranges, poses, off2, max_residual=0.5, stride=1, top_k=16, variant=None):
    loc, _ = track_ref.points2(thetas, ranges, off2)
    return score(dist, shape, origin, step, loc, poses, max_residual, top_k, variant)


# ---- pose grids -----------------------------------------------------------------------------------------------------------
def pose_grid2(xs, ys, thetas):
    """[m, 6] float32, the angle the slowest axis, then y, then x; cos and sin in float64, cast."""
    xs, ys, th = (np.asarray(v, F64).ravel() for v in (xs, ys, thetas))
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    c, s = np.cos(T), np.sin(T)
    return np.stack([X, Y, c, s, -s, c], axis=-1).reshape(-1, 6).astype(F32)


def exp_so3(w):
    w = np.asarray(w, F64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def pose_grid3(pose12, offsets, rotvecs):
    """[a b, 12] float32: Exp(rotvec) R and t + offset in float64, cast; rotvec the slowest axis."""
    P = np.asarray(pose12, F64).ravel()
    t, R = P[:3], P[3:].reshape(3, 3).T
    off = np.asarray(offsets, F64).reshape(-1, 3)
    out = []
    for w in np.asarray(rotvecs, F64).reshape(-1, 3):
        Rw = exp_so3(w) @ R
        out.append(np.concatenate([t[None, :] + off, np.tile(Rw.T.ravel(), (off.shape[0], 1))], axis=1))
    return np.concatenate(out, axis=0).astype(F32)


# ---- locate and refine ----------------------------------------------------------------------------------------------------
def locate(dist, shape, origin, step, loc, poses, track_fn, refine=8, max_residual=0.5, top_k=16):
    """Score the batch, run track_fn(pose0) -> track_ref result from each of the first `refine` ranked poses, score the refined
    poses with the same options and return the one of the lowest cost (ties: the better first rank).  (pose f32, info)."""
    dim = len(shape)
    poses = np.asarray(poses, F32).reshape(-1, 12 if dim == 3 else 6)
    cost, inliers, order = score(dist, shape, origin, step, loc, poses, max_residual, top_k)
    info = dict(cost=cost, inliers=inliers, order=order, candidates=order[:max(0, int(refine))], tracks=[], refined=None,
                refined_cost=None, refined_inliers=None, best=0)
    if refine <= 0:
        return poses[order[0]].copy(), info
    info["tracks"] = [track_fn(poses[i]) for i in info["candidates"]]
    refined = np.stack([t["pose"] for t in info["tracks"]]).astype(F32)
    c2, n2, _ = score(dist, shape, origin, step, loc, refined, max_residual, top_k)
    best = int(np.argmin(c2))
    info.update(refined=refined, refined_cost=c2, refined_inliers=n2, best=best)
    return refined[best].copy(), info


__all__ = ["default_opts", "world_points", "terms", "reduce_pose_terms", "rank", "score", "score_depth", "score_scan", "pose_grid2",
           "pose_grid3", "exp_so3", "locate"]
