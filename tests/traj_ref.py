"""numpy reference of the trajectory optimiser (csrc/traj.hip), written from the contract in float32 without FMA
and vectorised over the batch: only the iterations and the j loop of the metric are Python loops.

x is [m, N, dim] float32; x[:, 0] and x[:, N - 1] never move; n = N - 2 interior points.  `variant` selects one of the
deliberately defective forms (VARIANTS) that tests/test_traj_ref.py must tell from the reference."""
import numpy as np

import dfield_ref

F32 = np.float32
TREE = 256
VARIANTS = ("desc_j", "thomas", "fused_a", "npsum", "per_waypoint_trust", "search_lt")
OPT_NAMES = ("clearance", "margin", "w_smooth", "w_obs", "rate", "max_move", "tol", "iters", "sub")


def default_opts(dim, step):
    """The documented defaults of gpis_traj_default_opts."""
    s = F32(step)
    return dict(clearance=F32(0), margin=F32(3) * s, w_smooth=F32(1), w_obs=F32(0.25) * s, rate=F32(0.02),
                max_move=F32(0.5) * s, tol=F32(0.01) * s, iters=100, sub=3)


def _norm(v):
    """sqrtf of the squares summed left to right over the last axis."""
    sq = v[..., 0] * v[..., 0]
    for a in range(1, v.shape[-1]):
        sq = sq + v[..., a] * v[..., a]
    return np.sqrt(sq), sq


def tree_sum(v, variant=None):
    """[m, k <= 256] -> [m]: padded with 0 to 256, then for h = 128 .. 1: v[k] += v[k + h] for k < h."""
    v = np.asarray(v, F32)
    if variant == "npsum":
        return np.sum(v, axis=1, dtype=F32)
    w = np.zeros((v.shape[0], TREE), F32)
    w[:, :v.shape[1]] = v
    h = TREE // 2
    while h >= 1:
        w[:, :h] = w[:, :h] + w[:, h:2 * h]
        h //= 2
    return w[:, 0].copy()


# ---- resampling ---------------------------------------------------------------------------------------------------------------
def arc_lengths(q):
    """s [L] of one path q [L, dim]: the serial ascending sum."""
    q = np.asarray(q, F32)
    s = np.zeros(q.shape[0], F32)
    if q.shape[0] > 1:
        d, _ = _norm(q[1:] - q[:-1])
        acc = F32(0)
        for k in range(1, q.shape[0]):
            acc = F32(acc + d[k - 1])
            s[k] = acc
    return s


def resample_one(q, N, variant=None):
    q = np.asarray(q, F32)
    L, dim = q.shape
    if L == 1:
        return np.repeat(q, N, axis=0)
    s = arc_lengths(q)
    t = np.arange(N, dtype=F32) * (s[L - 1] / F32(N - 1))
    side = "left" if variant == "search_lt" else "right"
    k = np.clip(np.searchsorted(s[:L - 1], t, side=side) - 1, 0, L - 2)
    w = (t - s[k]) / (s[k + 1] - s[k])
    x = (q[k] + w[:, None] * (q[k + 1] - q[k])).astype(F32)
    x[0] = q[0]
    x[N - 1] = q[L - 1]
    return x


def resample(off, points, pstatus, N, variant=None):
    """(x [m, N, dim] f32, in_status [m] u8) from the packed paths of gpis_plan_paths: status 0 paths resampled, the others NaN
    with input status 2."""
    points = np.asarray(points, F32)
    m, dim = len(pstatus), points.shape[1]
    x = np.full((m, N, dim), np.nan, F32)
    st = np.full(m, 2, np.uint8)
    for p in range(m):
        if pstatus[p] == 0 and off[p + 1] > off[p]:
            x[p] = resample_one(points[off[p]:off[p + 1]], N, variant)
            st[p] = 0
    return x, st


def input_status(x):
    """Input status of caller-supplied waypoints: 2 where a coordinate is not finite."""
    x = np.asarray(x, F32)
    return np.where(np.isfinite(x).all(axis=(1, 2)), 0, 2).astype(np.uint8)


# ---- the optimiser ------------------------------------------------------------------------------------------------------------
def _sample(field, pts):
    """(d [..], grad [.., dim], fin [..]) at pts [.., dim]."""
    dist, shape, origin, step = field
    dim = len(shape)
    o = dfield_ref.sample(dist, shape, origin, step, pts.reshape(-1, dim)).reshape(pts.shape[:-1] + (1 + dim,))
    d, g = o[..., 0], o[..., 1:]
    return d, g, np.isfinite(d) & np.isfinite(g).all(axis=-1)


def point_terms(d, fin, clearance, margin):
    """(q, c, e) of step 1."""
    with np.errstate(all="ignore"):
        e = (d - clearance).astype(F32)
        u = (e - margin).astype(F32)
        q = np.where(e >= margin, F32(0), np.where(e >= 0, u / margin, F32(-1)))
        c = np.where(e >= margin, F32(0), np.where(e >= 0, (u * u) / (F32(2) * margin), F32(0.5) * margin - e))
    return np.where(fin, q, F32(0)).astype(F32), np.where(fin, c, F32(0)).astype(F32), e


def metric(g, variant=None):
    """delta [m, n, dim] = inverse(tridiag(-1, 2, -1)) g in the closed form of step 3."""
    m, n, dim = g.shape
    i = np.arange(1, n + 1)
    if variant == "thomas":
        # a Thomas solve of tridiag(-1, 2, -1) delta = g in float32
        cp = np.zeros(n, F32)
        dp = np.zeros_like(g)
        cp[0] = F32(-1) / F32(2)
        dp[:, 0] = g[:, 0] / F32(2)
        for k in range(1, n):
            den = F32(F32(2) + cp[k - 1])
            cp[k] = F32(-1) / den
            dp[:, k] = (g[:, k] + dp[:, k - 1]) / den
        out = np.zeros_like(g)
        out[:, n - 1] = dp[:, n - 1]
        for k in range(n - 2, -1, -1):
            out[:, k] = dp[:, k] - cp[k] * out[:, k + 1]
        return out
    acc = np.zeros((m, n, dim), F32)
    js = range(n, 0, -1) if variant == "desc_j" else range(1, n + 1)
    for j in js:
        cf = (np.minimum(i, j) * (n + 1 - np.maximum(i, j))).astype(F32)
        acc = acc + cf[None, :, None] * g[:, j - 1, None, :]
    return (acc / F32(n + 1)).astype(F32)


def evaluate(field, x, o, variant=None):
    """dict(length, smooth, obstacle, min_dist, nonfinite, collides) of trajectories x [m, N, dim]."""
    m, N, dim = x.shape
    cl, mg, sub = F32(o["clearance"]), F32(o["margin"]), int(o["sub"])
    v = (x[:, 1:] - x[:, :-1]).astype(F32)
    ln, sq = _norm(v)
    d, g, fin = _sample(field, x)
    _, c, _ = point_terms(d[:, 1:-1], fin[:, 1:-1], cl, mg)
    ds = [d]
    for s in range(1, sub + 1):
        w = F32(s) / F32(sub + 1)
        ds.append(_sample(field, (x[:, :-1] + w * v).astype(F32))[0])
    alld = np.concatenate(ds, axis=1)
    good = np.isfinite(alld)
    md = np.where(good, alld, F32(np.inf)).min(axis=1).astype(F32)
    return dict(length=tree_sum(ln, variant), smooth=tree_sum(sq, variant), obstacle=tree_sum(c, variant), min_dist=md,
                nonfinite=(~good).sum(axis=1).astype(np.int32), collides=(md < cl).astype(np.uint8))


def optimize(dist, shape, origin, step, x, in_status=None, opts=None, variant=None, trace=None):
    """The whole call on host waypoints x [m, N, dim].  Returns dict(x, status, iterations, length, smooth, obstacle, min_dist,
    nonfinite, collides).  trace: a dict that receives per-trajectory populations (hit the trust region, e == 0, e == margin,
    non-finite interior sample, inside an obstacle)."""
    x0 = np.ascontiguousarray(x, F32)
    m, N, dim = x0.shape
    n = N - 2
    o = default_opts(dim, step)
    o.update(opts or {})
    cl, mg, ws, wo = F32(o["clearance"]), F32(o["margin"]), F32(o["w_smooth"]), F32(o["w_obs"])
    rate, mm, tol = F32(o["rate"]), F32(o["max_move"]), F32(o["tol"])
    field = (np.ascontiguousarray(dist, F32).ravel(), tuple(shape), tuple(origin), F32(step))
    ist = input_status(x0) if in_status is None else np.asarray(in_status, np.uint8)
    live = ist == 0
    idx = np.flatnonzero(live)
    xs = x0[idx].copy()
    k = idx.size
    status = np.ones(k, np.uint8)
    used = np.zeros(k, np.int32)
    act = np.ones(k, bool)
    tr = dict(trust=np.zeros(k, bool), e_zero=np.zeros(k, bool), e_margin=np.zeros(k, bool), nonfinite=np.zeros(k, bool),
              inside=np.zeros(k, bool))
    with np.errstate(all="ignore"):
        for it in range(int(o["iters"])):
            if not act.any():
                break
            a_ix = np.flatnonzero(act)
            xa = xs[a_ix]
            xi, xm, xp = xa[:, 1:-1], xa[:, :-2], xa[:, 2:]
            d, gr, fin = _sample(field, xi)
            q, _, e = point_terms(d, fin, cl, mg)
            gr = np.where(fin[..., None], gr, F32(0)).astype(F32)
            if variant == "fused_a":
                aa = ((F32(2) * xi - xm) - xp).astype(F32)
            else:
                aa = ((xi - xm) + (xi - xp)).astype(F32)
            g = (ws * aa + wo * (q[..., None] * gr)).astype(F32)
            delta = metric(g, variant)
            r, _ = _norm(delta)
            R = r.max(axis=1).astype(F32)
            capped = ~(rate * R <= mm)
            kappa = np.where(capped, mm / R, rate).astype(F32)
            if variant == "per_waypoint_trust":
                kw = np.where(rate * r <= mm, rate, mm / r).astype(F32)
                xa[:, 1:-1] = xi - kw[..., None] * delta
            else:
                xa[:, 1:-1] = xi - kappa[:, None, None] * delta
            xs[a_ix] = xa
            used[a_ix] = it + 1
            stop = (kappa * R).astype(F32) < tol
            status[a_ix[stop]] = 0
            act[a_ix[stop]] = False
            tr["trust"][a_ix] |= capped
            tr["e_zero"][a_ix] |= (fin & (e == 0)).any(axis=1)
            tr["e_margin"][a_ix] |= (fin & (e == mg)).any(axis=1)
            tr["nonfinite"][a_ix] |= (~fin).any(axis=1)
            tr["inside"][a_ix] |= (fin & (e < 0)).any(axis=1)
        ev = evaluate(field, xs, o, variant)
    out = dict(x=x0.copy(), status=np.full(m, 2, np.uint8), iterations=np.zeros(m, np.int32),
               length=np.full(m, np.nan, F32), smooth=np.full(m, np.nan, F32), obstacle=np.full(m, np.nan, F32),
               min_dist=np.full(m, np.nan, F32), nonfinite=np.zeros(m, np.int32), collides=np.zeros(m, np.uint8))
    out["x"][idx] = xs
    out["status"][idx] = status
    out["iterations"][idx] = used
    for key in ("length", "smooth", "obstacle", "min_dist", "nonfinite", "collides"):
        out[key][idx] = ev[key]
    if trace is not None:
        for key, v in tr.items():
            full = np.zeros(m, bool)
            full[idx] = v
            trace[key] = full
    return out


def max_bend(x):
    """The largest |a_i| of every trajectory, in float64 (a diagnostic, not part of the contract)."""
    x = np.asarray(x, np.float64)
    a = (x[:, 1:-1] - x[:, :-2]) + (x[:, 1:-1] - x[:, 2:])
    return np.sqrt((a ** 2).sum(-1)).max(axis=1)
