"""numpy reference of the body smoother (traj_body_opt_kernel of csrc/traj.hip, gpis_smooth_*): §7i's optimiser
(tests/traj_ref.py) with the obstacle term applied at the balls of a footprint (tests/body_ref.py), written from the contract and
independent of the product.  It is vectorised over the batch and the waypoints: only the iterations, the balls and the j loop of
the metric are Python loops.

Contract.  Everything of §7i that is not named here keeps §7i's rule and bits: the ends fixed, a_i, the closed-form metric
(ascending j from 0.f), R with a NaN-keeping maximum, kappa, the update before the stop test, tol, status 0 / 1 / 2, iters = 0,
float32 without FMA.  dim 2 and 3; in 3-D the body turns about z only.  Per iteration, on the current iterate x (float32):
- Headings.  Waypoint i = 0 .. N - 1 gets (c, s) in double from the float32 waypoints by body_ref.traj_clearance's chord rule:
  e = x[k + 1] - x[k] (the first two components), n2 = e0 e0 + e1 e1, nn = sqrt(n2), (c, s) = (e0 / nn, e1 / nn), with k the
  smallest index >= k0 = min(i, N - 2) and <= N - 2 with n2 > 0; if there is none, the largest index < k0 with n2 > 0; if there
  is none, (c, s) = (1, 0).  Waypoint i owns its chord iff n2 > 0 at k0 (then k = k0); nn_i is that chord's nn.  The last
  waypoint shares chord N - 2 with waypoint N - 2.
- Balls, j ascending.  w_j = the body rule's position (body_ref.ball_positions, double); the sample is dfield_ref.sample at
  (float)w_j: (smp, grad); fin_j = smp and every component of grad finite.  d_j = (float)((double)smp - rho_j);
  e_j = d_j - clearance and q_j = §7i's q(e_j) in float32; a sample that is not fin has q_j = 0.f and grad_j = 0.f (it
  contributes a zero: unknown space is free while iterating).
- f_i = q_0 grad_0, then f_i + q_j grad_j (every component; float32).
- r_j = ((float)((-s) b0 - c b1), (float)(c b0 - s b1)) (the products and the difference in double);
  tau_i = q_0 (grad_0[0] r_0[0] + grad_0[1] r_0[1]), then tau_i + q_j (...) (float32; grad's z never enters).
- t_i = ((tau_i / (float)nn_i) * (-(float)s), (tau_i / (float)nn_i) * (float)c) if waypoint i owns its chord, else (0.f, 0.f).
- T_k = t_k for k < N - 2, T_{N-2} = t_{N-2} + t_{N-1}.
- g_i[a] = w_smooth a_i[a] + w_obs (f_i[a] + w_turn (T_{i-1}[a] - T_i[a])) for a < 2 and interior i;
  g_i[2] = w_smooth a_i[2] + w_obs f_i[2].
Evaluation on the result: length, smooth, min_dist, nonfinite, collides are §7i's (the point's, at the waypoints and the `sub`
points).  obstacle = §7i's tree over the interior waypoints of (c(e_0), then + c(e_j), j ascending) with §7i's point cost c and
e_j, fin_j as above on the result's headings.  The body result D_min, waypoint, ball, body_collides is
body_ref.traj_clearance(..., clearance = (double)clearance) on the result: the same headings, d = (double)smp - rho_j in
double, a NaN sample makes the waypoint off (it collides), ties go to the smallest (i, j), every waypoint off: NaN, -1, -1, 1;
status 2: NaN, -1, -1, 0.

Zero signs.  With body_ref.point the ball sits at p + (c 0 - s 0) = p + 0: a waypoint coordinate -0 is sampled at +0, which
can change only the sign of a zero sample, weight or gradient; r_j = (+-0, +-0), so every t_i is +-0 and f_i + w_turn (+-0) is
f_i up to the sign of a zero.  g reaches x only through the metric, whose sum starts at +0.f: (+0) + (+-0) = +0 and a sum is
-0 only if both terms are, so the accumulator is never -0 and no sign of a zero in g survives it.  x, status, iterations,
length, smooth, obstacle, min_dist therefore have traj_ref.optimize's bits for any w_turn; the contract needs no extra rule.

Resampling of pose paths: §7i's rule with w = 0 where s_{k+1} == s_k (a turn in place repeats a point; §7i's quotient would be
0 / 0 there).  The segment search skips such segments except at the path's end and in a path of length 0.  Every other path
keeps §7i's bits.

`variant` builds the defective forms tests/test_traj_body_ref.py rejects (VARIANTS); None is the contract."""
import numpy as np

import body_ref
import dfield_ref
import traj_ref

F32 = np.float32
F64 = np.float64
VARIANTS = ("tau_sign", "last_alone", "desc_balls", "nearest_only", "prev_headings", "q_double", "r_unrotated")


def default_opts(dim, step, balls):
    """(opts, w_turn): the documented defaults of gpis_smooth_body_default_opts."""
    o = traj_ref.default_opts(dim, step)
    o["w_obs"] = F32(F32(0.25) * F32(step)) / F32(max(int(balls), 1))
    return o, F32(1)


# ---- resampling of pose paths -------------------------------------------------------------------------------------------------
def resample_one(q, N):
    """traj_ref.resample_one with w = 0 on a segment of no length."""
    q = np.asarray(q, F32)
    L, dim = q.shape
    if L == 1:
        return np.repeat(q, N, axis=0)
    s = traj_ref.arc_lengths(q)
    t = np.arange(N, dtype=F32) * (s[L - 1] / F32(N - 1))
    k = np.clip(np.searchsorted(s[:L - 1], t, side="right") - 1, 0, L - 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(s[k + 1] == s[k], F32(0), (t - s[k]) / (s[k + 1] - s[k])).astype(F32)
    x = (q[k] + w[:, None] * (q[k + 1] - q[k])).astype(F32)
    x[0] = q[0]
    x[N - 1] = q[L - 1]
    return x


def resample(off, points, pstatus, N):
    """traj_ref.resample over the packed pose paths of gpis_pplan_get_paths (the points alone) with resample_one above."""
    points = np.asarray(points, F32).reshape(-1, 2)
    m = len(pstatus)
    x = np.full((m, N, 2), np.nan, F32)
    st = np.full(m, 2, np.uint8)
    for p in range(m):
        if pstatus[p] == 0 and off[p + 1] > off[p]:
            x[p] = resample_one(points[off[p]:off[p + 1]], N)
            st[p] = 0
    return x, st


# ---- headings -----------------------------------------------------------------------------------------------------------------
def headings(x):
    """(c, s, own, nn) [m, N]: the chord rule of every waypoint of x [m, N, dim] f32, whether it owns its chord, and the
    length of the chord it took (1 where there is none)."""
    X = np.asarray(x, F32)[..., :2].astype(F64)
    m, N = X.shape[:2]
    K = N - 1
    with np.errstate(all="ignore"):
        e = X[:, 1:] - X[:, :-1]
        n2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
        pos = n2 > 0
        idx = np.arange(K)
        nxt = np.minimum.accumulate(np.where(pos, idx, K)[:, ::-1], axis=1)[:, ::-1]      # the first chord >= k with a length
        prv = np.maximum.accumulate(np.where(pos, idx, -1), axis=1)                        # the last chord <= k with one
        k0 = np.minimum(np.arange(N), N - 2)
        kf = nxt[:, k0]
        kb = np.where(k0 >= 1, prv[:, np.maximum(k0 - 1, 0)], -1)
        k = np.where(kf < K, kf, kb)
        have = k >= 0
        kk = np.where(have, k, 0)
        nn = np.sqrt(np.take_along_axis(n2, kk, axis=1))
        c = np.where(have, np.take_along_axis(e[..., 0], kk, axis=1) / nn, 1.0)
        s = np.where(have, np.take_along_axis(e[..., 1], kk, axis=1) / nn, 0.0)
    return c, s, kf == k0, np.where(have, nn, 1.0), dict(kf=kf, kb=kb, k0=k0, K=K)


def _ball_samples(field, body, x, c, s, order=None):
    """For every ball j (in `order`): (j, smp [m, N] f32, grad [m, N, dim] f32, fin)."""
    dist, shape, origin, step = field
    m, N, dim = x.shape
    X = x.astype(F64)
    W = body_ref.ball_positions(body, [X[..., a] for a in range(dim)], c, s)
    for j in (range(body["m"]) if order is None else order):
        o = dfield_ref.sample(dist, shape, origin, step, np.stack(W[j], axis=-1).astype(F32).reshape(-1, dim)).reshape(m, N, 1 + dim)
        smp, gr = o[..., 0], o[..., 1:]
        yield j, smp, gr, np.isfinite(smp) & np.isfinite(gr).all(axis=-1)


def body_gradient(field, body, x, cl, mg, w_turn, variant=None, heading_x=None, tr=None):
    """(f [m, N - 2, dim], turn [m, N - 2, 2]) of the interior waypoints of the iterate x: the force and T_{i-1} - T_i."""
    m, N, dim = x.shape
    c, s, own, nn, hk = headings(x if heading_x is None else heading_x)
    f = tau = None
    order = range(body["m"] - 1, -1, -1) if variant == "desc_balls" else None
    samples = list(_ball_samples(field, body, x, c, s, order))
    if variant == "nearest_only":
        with np.errstate(invalid="ignore"):
            dd = np.stack([np.where(np.isnan(sm), np.inf, sm.astype(F64) - float(body["rho"][j])) for j, sm, _, _ in samples])
        near = dd.argmin(axis=0)
    with np.errstate(all="ignore"):
        for n_, (j, smp, gr, fin) in enumerate(samples):
            rho, b = float(body["rho"][j]), [float(v) for v in body["b"][j]]
            d = (smp.astype(F64) - rho).astype(F32)
            if variant == "q_double":
                e64 = d.astype(F64) - float(cl)
                q = np.where(e64 >= float(mg), 0.0, np.where(e64 >= 0, (e64 - float(mg)) / float(mg), -1.0))
                q, e = np.where(fin, q, 0.0).astype(F32), e64.astype(F32)
            else:
                q, _, e = traj_ref.point_terms(d, fin, cl, mg)
            if variant == "nearest_only":
                q = np.where(near == n_, q, F32(0))
            gr = np.where(fin[..., None], gr, F32(0)).astype(F32)
            if variant == "r_unrotated":
                r0, r1 = np.full(c.shape, F32(-b[1])), np.full(c.shape, F32(b[0]))
            else:
                r0, r1 = ((-s) * b[0] - c * b[1]).astype(F32), (c * b[0] - s * b[1]).astype(F32)
            fj = (q[..., None] * gr).astype(F32)
            tj = (q * (gr[..., 0] * r0 + gr[..., 1] * r1).astype(F32)).astype(F32)
            f = fj if f is None else (f + fj).astype(F32)
            tau = tj if tau is None else (tau + tj).astype(F32)
            if tr is not None:
                tr["inside"] |= (fin & (e < 0)).any(axis=1)
                tr["e_zero"] |= (fin & (e == 0)).any(axis=1)
                tr["ball_off"] |= np.isnan(smp).any(axis=1)
                tr["nonfinite"] |= (~fin).any(axis=1)
        if variant == "tau_sign":
            tau = (-tau).astype(F32)
        u = (tau / nn.astype(F32)).astype(F32)
        t = np.stack([u * (-(s.astype(F32))), u * c.astype(F32)], axis=-1).astype(F32)
        t = np.where(own[..., None], t, F32(0)).astype(F32)
        T = t[:, :N - 1].copy()
        if variant != "last_alone":
            T[:, N - 2] = t[:, N - 2] + t[:, N - 1]
        turn = (T[:, :-1] - T[:, 1:]).astype(F32)
    if tr is not None:
        zero = ~own
        tr["zero_fwd"] |= (zero & (hk["kf"] < hk["K"])).any(axis=1)
        tr["zero_back"] |= (zero & (hk["kf"] >= hk["K"]) & (hk["kb"] >= 0)).any(axis=1)
        tr["zero_none"] |= (zero & (hk["kf"] >= hk["K"]) & (hk["kb"] < 0)).any(axis=1)
        tr["shared_last"] |= (t[:, N - 1] != 0).any(axis=1)
        tr["turn"] |= (turn != 0).any(axis=(1, 2))
    return f[:, 1:-1], turn


def evaluate_body(field, body, x, cl, mg, variant=None):
    """dict(obstacle [m] f32, D_min [m] f64, waypoint, ball, body_collides [m] i32) of trajectories x [m, N, dim]."""
    m, N, dim = x.shape
    c, s, _, _, _ = headings(x)
    D = np.full((m, N), np.inf, F64)
    jm = np.zeros((m, N), np.int32)
    off = np.zeros((m, N), bool)
    cost = None
    with np.errstate(all="ignore"):
        for j, smp, gr, fin in _ball_samples(field, body, x, c, s):
            rho = float(body["rho"][j])
            d64 = smp.astype(F64) - rho
            off |= np.isnan(d64)
            lower = d64 < D
            D = np.where(lower, d64, D)
            jm = np.where(lower, np.int32(j), jm)
            _, cj, _ = traj_ref.point_terms(d64.astype(F32), fin, cl, mg)
            cost = cj if cost is None else (cost + cj).astype(F32)
        out = dict(obstacle=traj_ref.tree_sum(cost[:, 1:-1], variant), D_min=np.full(m, np.nan, F64), waypoint=np.full(m, -1, np.int32),
                   ball=np.full(m, -1, np.int32), body_collides=np.zeros(m, np.int32))
        cand = np.where(off, np.inf, D)
        out["body_collides"][:] = (off.any(axis=1) | (cand < float(cl)).any(axis=1)).astype(np.int32)
        lo = cand.min(axis=1)
        for r in range(m):
            if lo[r] < np.inf:
                i = int(np.flatnonzero(cand[r] == lo[r])[0])
                out["D_min"][r], out["waypoint"][r], out["ball"][r] = D[r, i], i, jm[r, i]
            elif not off[r].all():
                out["D_min"][r] = np.inf
    return out


TRACE_KEYS = ("trust", "tol_stop", "inside", "e_zero", "ball_off", "nonfinite", "zero_fwd", "zero_back", "zero_none", "shared_last", "turn")


def optimize(dist, shape, origin, step, body, x, in_status=None, opts=None, w_turn=None, variant=None, trace=None):
    """The whole call on host waypoints x [m, N, dim].  Returns traj_ref.optimize's dict with `obstacle` the body's and D_min,
    waypoint, ball, body_collides added.  trace: a dict that receives per-trajectory populations (TRACE_KEYS)."""
    x0 = np.ascontiguousarray(x, F32)
    m, N, dim = x0.shape
    if body["m"] == 0 or body["dim"] != dim or dim != len(shape):
        raise ValueError("an empty footprint or one of another dim")
    o, wt = default_opts(dim, step, body["m"])
    o.update(opts or {})
    wt = F32(wt if w_turn is None else w_turn)
    if not (np.isfinite(wt) and wt >= 0):
        raise ValueError("w_turn negative or not finite")
    cl, mg, ws, wo = F32(o["clearance"]), F32(o["margin"]), F32(o["w_smooth"]), F32(o["w_obs"])
    rate, mm, tol = F32(o["rate"]), F32(o["max_move"]), F32(o["tol"])
    field = (np.ascontiguousarray(dist, F32).ravel(), tuple(shape), tuple(origin), F32(step))
    ist = traj_ref.input_status(x0) if in_status is None else np.asarray(in_status, np.uint8)
    idx = np.flatnonzero(ist == 0)
    xs = x0[idx].copy()
    k = idx.size
    status = np.ones(k, np.uint8)
    used = np.zeros(k, np.int32)
    act = np.ones(k, bool)
    tr = {key: np.zeros(k, bool) for key in TRACE_KEYS}
    prev = xs.copy()
    with np.errstate(all="ignore"):
        for it in range(int(o["iters"])):
            if not act.any():
                break
            a_ix = np.flatnonzero(act)
            xa = xs[a_ix]
            xi, xm, xp = xa[:, 1:-1], xa[:, :-2], xa[:, 2:]
            sub = {key: np.zeros(a_ix.size, bool) for key in TRACE_KEYS}
            f, turn = body_gradient(field, body, xa, cl, mg, wt, variant, prev[a_ix] if variant == "prev_headings" else None, sub)
            aa = ((xi - xm) + (xi - xp)).astype(F32)
            g = np.empty_like(aa)
            g[..., :2] = ws * aa[..., :2] + wo * (f[..., :2] + wt * turn)
            if dim == 3:
                g[..., 2] = ws * aa[..., 2] + wo * f[..., 2]
            delta = traj_ref.metric(g.astype(F32))
            r, _ = traj_ref._norm(delta)
            R = r.max(axis=1).astype(F32)
            capped = ~(rate * R <= mm)
            kappa = np.where(capped, mm / R, rate).astype(F32)
            prev[a_ix] = xa
            xa = xa.copy()
            xa[:, 1:-1] = xi - kappa[:, None, None] * delta
            xs[a_ix] = xa
            used[a_ix] = it + 1
            stop = (kappa * R).astype(F32) < tol
            status[a_ix[stop]] = 0
            act[a_ix[stop]] = False
            sub["trust"], sub["tol_stop"] = capped, stop
            for key in TRACE_KEYS:
                tr[key][a_ix] |= sub[key]
        ev = traj_ref.evaluate(field, xs, o) if k else None
        eb = evaluate_body(field, body, xs, cl, mg) if k else None
    out = dict(x=x0.copy(), status=np.full(m, 2, np.uint8), iterations=np.zeros(m, np.int32),
               length=np.full(m, np.nan, F32), smooth=np.full(m, np.nan, F32), obstacle=np.full(m, np.nan, F32),
               min_dist=np.full(m, np.nan, F32), nonfinite=np.zeros(m, np.int32), collides=np.zeros(m, np.uint8),
               D_min=np.full(m, np.nan, F64), waypoint=np.full(m, -1, np.int32), ball=np.full(m, -1, np.int32),
               body_collides=np.zeros(m, np.int32))
    if k:
        out["x"][idx] = xs
        out["status"][idx] = status
        out["iterations"][idx] = used
        for key in ("length", "smooth", "min_dist", "nonfinite", "collides"):
            out[key][idx] = ev[key]
        for key in ("obstacle", "D_min", "waypoint", "ball", "body_collides"):
            out[key][idx] = eb[key]
    if trace is not None:
        for key, v in tr.items():
            full = np.zeros(m, bool)
            full[idx] = v
            trace[key] = full
    return out


__all__ = ["default_opts", "resample_one", "resample", "headings", "body_gradient", "evaluate_body", "optimize", "VARIANTS", "TRACE_KEYS"]
