"""Reference for the robot's footprint (csrc/body.h, csrc/body.hip, the BODY instantiations of csrc/mppi.hip,
traj_body_check_kernel of csrc/traj.hip, gpis_body_*): a numpy restatement of the contract, written independently
of the product (it imports nothing from gpismap_amd).  The model, the costs, the weights and the update are the sampling
controller's (tests/mppi_ref.py), the moving balls are tests/obst_ref.py's, the field sample is the distance field's
(tests/dfield_ref.py); the rollout loop is restated here with the body in the point's place.  Without a footprint every function
here is obst_ref's, and with the one-ball zero footprint it has obst_ref's bits (tests/test_body_ref.py holds it to both).

Contract (every floating-point expression is double, written left to right, nothing contracted; / and sqrt are IEEE):
- A footprint: m balls fixed to the robot, 0 <= m <= 16 (discs in 2-D, spheres in 3-D), each an offset b[dim] in the body frame
  (x forward, y left, z up) and a radius rho >= 0.
- The body rule.  A state is (p, c, s): the position p[dim] and the heading (c, s), a yaw about z in 3-D.  Ball j sits at
    w0 = p0 + (c b0 - s b1);  w1 = p1 + (s b0 + c b1);  w2 = p2 + b2
  its sample is dfield_ref.sample at ((float)w0, (float)w1, (float)w2); d_j = (double)sample - rho_j; D = the minimum over j
  ascending, from +inf, by (d_j < D ? d_j : D); jmin = the first j that attains it.  Any NaN sample (a ball off the lattice)
  makes the body off: D = NaN, jmin = -1.  The heading is used as given: callers pass unit headings.
- clearance(): a batch of states [n, dim + 2], 1 <= n <= 2^24: per state D and jmin; below = states with D < clearance; off =
  states off the lattice; least = the index of the least D among the others (the lowest on ties; -1 if every state is off).
  m = 0 is a state error (nothing to check); a non-finite state or a heading of norm 0 an argument error.
- A controller step with a footprint is obst_ref.step with the stage cost's sampled distance replaced by D at the new position
  and the new heading (the one after the step's Cayley update: the state nominal_states records): NaN -> w_off; D < clearance
  -> w_col and hits += 1; the band as before.  With a non-empty set of moving balls: sep_j = (the minimum over the set's balls
  i ascending, from +inf, of sqrt(|w_j - o_i|^2) - r_i, from the double w_j) - rho_j per body ball j ascending; Dm = their
  minimum from +inf by the same strict comparison; dyn_hits, min_sep and the nominal rollout's values keep their meaning with
  that Dm.  Everything else -- the terminal term (at the reference point p), the control cost, the weights, the update, the
  tick, shift -- is mppi_ref's.  The nominal rollout after the update uses the same rule.
- traj_clearance(): the waypoints x [m, N, dim] float32 of smoothed trajectories.  The heading at waypoint i comes from a
  horizontal chord, in double from the float32 waypoints: e = x[k + 1] - x[k] (the first two components), n2 = e0 e0 + e1 e1,
  (c, s) = (e0 / sqrt(n2), e1 / sqrt(n2)), with k the smallest index >= min(i, N - 2) and <= N - 2 with n2 > 0; if there is
  none, the largest index < min(i, N - 2) with n2 > 0; if there is none, (c, s) = (1, 0).  Then the body rule at every waypoint.
  Per trajectory: D_min, the least D by a strict comparison from +inf (ties: the smallest (i, j)), the waypoint and the ball
  where it occurs, collides = 1 if some D < clearance or some waypoint is off the lattice.  Every waypoint off: NaN, -1, -1, 1.
  A trajectory of smoothing status 2 (no result): NaN, -1, -1, 0.

The `variant` arguments build the defective variants tests/test_body_ref.py rejects; None is the contract:
  "heading_before" (the body turned by the heading from before the step), "rot_sign" (the rotation's sign flipped), "no_radius"
  (d_j = the sample), "min_first" (D and Dm start from the first ball's value instead of +inf and the body counts as off when
  that running minimum is NaN: a NaN in the first ball is never replaced, one in a later ball is never taken), "skip_off" (a
  ball off the lattice is skipped instead of making the body off), "rot_b2" (b2 scaled by c as if the rotation reached it),
  "cast_first" (the float32 cast applied to p, c, s and b before the rotation, which then runs in float32); traj_clearance()'s own is "last_x" (the last waypoint's heading taken as (1, 0))."""
import math

import numpy as np

import dfield_ref
import mppi_ref
import obst_ref
import pf_ref

F32 = np.float32
F64 = np.float64
U64 = np.uint64
MAX_M = 16
MAX_STATES = 1 << 24
VARIANTS = ("heading_before", "rot_sign", "no_radius", "min_first", "skip_off", "rot_b2", "cast_first")
TRAJ_VARIANTS = ("last_x",)


def make(dim, offset, radius, check=True):
    """A footprint: dict(dim, m, b [m, dim], rho [m]).  ValueError for what gpis_body_set refuses with GPIS_ERR_ARG,
    OverflowError for GPIS_ERR_LIMIT (check=False: a case feeds the rollouts what the library would refuse)."""
    if dim not in (2, 3):
        raise ValueError("dim outside {2, 3}")
    b = np.asarray(offset, F64).reshape(-1, dim).copy()
    rho = np.asarray(radius, F64).ravel().copy()
    if b.shape[0] != rho.size:
        raise ValueError("one row per ball")
    if check:
        if rho.size > MAX_M:
            raise OverflowError("more than 16 balls")
        if not (np.isfinite(b).all() and np.isfinite(rho).all()):
            raise ValueError("a non-finite entry")
        if (rho < 0).any():
            raise ValueError("a negative radius")
    return dict(dim=dim, m=int(rho.size), b=b, rho=rho)


def point(dim):
    """The one-ball zero footprint: the point's bits."""
    return make(dim, np.zeros((1, dim)), [0.0])


def box(length, width, n):
    """n equal discs along the x axis whose union covers a length x width rectangle centred on the reference point: centres at
    -length / 2 + (j + 1 / 2) (length / n), radius hypot(width / 2, length / (2 n))."""
    off = np.zeros((int(n), 2), F64)
    off[:, 0] = -0.5 * float(length) + (np.arange(int(n), dtype=F64) + 0.5) * (float(length) / int(n))
    return make(2, off, np.full(int(n), math.hypot(0.5 * float(width), float(length) / (2.0 * int(n))), F64))


def states_from_poses(poses, dim):
    """States [n, dim + 2] of poses [t, R] (6 / 12 values each), the heading normalised as mppi_ref.start_state does."""
    P = np.asarray(poses, F64).reshape(-1, 12 if dim == 3 else 6)
    return np.stack([mppi_ref.start_state(p, dim) for p in P])


def ball_positions(body, pos, c, s, variant=None):
    """[m][dim] arrays: where the balls of `body` sit for the states (pos: dim arrays, c, s arrays)."""
    dim = body["dim"]
    out = []
    for j in range(body["m"]):
        b = [float(v) for v in body["b"][j]]
        if variant == "cast_first":
            p32, c32, s32, b32 = [a.astype(F32) for a in pos], c.astype(F32), s.astype(F32), [F32(v) for v in b]
            w = [(p32[0] + (c32 * b32[0] - s32 * b32[1])).astype(F64), (p32[1] + (s32 * b32[0] + c32 * b32[1])).astype(F64)]
            if dim == 3:
                w.append((p32[2] + b32[2]).astype(F64))
        elif variant == "rot_sign":
            w = [pos[0] + (c * b[0] + s * b[1]), pos[1] + (c * b[1] - s * b[0])]
            if dim == 3:
                w.append(pos[2] + b[2])
        else:
            w = [pos[0] + (c * b[0] - s * b[1]), pos[1] + (s * b[0] + c * b[1])]
            if dim == 3:
                w.append(pos[2] + (c * b[2] if variant == "rot_b2" else b[2]))
        out.append(w)
    return out


def body_rule(field, body, pos, c, s, variant=None, br=None):
    """(D [n] f64, jmin [n] i32) of the body rule at the states; field = (dist, shape, origin, step).  br: a dict whose
    second_ball_nearer (a ball after the first lowered D) and tie (a later ball's d equalled D) it counts."""
    dist, shape, origin, step = field
    n = pos[0].shape[0]
    W = ball_positions(body, pos, c, s, variant)
    D = np.full(n, np.inf, F64)
    jmin = np.zeros(n, np.int32)
    off = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        for j, w in enumerate(W):
            smp = dfield_ref.sample(dist, shape, origin, step, np.stack(w, axis=1).astype(F32))[:, 0].astype(F64)
            d = smp if variant == "no_radius" else smp - float(body["rho"][j])
            nan = np.isnan(d)
            if variant == "skip_off":
                d = np.where(nan, np.inf, d)
            elif variant != "min_first":
                off |= nan
            if j == 0 and variant == "min_first":
                D, jmin = d.copy(), np.zeros(n, np.int32)
                continue
            if br is not None and j > 0:
                br["second_ball_nearer"] = br.get("second_ball_nearer", 0) + int((d < D).sum())
                br["tie"] = br.get("tie", 0) + int((d == D).sum())
            lower = d < D
            D = np.where(lower, d, D)
            jmin = np.where(lower, np.int32(j), jmin)
    if variant == "skip_off":
        off = np.isinf(D) & (D > 0)
    if variant == "min_first":
        off = np.isnan(D)
    D = np.where(off, np.nan, D)
    jmin = np.where(off, np.int32(-1), jmin).astype(np.int32)
    return D, jmin


def clearance(dist, shape, origin, step, body, states, clearance=0.0, variant=None, br=None):
    """The batch query: dict(D [n] f64, ball [n] i32, below, off, least)."""
    dim = len(shape)
    S = np.asarray(states, F64).reshape(-1, dim + 2)
    if body["m"] == 0:
        raise RuntimeError("an empty footprint: nothing to check")
    if body["dim"] != dim or not (1 <= S.shape[0] <= MAX_STATES) or not math.isfinite(float(clearance)):
        raise ValueError("bad arguments")
    if not np.isfinite(S).all() or not (np.sqrt(S[:, dim] * S[:, dim] + S[:, dim + 1] * S[:, dim + 1]) > 0).all():
        raise ValueError("a non-finite state or a heading of norm 0")
    D, jm = body_rule((dist, shape, origin, step), body, [S[:, a].copy() for a in range(dim)], S[:, dim].copy(), S[:, dim + 1].copy(),
                      variant, br)
    off = np.isnan(D)
    least = -1
    if not off.all():
        lo = np.min(D[~off])
        least = int(np.flatnonzero(~off & (D == lo))[0])
    with np.errstate(invalid="ignore"):
        below = int((D < float(clearance)).sum())
    return dict(D=D, ball=jm, below=below, off=int(off.sum()), least=least)


def rollouts(dist, shape, origin, step, start, Ubar, z, o, cost=None, goal=None, variant=None, states=False, obst=None, t_now=0.0, body=None):
    """obst_ref.rollouts with the body in the point's place: the same arguments and the same dict; the counters off, col, band,
    free count the branches the body's D took, second_ball_nearer and tie are body_rule's, dyn_* are the moving balls' term's,
    dyn_rear counts the steps at which a body ball after the first lowered Dm."""
    if body is None or body["m"] == 0:
        return obst_ref.rollouts(dist, shape, origin, step, start, Ubar, z, o, cost, goal, None, states, obst, t_now)
    assert (cost is None) != (goal is None)
    dim = len(shape)
    assert body["dim"] == dim
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    m = z.shape[0]
    dt, gamma = float(o["dt"]), float(o["gamma"])
    sig, lo, hi = ([float(v) for v in o[k]] for k in ("sigma", "umin", "umax"))
    clr, mar = float(o["clearance"]), float(o["margin"])
    w_obs, w_col, w_off, w_goal = (float(o[k]) for k in ("w_obs", "w_col", "w_off", "w_goal"))
    n = 0 if obst is None else obst["n"]
    if n:
        assert obst["dim"] == dim
        oc, ov, orad = obst["c"], obst["v"], obst["r"]
        dclr, dmar, dw_obs, dw_col = (float(obst["opts"][k]) for k in obst_ref.OPT_KEYS)
        E0 = float(t_now) - obst["epoch"]
    field = (dist, shape, origin, step)
    pos = [np.full(m, float(start[a]), F64) for a in range(dim)]
    c, s = np.full(m, float(start[dim]), F64), np.full(m, float(start[dim + 1]), F64)
    J = np.zeros(m, F64)
    hits = np.zeros(m, np.int32)
    dyn_hits = np.zeros(m, np.int32)
    min_sep = np.full(m, np.inf, F64)
    d = np.zeros((m, T, U), F64)
    br = dict(off=0, col=0, band=0, free=0, clamped=0, second_ball_nearer=0, tie=0, dyn_col=0, dyn_band=0, dyn_free=0, dyn_off=0, dyn_rear=0)
    hist = [np.stack(pos + [c, s], axis=1)] if states else None
    half = 0.5 * dt
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            v = []
            for u in range(U):
                ub = float(Ubar[t, u])
                e = sig[u] * z[:, t, u]
                vu = np.minimum(np.maximum(ub + e, lo[u]), hi[u])
                br["clamped"] += int(np.count_nonzero(vu != ub + e))
                d[:, t, u] = vu - ub
                v.append(vu)
            a = half * v[U - 1]
            den = 1.0 + a * a
            cn = (1.0 - a * a) / den
            sn = (a + a) / den
            c1, s1 = c * cn - s * sn, s * cn + c * sn
            nn = np.sqrt(c1 * c1 + s1 * s1)
            c1, s1 = c1 / nn, s1 / nn
            bx = v[0] * dt
            if dim == 2:
                pos = [pos[0] + c * bx, pos[1] + s * bx]
            else:
                by = v[1] * dt
                pos = [pos[0] + (c * bx - s * by), pos[1] + (s * bx + c * by), pos[2] + v[2] * dt]
            cb, sb = (c, s) if variant == "heading_before" else (c1, s1)         # the heading that turns the body
            c, s = c1, s1
            if states:
                hist.append(np.stack(pos + [c, s], axis=1))
            dd, _ = body_rule(field, body, pos, cb, sb, variant, br)
            off = np.isnan(dd)
            col = ~off & (dd < clr)
            band = ~off & ~col & (dd < clr + mar)
            r = ((clr + mar) - dd) / mar if mar > 0.0 else np.zeros(m)
            j = np.where(off, w_off, np.where(col, w_col, np.where(band, (w_obs * r) * r, 0.0)))
            hits += col.astype(np.int32)
            br["off"] += int(off.sum()); br["col"] += int(col.sum()); br["band"] += int(band.sum())
            br["free"] += int((~off & ~col & ~band).sum())
            acc = np.zeros(m, F64)
            for u in range(U):
                if sig[u] > 0.0:
                    acc = acc + (float(Ubar[t, u]) * d[:, t, u]) / (sig[u] * sig[u])
            g = gamma * acc
            if not n:
                J = (J + j) + g
                continue
            # the moving balls' term, at the body's balls
            e = E0 + (float(t + 1) * dt)
            W = ball_positions(body, pos, cb, sb, variant)
            Dm = np.full(m, np.inf, F64)
            for jb, w in enumerate(W):
                sep = np.full(m, np.inf, F64)
                for i in range(n):
                    ob = [float(oc[i, b]) + float(ov[i, b]) * e for b in range(dim)]
                    q = w[0] - ob[0]
                    s2 = q * q
                    for b in range(1, dim):
                        q = w[b] - ob[b]
                        s2 = s2 + q * q
                    si = np.sqrt(s2) - float(orad[i])
                    sep = np.where(si < sep, si, sep)
                sj = sep if variant == "no_radius" else sep - float(body["rho"][jb])
                if jb == 0 and variant == "min_first":
                    Dm = sj
                    continue
                if jb > 0:
                    br["dyn_rear"] += int((sj < Dm).sum())
                Dm = np.where(sj < Dm, sj, Dm)
            dcol = Dm < dclr
            dband = ~dcol & (Dm < dclr + dmar)
            rr = ((dclr + dmar) - Dm) / dmar if dmar > 0.0 else np.zeros(m)
            jd = np.where(dcol, dw_col, np.where(dband, (dw_obs * rr) * rr, 0.0))
            dyn_hits += dcol.astype(np.int32)
            min_sep = np.where(Dm < min_sep, Dm, min_sep)
            br["dyn_col"] += int(dcol.sum()); br["dyn_band"] += int(dband.sum()); br["dyn_free"] += int((~dcol & ~dband).sum())
            br["dyn_off"] += int((off & (dcol | dband)).sum())
            J = ((J + j) + jd) + g
    if cost is not None:
        uu, ok = mppi_ref.lattice_coord(np.stack(pos, axis=1).astype(F32), shape, origin, step)
        idx = np.zeros(m, np.int64)
        stride = 1
        for a in range(dim):
            ua = np.where(ok, uu[a], F32(0))
            ia = np.floor((ua + F32(0.5)).astype(F32)).astype(np.int64)
            idx += np.minimum(ia, shape[a] - 1) * stride
            stride *= shape[a]
        G = np.asarray(cost, F32).ravel()[idx]
        blocked = ok & np.isinf(G)
        term = np.where(~ok, w_off, np.where(blocked, w_col, w_goal * np.where(blocked, F32(0), G).astype(F64)))
        br.update(term_off=int((~ok).sum()), term_blocked=int(blocked.sum()), term_cost=int((ok & ~blocked).sum()))
    else:
        gg = [float(v) for v in np.asarray(goal, F64).ravel()[:dim]]
        s2 = (pos[0] - gg[0]) * (pos[0] - gg[0])
        for a in range(1, dim):
            s2 = s2 + (pos[a] - gg[a]) * (pos[a] - gg[a])
        term = w_goal * np.sqrt(s2)
        br.update(term_goal=m)
    J = J + term
    out = dict(J=J, hits=hits, d=d, branches=br, dyn_hits=dyn_hits, min_sep=min_sep)
    if states:
        out["states"] = np.stack(hist, axis=1)
    return out


def roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0, body=None):
    """obst_ref.roll with the footprint: the K rollouts and the reference's own weights."""
    dim = len(shape)
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    z = mppi_ref.noise(seed, tick, np.arange(K, dtype=U64), Ubar.shape[0], U)
    r = rollouts(dist, shape, origin, step_, mppi_ref.start_state(pose, dim), Ubar, z, o, cost, goal, variant, obst=obst, t_now=t_now, body=body)
    r.update(q=mppi_ref.weights(r["J"], o["lam"]), Jmin=float(r["J"].min()), best=mppi_ref.best_index(r["J"]))
    return r


def finish(r, q, dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0, body=None):
    """obst_ref.finish with the footprint: the nominal rollout applies the body rule."""
    dim = len(shape)
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    q = np.asarray(q, U64)
    Tq, Th, S2 = pf_ref.totals(q)
    Un = mppi_ref.update(Ubar, q, r["d"], o)
    nom = rollouts(dist, shape, origin, step_, mppi_ref.start_state(pose, dim), Un, np.zeros((1, T, U), F64), o, cost, goal, variant,
                   states=True, obst=obst, t_now=t_now, body=body)
    return dict(T=Tq, Th=Th, S2=S2, neff=pf_ref.neff(Th, S2), nhit=int(np.count_nonzero(r["hits"])), U=Un, u0=Un[0].copy(),
                nominal_states=nom["states"][0], nominal_cost=float(nom["J"][0]), nominal_hits=int(nom["hits"][0]),
                ndyn=int(np.count_nonzero(r["dyn_hits"])), nominal_dyn_hits=int(nom["dyn_hits"][0]),
                nominal_min_sep=float(nom["min_sep"][0]), nominal_branches=nom["branches"])


def step(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0, body=None):
    """One controller step with a footprint: roll's and finish's dicts merged.  body None or empty: obst_ref.step."""
    if body is None or body["m"] == 0:
        return obst_ref.step(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost, goal, None, obst, t_now)
    r = roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost, goal, variant, obst, t_now, body)
    r.update(finish(r, r["q"], dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost, goal, variant, obst, t_now, body))
    return r


def chord_heading(xy, i, variant=None):
    """(c, s) of waypoint i of one trajectory's first two components xy [N, 2] (float64 copies of the float32 waypoints)."""
    N = xy.shape[0]
    if variant == "last_x" and i == N - 1:
        return 1.0, 0.0
    k0 = min(i, N - 2)
    for k in list(range(k0, N - 1)) + list(range(k0 - 1, -1, -1)):
        e0, e1 = xy[k + 1, 0] - xy[k, 0], xy[k + 1, 1] - xy[k, 1]
        n2 = e0 * e0 + e1 * e1
        if n2 > 0:
            nn = np.sqrt(n2)
            return float(e0 / nn), float(e1 / nn)
    return 1.0, 0.0


def traj_clearance(dist, shape, origin, step, body, x, status, clearance=0.0, variant=None, trace=None):
    """The footprint along smoothed trajectories x [m, N, dim] f32 of smoothing status [m]: dict(D_min [m] f64, waypoint, ball,
    collides [m] i32).  trace counts zero_chord (a waypoint whose own chord has no length), back (a heading taken from a chord
    before the waypoint), none (no chord at all)."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    if body["m"] == 0:
        raise RuntimeError("an empty footprint: nothing to check")
    if body["dim"] != dim or dim != len(shape) or not math.isfinite(float(clearance)):
        raise ValueError("bad arguments")
    out = dict(D_min=np.full(m, np.nan, F64), waypoint=np.full(m, -1, np.int32), ball=np.full(m, -1, np.int32), collides=np.zeros(m, np.int32))
    with np.errstate(invalid="ignore"):
        for r in range(m):
            if status[r] == 2:
                continue
            X = x[r].astype(F64)
            cs = np.array([chord_heading(X[:, :2], i, variant) for i in range(N)], F64)
            if trace is not None:
                for i in range(N):
                    k0 = min(i, N - 2)
                    e = X[k0 + 1, :2] - X[k0, :2]
                    if not (e[0] * e[0] + e[1] * e[1] > 0):
                        trace["zero_chord"] = trace.get("zero_chord", 0) + 1
                        fwd = any((X[k + 1, 0] - X[k, 0]) ** 2 + (X[k + 1, 1] - X[k, 1]) ** 2 > 0 for k in range(k0, N - 1))
                        bwd = any((X[k + 1, 0] - X[k, 0]) ** 2 + (X[k + 1, 1] - X[k, 1]) ** 2 > 0 for k in range(0, k0))
                        key = "fwd" if fwd else ("back" if bwd else "none")
                        trace[key] = trace.get(key, 0) + 1
            D, jm = body_rule((dist, shape, origin, step), body, [X[:, a].copy() for a in range(dim)], cs[:, 0].copy(), cs[:, 1].copy(),
                              None if variant in TRAJ_VARIANTS else variant)
            off = np.isnan(D)
            out["collides"][r] = 1 if (off.any() or (D < float(clearance)).any()) else 0
            cand = np.where(off, np.inf, D)
            if cand.min() < np.inf:
                i = int(np.flatnonzero(cand == cand.min())[0])
                out["D_min"][r], out["waypoint"][r], out["ball"][r] = D[i], i, jm[i]
            elif not off.all():
                out["D_min"][r] = np.inf
    return out


class Controller(obst_ref.Controller):
    """obst_ref.Controller whose step takes a footprint as well."""

    def step(self, dist, shape, origin, step_, pose, o, cost=None, goal=None, obst=None, t_now=0.0, body=None):
        mppi_ref.check_opts(o, self.dim)
        if not math.isfinite(float(t_now)) or (obst is not None and obst["dim"] != self.dim) or (body is not None and body["dim"] != self.dim):
            raise ValueError("a non-finite time, or a set or a footprint of another dim")
        self.tick += 1
        self.last = step(dist, shape, origin, step_, pose, self.U, self.seed, self.tick, self.K, o, cost, goal, None, obst, t_now, body)
        self.U = self.last["U"]
        return self.last["u0"], self.last


__all__ = ["make", "point", "box", "states_from_poses", "ball_positions", "body_rule", "clearance", "rollouts", "roll", "finish", "step",
           "chord_heading", "traj_clearance", "Controller", "MAX_M", "MAX_STATES", "VARIANTS", "TRAJ_VARIANTS"]
