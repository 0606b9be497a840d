"""Reference for the footprint in the moving-obstacle check and in re-timing (csrc/traj.hip's traj_body_time_check_kernel,
traj_body_retime_kernel and traj_body_states_kernel, gpis_timed_body_*): a numpy restatement of the contract, written independently of the product (it imports nothing from gpismap_amd).
It composes the references it extends: the timed position is timing_ref.position, the chord rule body_ref.chord_heading, the
body rule's ball positions body_ref.ball_positions, the dynamic programme's own slots, walk and schedule readers retime_ref's;
the separation of an interval is obst_ref.check's expression, restated here for a body ball (tests/test_body_time_ref.py holds
every function to obst_ref.check, retime_ref.solve and retime_ref.check bit for bit on the one-ball zero footprint).

Contract.  Every floating-point expression is double, written left to right, nothing contracted; / and sqrt are IEEE.
- The timed pose.  For a trajectory of timing status 0 and tau >= 0: p(tau) = timing_ref.position; i(tau) = the segment index
  that position's bisection ends on (the largest i <= N - 2 with t_i <= tau), N - 1 for tau >= t[N-1]; (c, s)(tau) =
  body_ref.chord_heading at waypoint i(tau): the horizontal chord, searched forward from min(i, N - 2), then backward, (1, 0)
  with no usable chord.  The body holds its segment's heading; it turns at knots.
- Ball positions.  w_j(tau) = the body rule's position of ball j at (p, c, s)(tau): w0 = p0 + (c b0 - s b1), w1 = p1 + (s b0 +
  c b1), w2 = p2 + b2, in double with no float32 cast.  No field is sampled.
- The separation of one interval.  Poses at tau_k and tau_{k+1}, body ball j, moving ball i: obst_ref.check's expression with
  p_k := w_j(tau_k) and p_{k+1} - p_k := w_j(tau_{k+1}) - w_j(tau_k); sep = (sqrt(s2) - r_i) - rho_j.  Between two samples a
  body ball's centre moves on the chord of its arc.  With the one-ball zero footprint every output has the point call's bits.
- check(): obst_ref.check with that separation over k, i, j ascending: the least sep by a strict comparison from +inf (ties: the
  smallest (k, i, j)), min_ball = j, first_hit = the least k with some sep < clearance; a NaN sep is not below the clearance.
  n = 0 and untimed rows: the point call's answers with min_ball = -1.
- solve(): retime_ref.solve's dynamic programme with pause_free[a][p] iff no (i, j) has sep < clearance with the pose of own slot
  a held (every ball's displacement 0) and play_free[a][p] iff none has going from the pose of own slot a to that of a + 1, both
  at real slot a + p.  Everything else is retime_ref.solve's; the dict gains body = the number of body balls.
- sched_check(): retime_ref.check with the pose of own(k) at real slot k.  The certificate: with the solve's set, footprint and
  clearance and steps <= arrive a schedule of status 0 or 1 has collides = 0 and min_sep >= clearance.
- states(): the timed poses [m, steps + 1, dim + 2] = (p, c, s) at t0 + k dt, or along a schedule at own(k) with dt = the slot;
  NaN for rows without a timing or a schedule.

The `variant` arguments build the defective variants tests/test_body_time_ref.py rejects; None is the contract:
  "heading_next" (the heading of segment i + 1), "no_rho" (rho_j not subtracted), "play_hold" (the play cell with the heading of
  own slot a at both ends), "pause_sample" (the pause cell at its first sample only: s = 0)."""
import math

import numpy as np

import body_ref
import obst_ref
import retime_ref
import timing_ref

F32 = np.float32
F64 = np.float64
VARIANTS = ("heading_next", "no_rho", "play_hold", "pause_sample")
CHECK_KEYS = ("min_sep", "min_time", "min_obstacle", "min_ball", "first_hit", "collides")


def _count(trace, key, n=1):
    if trace is not None:
        trace[key] = trace.get(key, 0) + n


def segment(ts, tau):
    """i(tau): the index timing_ref.position's bisection ends on; N - 1 from the duration on."""
    N = ts.shape[0]
    if tau >= ts[N - 1]:
        return N - 1
    lo, hi = 0, N - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if ts[mid] <= tau:
            lo = mid
        else:
            hi = mid - 1
    return lo


def pose(xs, vs, ts, tau, variant=None, trace=None):
    """(p [dim], i, c, s) of one trajectory (float64 arrays xs [N, dim], vs, ts [N]) at tau.  trace counts past (tau from the
    duration on), on_knot (tau on a knot after the first), and where the chord came from: chord_own, chord_fwd, chord_back,
    chord_none."""
    N = ts.shape[0]
    p = timing_ref.position(xs, vs, ts, tau)
    i = segment(ts, tau)
    if trace is not None:
        _count(trace, "past" if i == N - 1 else "inside")
        if i < N - 1 and i > 0 and ts[i] == tau:
            _count(trace, "on_knot")
    if variant == "heading_next":
        i = min(i + 1, N - 1)
    c, s = body_ref.chord_heading(xs[:, :2], i)
    if trace is not None:
        n2 = lambda k: (xs[k + 1, 0] - xs[k, 0]) * (xs[k + 1, 0] - xs[k, 0]) + (xs[k + 1, 1] - xs[k, 1]) * (xs[k + 1, 1] - xs[k, 1])
        k0 = min(i, N - 2)
        if n2(k0) > 0:
            _count(trace, "chord_own")
        elif any(n2(k) > 0 for k in range(k0, N - 1)):
            _count(trace, "chord_fwd")
        elif any(n2(k) > 0 for k in range(k0)):
            _count(trace, "chord_back")
        else:
            _count(trace, "chord_none")
    return p, i, F64(c), F64(s)


def poses(xs, vs, ts, taus, variant=None, trace=None):
    """[len(taus), dim + 2] f64: the timed poses at the given times (equal times are evaluated once)."""
    memo, out = {}, []
    for tau in taus:
        key = float(tau)
        if key not in memo:
            p, _, c, s = pose(xs, vs, ts, tau, variant, trace)
            memo[key] = np.concatenate([p, [c, s]])
        out.append(memo[key])
    return np.stack(out)


def ball_tracks(body, Q):
    """W [K, m_body, dim]: where the body's balls sit at the poses Q [K, dim + 2] (body_ref.ball_positions, in double)."""
    dim = body["dim"]
    W = body_ref.ball_positions(body, [Q[:, a].copy() for a in range(dim)], Q[:, dim].copy(), Q[:, dim + 1].copy())
    return np.stack([np.stack(w, axis=1) for w in W], axis=1)


def seps(W0, dW, e0, e1, S, body, sample_only=False, variant=None):
    """(sep, s) [K, n, m_body]: obst_ref.check's expression for the intervals that start with the body's balls at W0
    [K, m_body, dim] and move them by dW while the balls of S go from their places at the elapsed times e0 [K] to those at e1."""
    dim = W0.shape[2]
    o0 = S["c"][None, :, :] + S["v"][None, :, :] * e0[:, None, None]                            # [K, n, dim]
    o1 = S["c"][None, :, :] + S["v"][None, :, :] * e1[:, None, None]
    A = W0[:, None, :, :] - o0[:, :, None, :]                                                   # [K, n, mb, dim]
    B = dW[:, None, :, :] - (o1 - o0)[:, :, None, :]
    bb, ab = B[..., 0] * B[..., 0], A[..., 0] * B[..., 0]
    for a in range(1, dim):
        bb = bb + B[..., a] * B[..., a]
        ab = ab + A[..., a] * B[..., a]
    xx = (-ab) / np.where(bb > 0, bb, F64(1.0))
    s = np.where(xx > 0, xx, F64(0.0))
    s = np.where(s < 1, s, F64(1.0))
    s = np.where(bb > 0, s, F64(0.0))
    if sample_only:
        s = np.zeros_like(s)
    q = A[..., 0] + s * B[..., 0]
    s2 = q * q
    for a in range(1, dim):
        q = A[..., a] + s * B[..., a]
        s2 = s2 + q * q
    sep = np.sqrt(s2) - S["r"][None, :, None]
    if variant != "no_rho":
        sep = sep - body["rho"][None, None, :]
    return sep, s


def _check_args(S, body, dim):
    if body is None or body["m"] == 0:
        raise ValueError("no footprint, or an empty one")
    if body["dim"] != dim:
        raise ValueError("a footprint of another dim")
    if S["dim"] != dim:
        raise ValueError("a set of another dim")


def _blank(m):
    return dict(min_sep=np.full(m, np.nan, F64), min_time=np.full(m, np.nan, F64), min_obstacle=np.full(m, -1, np.int32),
                min_ball=np.full(m, -1, np.int32), first_hit=np.full(m, -1, np.int32), collides=np.zeros(m, np.int32))


def _reduce(out, r, sep, s, tau, dt, clearance, trace=None):
    """The row's five outputs and min_ball from sep, s [steps, n, mb] (k, i, j ascending is the flat order)."""
    n, mb = sep.shape[1], sep.shape[2]
    flat = np.where(np.isnan(sep), np.inf, sep).ravel()
    if flat.min() < np.inf:
        idx = int(np.flatnonzero(flat == flat.min())[0])
        bk, bi, bj = idx // (n * mb), (idx // mb) % n, idx % mb
        out["min_sep"][r] = flat[idx]
        out["min_time"][r] = tau[bk] + s[bk, bi, bj] * dt
        out["min_obstacle"][r], out["min_ball"][r] = bi, bj
        _count(trace, "rear" if bj > 0 else "front")
    hit = np.flatnonzero((sep < clearance).any(axis=(1, 2)))
    if hit.size:
        out["first_hit"][r], out["collides"][r] = int(hit[0]), 1
        _count(trace, "hit")
    _count(trace, "nan", int(np.isnan(sep).sum()))


def check(x, v, t, tstatus, S, body, dt, steps, t0=0.0, t_begin=0.0, clearance=None, variant=None, trace=None):
    """obst_ref.check with the footprint `body` (body_ref.make): its dict plus min_ball [m] i32."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    steps = int(steps)
    clearance = S["opts"]["clearance"] if clearance is None else clearance
    args = (dt, t0, t_begin, clearance)
    if not (all(math.isfinite(float(a)) for a in args) and 1 <= steps <= 4096 and dt > 0 and t0 >= 0 and clearance >= 0):
        raise ValueError("bad arguments")
    _check_args(S, body, dim)
    dt, t0, clearance = F64(dt), F64(t0), F64(clearance)
    TB = F64(t_begin) - F64(S["epoch"])
    out = _blank(m)
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0:
                _count(trace, "untimed")
                continue
            out["min_sep"][r] = np.inf
            if S["n"] == 0:
                _count(trace, "n0")
                continue
            xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
            tau = [t0 + F64(k) * dt for k in range(steps + 1)]
            W = ball_tracks(body, poses(xs, vs, ts, tau, variant, trace))
            e = np.array([TB + tk for tk in tau], F64)
            sep, s = seps(W[:-1], W[1:] - W[:-1], e[:-1], e[1:], S, body, variant=variant)
            _reduce(out, r, sep, s, tau, dt, clearance, trace)
    return out


def tables(Q, S, body, TB, o, variant=None, trace=None):
    """(pause_free [A + 1, P + 1], play_free [A, P + 1], reach [A + 1, P + 1]) from the poses Q [A + 1, dim + 2] of the own slots,
    every cell evaluated.  trace counts turn_block: play cells blocked whose two pause cells (a, p) and (a + 1, p) are free."""
    A, P = Q.shape[0] - 1, int(o["max_pause"])
    dim = Q.shape[1] - 2
    clr, slot = F64(o["clearance"]), F64(o["slot"])
    W = ball_tracks(body, Q)
    Wh = W
    if variant == "play_hold" and A > 0:                 # the next own slot's balls placed with this slot's heading
        Qn = Q[1:].copy()
        Qn[:, dim:] = Q[:-1, dim:]
        Wh = np.concatenate([W[:1], ball_tracks(body, Qn)])
    pause = np.zeros((A + 1, P + 1), bool)
    play = np.zeros((A, P + 1), bool)
    reach = np.zeros((A + 1, P + 1), bool)
    ps = np.arange(P + 1)
    for a in range(A + 1):
        k = a + ps
        e0, e1 = TB + k.astype(F64) * slot, TB + (k + 1).astype(F64) * slot
        W0 = np.broadcast_to(W[a], (P + 1,) + W[a].shape)
        sp, _ = seps(W0, np.zeros_like(W0), e0, e1, S, body, variant == "pause_sample", variant)
        pause[a] = ~(sp < clr).any(axis=(1, 2))
        if a < A:
            dW = np.broadcast_to(Wh[a + 1] - W[a], W0.shape)
            sq, _ = seps(W0, dW, e0, e1, S, body, variant=variant)
            play[a] = ~(sq < clr).any(axis=(1, 2))
        r = reach[a]
        if a == 0:
            r[0] = True
        else:
            r |= reach[a - 1] & play[a - 1]
        for p in range(1, P + 1):
            r[p] = r[p] or (r[p - 1] and pause[a, p - 1])
    if trace is not None and A > 0:
        _count(trace, "turn_block", int((~play & pause[:-1] & pause[1:]).sum()))
    return pause, play, reach


def solve(x, v, t, tstatus, S, body, t_begin=0.0, opts=None, variant=None, trace=None, keep=None):
    """retime_ref.solve with the footprint `body`: its dict, plus body = the number of body balls.  trace counts the statuses,
    n0, the walk's counters (retime_ref.solve's) and pose()'s and tables()' counters."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    o = dict(retime_ref.default_opts(dim, 1.0) if opts is None else opts)
    retime_ref.check_opts(o)
    if not math.isfinite(float(t_begin)):
        raise ValueError("a non-finite t_begin")
    _check_args(S, body, dim)
    TB = F64(t_begin) - F64(S["epoch"])
    out = {k: np.full(m, -1, np.int32) for k in retime_ref.RES_KEYS}
    out["own"] = np.full((m, retime_ref.OWN_LEN), -1, np.int32)
    out.update(opts=o, t_begin=float(t_begin), dim=dim, body=body["m"])
    tr = trace if trace is not None else {}
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0:
                out["status"][r] = 2
                _count(tr, "status2")
                continue
            xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
            A = retime_ref.own_slots(ts[N - 1], o["slot"])
            if A > retime_ref.MAX_OWN:
                out["status"][r] = 4
                _count(tr, "status4")
                continue
            if S["n"] == 0:
                out["status"][r], out["arrive"][r], out["pauses"][r], out["own_slots"][r] = 0, A, 0, A
                out["own"][r] = np.minimum(np.arange(retime_ref.OWN_LEN), A)
                _count(tr, "status0")
                _count(tr, "n0")
                continue
            Q = poses(xs, vs, ts, [F64(a) * F64(o["slot"]) for a in range(A + 1)], variant, tr)
            pause, play, reach = tables(Q, S, body, TB, o, variant, tr)
            if keep is not None:
                keep[r] = dict(Q=Q, pause=pause, play=play, reach=reach)
            hit = np.flatnonzero(reach[A])
            out["own_slots"][r] = A
            if hit.size == 0:
                out["status"][r] = 3
                _count(tr, "status3")
                continue
            pstar = int(hit[0])
            own, first, w = retime_ref.walk(pause, play, reach, pstar, o["press_on"])
            out["status"][r] = 1 if pstar > 0 else 0
            out["arrive"][r], out["pauses"][r], out["first_pause"][r] = A + pstar, pstar, first
            out["own"][r, :own.size] = own
            out["own"][r, own.size:] = A
            _count(tr, "status%d" % out["status"][r])
            for k in ("both", "play", "pause"):
                _count(tr, k, w[k])
    return out


def sched_poses(x, v, t, sched, r, k0, count, variant=None, trace=None):
    """The poses of own(k0 + j), j = 0 .. count - 1, of trajectory r: [count, dim + 2] f64."""
    xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
    slot = F64(sched["opts"]["slot"])
    return poses(xs, vs, ts, [F64(retime_ref.own_at(sched, r, k0 + j)) * slot for j in range(count)], variant, trace)


def sched_check(x, v, t, tstatus, sched, S, body, steps, clearance=None, variant=None, trace=None):
    """retime_ref.check with the footprint `body`: the pose of own(k) at real slot k; check()'s dict."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    steps = int(steps)
    clearance = S["opts"]["clearance"] if clearance is None else clearance
    if not (math.isfinite(float(clearance)) and 1 <= steps <= 4096 and clearance >= 0):
        raise ValueError("bad arguments")
    _check_args(S, body, dim)
    slot, clearance = F64(sched["opts"]["slot"]), F64(clearance)
    TB = F64(sched["t_begin"]) - F64(S["epoch"])
    out = _blank(m)
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0 or sched["status"][r] >= 2:
                continue
            out["min_sep"][r] = np.inf
            if S["n"] == 0:
                continue
            W = ball_tracks(body, sched_poses(x, v, t, sched, r, 0, steps + 1, variant, trace))
            tau = [F64(0.0) + F64(k) * slot for k in range(steps + 1)]
            e = np.array([TB + tk for tk in tau], F64)
            sep, s = seps(W[:-1], W[1:] - W[:-1], e[:-1], e[1:], S, body, variant=variant)
            _reduce(out, r, sep, s, tau, slot, clearance, trace)
    return out


def states(x, v, t, tstatus, dt, steps, t0=0.0, sched=None, variant=None, trace=None):
    """The timed poses [m, steps + 1, dim + 2] f64 at t0 + k dt; with a schedule at own(k) (dt and t0 are not read)."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    steps = int(steps)
    if not 1 <= steps <= 4096:
        raise ValueError("bad arguments")
    if sched is None and not (math.isfinite(float(dt)) and math.isfinite(float(t0)) and dt > 0 and t0 >= 0):
        raise ValueError("bad arguments")
    out = np.full((m, steps + 1, dim + 2), np.nan, F64)
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0 or (sched is not None and sched["status"][r] >= 2):
                continue
            if sched is not None:
                out[r] = sched_poses(x, v, t, sched, r, 0, steps + 1, variant, trace)
            else:
                xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
                out[r] = poses(xs, vs, ts, [F64(t0) + F64(k) * F64(dt) for k in range(steps + 1)], variant, trace)
    return out


__all__ = ["segment", "pose", "poses", "ball_tracks", "seps", "check", "tables", "solve", "sched_poses", "sched_check", "states",
           "VARIANTS", "CHECK_KEYS"]
