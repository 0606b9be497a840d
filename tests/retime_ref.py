"""Reference for the re-timing of timed trajectories (csrc/traj.hip's traj_retime_kernel and the schedule-reading kernels,
gpis_retime_*): a numpy restatement of the contract, written independently of the product (it imports nothing from
gpismap_amd).  The timed position is timing_ref.position; the separation of an interval from a ball is obst_ref.check's
expression, restated here for one interval; the control stage is timing_ref.controls' second stage, restated on given positions
(tests/test_retime_ref.py holds both restatements to the originals on the identity schedule).

Contract.  A batch of timed trajectories (x [m, N, dim] f32 with v, t [m, N] f32 and the timing status [m], as timing_ref.time
gives them), a set S of n balls (obst_ref.make), t_begin (the absolute time at which the schedule starts) and the options slot
(seconds, > 0), max_pause P (0 .. 255), clearance (>= 0), press_on (0 / 1).  Every floating-point expression is double, written
left to right, nothing contracted; the schedule itself is integers and flags and depends on no order.  For each trajectory of
timing status 0:
- Own time runs in slots.  A = the least integer a >= 0 with (double)a * slot >= (double)t[N-1].  pos_a = timing_ref.position(x,
  v, t, (double)a * slot), a = 0 .. A.  A > 1024: status 4.
- sep(p0, dp, k, i): obst_ref.check's sep for one interval and ball i with p_k = p0, p_{k+1} - p_k = dp, t0 = 0, dt = slot, so
  e0 = TB + (double)k * slot, e1 = TB + (double)(k + 1) * slot, TB = t_begin - epoch; o0 = c + v * e0, o1 = c + v * e1,
  a = p0 - o0, b = dp - (o1 - o0), bb = sum b b, ab = sum a b (axis order from the first product), s = 0 unless bb > 0, else
  x = (-ab) / bb limited to [0, 1] by (x > 0 ? x : 0) and (s < 1 ? s : 1), q = a + s * b, sep = sqrt(sum q q) - r_i.
- Cell (a, p): own slot a after p pauses, at real slot a + p.  pause_free[a][p] iff no ball has sep(pos_a, 0, a + p, i) <
  clearance; play_free[a][p] iff no ball has sep(pos_a, pos_{a+1} - pos_a, a + p, i) < clearance.  A NaN separation is not below
  the clearance, as in the check.
- reach[0][0] = 1; reach[a][p] = (a > 0 and reach[a-1][p] and play_free[a-1][p]) or (p > 0 and reach[a][p-1] and
  pause_free[a][p-1]).  p* = the least p <= P with reach[A][p]; none: status 3.
- The schedule: walk back from (A, p*) to (0, 0).  press_on = 0: the play predecessor wherever it is reached and free, else the
  pause predecessor (pauses fall as early as the optimum allows); press_on = 1: the pause predecessor first (as late as
  allowed).  own[a + p] = a along the walk; own(k) = A for every k > arrive = A + p*.  first_pause = the least real slot k with
  own(k + 1) = own(k) and k < arrive, -1 without a pause.
- Per trajectory: status (0 clear as timed, 1 re-timed with pauses, 2 no timing, 3 none within max_pause, 4 too long for this
  slot), arrive, pauses = p*, own_slots = A, first_pause, own [OWN_LEN].  Status 2 and 4: -1 everywhere; status 3: own_slots = A
  and -1 elsewhere.  With n = 0: status 0 and own(k) = min(k, A).
- Pauses are instantaneous: the controller's model commands velocities, the timing's a_max / d_max are not kept across a pause.
controls(): timing_ref.controls' second stage with dt = slot on the positions pos_own(k0 + k), k = 0 .. T; a schedule of status
>= 2 stands still as an untimed trajectory does.  check(): obst_ref.check's five outputs with p_k = pos_own(k), k = 0 .. steps, and
the balls at the real slots (tau_k = (double)k * slot from the schedule's t_begin); status >= 2 answers as timing status 2.

The `variant` arguments build the defective variants tests/test_retime_ref.py rejects; None is the contract:
  "pause_sample" (a pause cell tested at its first sample only: s = 0), "pause_free" (pause cells taken as free), "time_a" (the
  ball's time taken at slot a instead of a + p), "walk_swapped" (the walk's preference swapped)."""
import math

import numpy as np

import obst_ref
import timing_ref

F32 = np.float32
F64 = np.float64
MAX_OWN = 1024
MAX_PAUSE = 255
OWN_LEN = MAX_OWN + MAX_PAUSE + 1
OPT_KEYS = ("slot", "max_pause", "clearance", "press_on")
VARIANTS = ("pause_sample", "pause_free", "time_a", "walk_swapped")
RES_KEYS = ("status", "arrive", "pauses", "own_slots", "first_pause")


def default_opts(dim, step):
    """The library's defaults (gpis_retime_default_opts) for a field of lattice step `step`."""
    return dict(slot=0.1, max_pause=63, clearance=float(F32(step)), press_on=0)


def check_opts(o):
    """ValueError for what the library answers with GPIS_ERR_ARG."""
    slot, clr = float(o["slot"]), float(o["clearance"])
    if not (math.isfinite(slot) and slot > 0 and math.isfinite(clr) and clr >= 0):
        raise ValueError("slot must be positive and clearance non-negative, both finite")
    if int(o["max_pause"]) != o["max_pause"] or not 0 <= int(o["max_pause"]) <= MAX_PAUSE or o["press_on"] not in (0, 1):
        raise ValueError("max_pause outside [0, 255] or press_on outside {0, 1}")


def own_slots(duration, slot):
    """A: the least integer a >= 0 with (double)a * slot >= (double)duration; MAX_OWN + 1 stands for anything above MAX_OWN."""
    dur, slot = F64(duration), F64(slot)
    if not dur / slot <= MAX_OWN + 2:
        return MAX_OWN + 1
    a = int(dur / slot)
    while a > 0 and F64(a - 1) * slot >= dur:
        a -= 1
    while F64(a) * slot < dur:
        a += 1
    return min(a, MAX_OWN + 1)


def positions(xs, vs, ts, A, slot):
    """pos_a [A + 1, dim] of one trajectory (float64 arrays)."""
    slot = F64(slot)
    return np.stack([timing_ref.position(xs, vs, ts, F64(a) * slot) for a in range(A + 1)])


def sep(p0, dp, k, S, TB, slot, sample_only=False):
    """sep [len(k), n] of the intervals that start at p0 [dim] with the displacement dp [dim] at the real slots k (an int array)
    from every ball of S."""
    k = np.asarray(k)
    slot = F64(slot)
    e0 = TB + k.astype(F64) * slot
    e1 = TB + (k + 1).astype(F64) * slot
    o0 = S["c"][None, :, :] + S["v"][None, :, :] * e0[:, None, None]
    o1 = S["c"][None, :, :] + S["v"][None, :, :] * e1[:, None, None]
    A = p0[None, None, :] - o0
    B = dp[None, None, :] - (o1 - o0)
    dim = p0.shape[0]
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
    return np.sqrt(s2) - S["r"][None, :]


def tables(pos, S, TB, o, variant=None):
    """(pause_free [A + 1, P + 1], play_free [A, P + 1], reach [A + 1, P + 1]) of one trajectory, every cell evaluated."""
    A, P = pos.shape[0] - 1, int(o["max_pause"])
    clr = F64(o["clearance"])
    pause = np.zeros((A + 1, P + 1), bool)
    play = np.zeros((A, P + 1), bool)
    reach = np.zeros((A + 1, P + 1), bool)
    zero = np.zeros(pos.shape[1], F64)
    ps = np.arange(P + 1)
    for a in range(A + 1):
        k = ps * 0 + a if variant == "time_a" else a + ps
        if variant == "pause_free":
            pause[a] = True
        else:
            pause[a] = ~(sep(pos[a], zero, k, S, TB, o["slot"], variant == "pause_sample") < clr).any(axis=1)
        if a < A:
            play[a] = ~(sep(pos[a], pos[a + 1] - pos[a], k, S, TB, o["slot"]) < clr).any(axis=1)
        r = reach[a]
        if a == 0:
            r[0] = True
        else:
            r |= reach[a - 1] & play[a - 1]
        for p in range(1, P + 1):
            r[p] = r[p] or (r[p - 1] and pause[a, p - 1])
    return pause, play, reach


def walk(pause, play, reach, pstar, press_on, variant=None):
    """own [arrive + 1], first_pause, and the counters of the walk: cells at which both predecessors were open (`both`), play
    and pause steps, pause groups."""
    A = reach.shape[0] - 1
    prefer_pause = bool(press_on) != (variant == "walk_swapped")
    a, p = A, pstar
    own = np.zeros(A + pstar + 1, np.int32)
    own[A + pstar] = A
    first, both, nplay, npause, groups, last_was_pause = -1, 0, 0, 0, 0, False
    while a > 0 or p > 0:
        by_play = a > 0 and reach[a - 1, p] and play[a - 1, p]
        by_pause = p > 0 and reach[a, p - 1] and pause[a, p - 1]
        assert by_play or by_pause
        both += int(by_play and by_pause)
        take_pause = by_pause if prefer_pause else not by_play
        if take_pause:
            p -= 1
            first = a + p
            npause += 1
            groups += int(not last_was_pause)
        else:
            a -= 1
            nplay += 1
        last_was_pause = bool(take_pause)
        own[a + p] = a
    return own, first, dict(both=both, play=nplay, pause=npause, groups=groups)


def solve(x, v, t, tstatus, S, t_begin=0.0, opts=None, variant=None, trace=None, keep=None):
    """The schedules: dict(status, arrive, pauses, own_slots, first_pause [m] i32, own [m, OWN_LEN] i32) plus the options and
    t_begin, as check() and controls() read them.  trace counts the statuses (status0 .. status4), n0, and the walk's counters
    (`groups` is the largest number of pause groups of one schedule); keep: a dict that receives the tables of every solved
    trajectory by index."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    o = dict(default_opts(dim, 1.0) if opts is None else opts)
    check_opts(o)
    if not math.isfinite(float(t_begin)):
        raise ValueError("a non-finite t_begin")
    if S["dim"] != dim:
        raise ValueError("a set of another dim")
    P = int(o["max_pause"])
    TB = F64(t_begin) - F64(S["epoch"])
    out = {k: np.full(m, -1, np.int32) for k in RES_KEYS}
    out["own"] = np.full((m, OWN_LEN), -1, np.int32)
    out.update(opts=o, t_begin=float(t_begin), dim=dim)
    tr = trace if trace is not None else {}

    def count(k, n=1):
        tr[k] = tr.get(k, 0) + n

    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0:
                out["status"][r] = 2
                count("status2")
                continue
            xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
            A = own_slots(ts[N - 1], o["slot"])
            if A > MAX_OWN:
                out["status"][r] = 4
                count("status4")
                continue
            if S["n"] == 0:
                out["status"][r], out["arrive"][r], out["pauses"][r], out["own_slots"][r] = 0, A, 0, A
                out["own"][r] = np.minimum(np.arange(OWN_LEN), A)
                count("status0")
                count("n0")
                continue
            pos = positions(xs, vs, ts, A, o["slot"])
            pause, play, reach = tables(pos, S, TB, o, variant)
            if keep is not None:
                keep[r] = dict(pos=pos, pause=pause, play=play, reach=reach)
            hit = np.flatnonzero(reach[A])
            out["own_slots"][r] = A
            if hit.size == 0:
                out["status"][r] = 3
                count("status3")
                continue
            pstar = int(hit[0])
            own, first, w = walk(pause, play, reach, pstar, o["press_on"], variant)
            out["status"][r] = 1 if pstar > 0 else 0
            out["arrive"][r], out["pauses"][r], out["first_pause"][r] = A + pstar, pstar, first
            out["own"][r, :own.size] = own
            out["own"][r, own.size:] = A
            count("status%d" % out["status"][r])
            for k in ("both", "play", "pause"):
                count(k, w[k])
            tr["groups"] = max(tr.get("groups", 0), w["groups"])
    return out


def own_at(sched, r, k):
    """own(k) of trajectory r for any real slot k >= 0."""
    return int(sched["own"][r, k]) if k < OWN_LEN else int(sched["own_slots"][r])


def sched_positions(x, v, t, sched, r, k0, count):
    """pos_own(k0 + j), j = 0 .. count - 1, of trajectory r: [count, dim] f64."""
    xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
    slot = F64(sched["opts"]["slot"])
    memo = {}
    out = []
    for j in range(count):
        a = own_at(sched, r, k0 + j)
        if a not in memo:
            memo[a] = timing_ref.position(xs, vs, ts, F64(a) * slot)
        out.append(memo[a])
    return np.stack(out)


def controls_of_positions(p, dt, w_limit, min_move):
    """timing_ref.controls' second stage on the positions p [T + 1, dim]: (U [T, nu], heading0 [2], clamped)."""
    T, dim = p.shape[0] - 1, p.shape[1]
    nu = 4 if dim == 3 else 2
    dt, w_limit, min_move = F64(dt), F64(w_limit), F64(min_move)
    half = F64(0.5) * dt
    U = np.zeros((T, nu), F64)
    D = [p[k + 1] - p[k] for k in range(T)]
    n = [np.sqrt(d[0] * d[0] + d[1] * d[1]) for d in D]
    mov = [n[k] > min_move for k in range(T)]
    first = mov.index(True) if any(mov) else -1
    H, last = [], -1
    for k in range(T):
        last = k if mov[k] else last
        j = last if last >= 0 else first
        H.append((F64(1.0), F64(0.0)) if j < 0 else (D[j][0] / n[j], D[j][1] / n[j]))
    H.append(H[T - 1])
    clamped = 0
    for k in range(T):
        c, s = H[k]
        c1, s1 = H[k + 1]
        d = D[k]
        U[k, 0] = (c * d[0] + s * d[1]) / dt
        if dim == 3:
            U[k, 1] = ((-s) * d[0] + c * d[1]) / dt
            U[k, 2] = d[2] / dt
        num = c * s1 - s * c1
        den = F64(1.0) + (c * c1 + s * s1)
        if den <= 0:
            w = (w_limit if num >= 0 else -w_limit) if w_limit > 0 else F64(0.0)
            clamped += 1
        else:
            w = (num / den) / half
            if w_limit > 0 and w > w_limit:
                w = w_limit
                clamped += 1
            elif w_limit > 0 and w < -w_limit:
                w = -w_limit
                clamped += 1
        U[k, nu - 1] = w
    return U, np.array(H[0], F64), clamped


def controls(x, v, t, tstatus, sched, T, k0=0, w_limit=0.0, min_move=1e-9):
    """Control sequences along the schedules from real slot k0 on: dict(U [m, T, nu] f64, heading0 [m, 2], p0 [m, dim],
    clamped [m] i32, p [m, T + 1, dim]).  A trajectory without a timing or a schedule (status >= 2): zero controls, heading0
    (1, 0), p0 = x_0, p = NaN."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    T, k0 = int(T), int(k0)
    if not (1 <= T <= timing_ref.MAX_T and 0 <= k0 <= 1 << 20 and w_limit >= 0 and np.isfinite(w_limit) and min_move >= 0 and
            np.isfinite(min_move)):
        raise ValueError("bad arguments")
    nu = 4 if dim == 3 else 2
    U = np.zeros((m, T, nu), F64)
    h0 = np.zeros((m, 2), F64)
    h0[:, 0] = 1.0
    p0 = x[:, 0].astype(F64)
    P = np.full((m, T + 1, dim), np.nan, F64)
    clamped = np.zeros(m, np.int32)
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0 or sched["status"][r] >= 2:
                continue
            p = sched_positions(x, v, t, sched, r, k0, T + 1)
            U[r], h0[r], clamped[r] = controls_of_positions(p, sched["opts"]["slot"], w_limit, min_move)
            p0[r] = p[0]
            P[r] = p
    return dict(U=U, heading0=h0, p0=p0, clamped=clamped, p=P)


def check(x, v, t, tstatus, sched, S, steps, clearance=None):
    """obst_ref.check's dict along the schedules: p_k = pos_own(k), k = 0 .. steps, the balls of S at the real slots from the
    schedule's t_begin.  clearance None: the set's own."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    steps = int(steps)
    clearance = S["opts"]["clearance"] if clearance is None else clearance
    if not (math.isfinite(float(clearance)) and 1 <= steps <= 4096 and clearance >= 0):
        raise ValueError("bad arguments")
    if S["dim"] != dim:
        raise ValueError("a set of another dim")
    slot, clearance = F64(sched["opts"]["slot"]), F64(clearance)
    TB = F64(sched["t_begin"]) - F64(S["epoch"])
    out = dict(min_sep=np.full(m, np.nan, F64), min_time=np.full(m, np.nan, F64), min_obstacle=np.full(m, -1, np.int32),
               first_hit=np.full(m, -1, np.int32), collides=np.zeros(m, np.int32))
    n = S["n"]
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0 or sched["status"][r] >= 2:
                continue
            out["min_sep"][r] = np.inf
            if n == 0:
                continue
            p = sched_positions(x, v, t, sched, r, 0, steps + 1)
            tau = [F64(0.0) + F64(k) * slot for k in range(steps + 1)]
            e = np.array([TB + tk for tk in tau], F64)
            o = S["c"][None, :, :] + S["v"][None, :, :] * e[:, None, None]
            A = p[:-1, None, :] - o[:-1]
            B = (p[1:] - p[:-1])[:, None, :] - (o[1:] - o[:-1])
            bb, ab = B[..., 0] * B[..., 0], A[..., 0] * B[..., 0]
            for a in range(1, dim):
                bb = bb + B[..., a] * B[..., a]
                ab = ab + A[..., a] * B[..., a]
            xx = (-ab) / np.where(bb > 0, bb, F64(1.0))
            s = np.where(xx > 0, xx, F64(0.0))
            s = np.where(s < 1, s, F64(1.0))
            s = np.where(bb > 0, s, F64(0.0))
            q = A[..., 0] + s * B[..., 0]
            s2 = q * q
            for a in range(1, dim):
                q = A[..., a] + s * B[..., a]
                s2 = s2 + q * q
            sp = np.sqrt(s2) - S["r"][None, :]
            flat = np.where(np.isnan(sp), np.inf, sp).ravel()
            if flat.min() < np.inf:
                idx = int(np.flatnonzero(flat == flat.min())[0])
                bk, bi = idx // n, idx % n
                out["min_sep"][r] = flat[idx]
                out["min_time"][r] = tau[bk] + s[bk, bi] * slot
                out["min_obstacle"][r] = bi
            hit = np.flatnonzero((sp < clearance).any(axis=1))
            if hit.size:
                out["first_hit"][r], out["collides"][r] = int(hit[0]), 1
    return out


__all__ = ["default_opts", "check_opts", "own_slots", "positions", "sep", "tables", "walk", "solve", "own_at", "sched_positions",
           "controls_of_positions", "controls", "check", "MAX_OWN", "MAX_PAUSE", "OWN_LEN", "OPT_KEYS", "VARIANTS", "RES_KEYS"]
