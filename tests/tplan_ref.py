"""Reference for the planner through space and time (csrc/tplan.hip, gpis_tplan_*): a numpy statement of the
contract, written independently of the product (it imports nothing from gpismap_amd).  The static part is plan_ref's Problem
(free space, point costs, the translations and their weights, the goals); the set of balls is obst_ref's; the slot clock, the
separation of one interval from one ball and the control stage are retime_ref's.  sep_s() below is retime_ref.sep for whole
arrays of intervals at once (and it also returns where in the interval the two are closest, which retime_ref.sep keeps to
itself); tests/test_tplan_ref.py holds it to retime_ref.sep bit for bit.

Contract (2-D fields only).  States are (lattice point p, real slot s), s = 0 .. S, each slot `slot` seconds long;
TB = t_begin - epoch in double.  World point P(p) = (double)(origin + (float)i * step) per axis.
- Moves out of p during slot s: the planner's translations (codes 9 .. 17 without 13, connectivity 0 / 1, no corner cutting,
  weight w = (len * step) * (0.5f * (c[p] + c[q]))) in rising code, then the wait p -> p, code 27, weight (wait * step) * c[p],
  all float32.
- A move p -> q during slot s is clear iff no ball i has sep(P(p), P(q) - P(p), s, i) < dyn_clearance (a NaN is not below it).
- h[S][p] = 0 at the kept goals and +inf elsewhere.  For s = S - 1 .. 0: h[s][p] = 0 at goals, +inf where p is not free, else
  the minimum of fl(h[s+1][q] + w) over the moves that exist, are clear during slot s and have h[s+1][q] finite.
- policy[s][p] = 13 at goals, else the minimising code (ties: the smaller h[s+1][q], then the order offered), 255 without a
  candidate; policy[S] = 13 at goals and 255 elsewhere.
- paths(): every start is at slot 0, snapped like a goal.  Status 1 outside / non-finite, 2 not free, 3 h[0] = +inf; status 0:
  the policy is followed from slot 0 until code 13, one float32 world point per slot: arrive + 1 points.
- check(): retime_ref.check's five outputs over the intervals s = 0 .. arrive - 1 of each status-0 path against any 2-D set.
- controls(): retime_ref.controls_of_positions on P(point at slot min(k0 + k, arrive)), k = 0 .. T, dt = slot.

The `variant` arguments build the defective variants tests/test_tplan_ref.py rejects; None is the contract:
  "sample_only" (a move tested at its first sample only), "slot_off" (the balls taken one slot late), "wait_first" (the wait
  offered before the translations), "target_only" (the clearance tested at the move's target at the end of the slot only)."""
import math

import numpy as np

import obst_ref      # noqa: F401  (the set S is obst_ref.make's dict: dim, n, c, v, r, epoch)
import plan_ref
import retime_ref

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
WAIT, STAY, NONE = 27, 13, 255
MAX_S = 1024
MAX_T = 256
OPT_KEYS = ("clearance", "margin", "gain", "connectivity", "slot", "horizon", "dyn_clearance", "wait", "keep_cost")
VARIANTS = ("sample_only", "slot_off", "wait_first", "target_only")
CHECK_KEYS = ("min_sep", "min_time", "min_obstacle", "first_hit", "collides")


def default_opts(step):
    """The library's defaults (gpis_tplan_default_opts) for a field of lattice step `step`."""
    step = float(F32(step))
    return dict(clearance=0.0, margin=float(F32(4) * F32(step)), gain=4.0, connectivity=1, slot=0.1, horizon=256, dyn_clearance=step,
                wait=0.5, keep_cost=0)


def check_opts(o, shape=None):
    """ValueError for what the library answers with GPIS_ERR_ARG, OverflowError for GPIS_ERR_LIMIT."""
    f = {k: float(o[k]) for k in ("clearance", "margin", "gain", "slot", "dyn_clearance", "wait")}
    if not all(math.isfinite(v) for v in f.values()):
        raise ValueError("a non-finite option")
    if f["margin"] < 0 or f["gain"] < 0 or f["gain"] > 1e4 or o["connectivity"] not in (0, 1):
        raise ValueError("the planner's ranges")
    if not f["slot"] > 0 or f["dyn_clearance"] < 0 or not 0 <= f["wait"] <= 1e4 or o["keep_cost"] not in (0, 1):
        raise ValueError("slot, dyn_clearance, wait or keep_cost outside its range")
    if int(o["horizon"]) != o["horizon"] or not 1 <= int(o["horizon"]) <= MAX_S:
        raise ValueError("horizon outside [1, 1024]")
    if shape is not None and shape[0] * shape[1] * (int(o["horizon"]) + 1) > (1 << 28 if o["keep_cost"] else 1 << 30):
        raise OverflowError("too many states")


def sep_s(p0, dp, e0, e1, S, sample_only=False):
    """(sep, s) of the intervals that start at p0 [..., 2] with the displacement dp [..., 2] while ball i goes from its place
    at the elapsed time e0 to that at e1 (arrays that broadcast against p0[..., 0]): [..., n] each.  retime_ref.sep's
    expression, operation for operation."""
    e0, e1 = np.asarray(e0, F64)[..., None], np.asarray(e1, F64)[..., None]
    A, B = [], []
    for a in range(2):
        o0 = S["c"][:, a] + S["v"][:, a] * e0
        o1 = S["c"][:, a] + S["v"][:, a] * e1
        A.append(p0[..., a, None] - o0)
        B.append(dp[..., a, None] - (o1 - o0))
    bb = B[0] * B[0] + B[1] * B[1]
    ab = A[0] * B[0] + A[1] * B[1]
    xx = (-ab) / np.where(bb > 0, bb, F64(1.0))
    s = np.where(xx > 0, xx, F64(0.0))
    s = np.where(s < 1, s, F64(1.0))
    s = np.where(bb > 0, s, F64(0.0))
    if sample_only:
        s = np.zeros_like(s)
    q = A[0] + s * B[0]
    s2 = q * q
    q = A[1] + s * B[1]
    s2 = s2 + q * q
    return np.sqrt(s2) - S["r"], s


def axis_points(origin, step, n):
    """P of the lattice indices -1 .. n along one axis: [n + 2] f64 (index i at [i + 1])."""
    return (F32(origin) + np.arange(-1, n + 1).astype(F32) * F32(step)).astype(F32).astype(F64)


def solve(dist, shape, origin, step, goals, S=None, t_begin=0.0, opts=None, variant=None, trace=None):
    """The plan: dict(cost0 [np] f32, policy [S + 1, np] u8, c [np] f32, cost_all [S + 1, np] f32 (always kept here), pb, opts,
    t_begin, n, goals, goals_kept, free, finite0, max_cost0).  S: an obst_ref set of dim 2, or None.  trace counts wait (states
    whose policy waits), ball_blocked (candidate moves closed by a ball alone), tie_q / tie_code (ties broken by h[s+1][q] / by
    the order offered), nan_sep (NaN separations met)."""
    o = dict(default_opts(step) if opts is None else opts)
    check_opts(o, shape)
    if len(shape) != 2:
        raise ValueError("2-D fields only")
    if not math.isfinite(float(t_begin)):
        raise ValueError("a non-finite t_begin")
    n = 0 if S is None else S["n"]
    if n and S["dim"] != 2:
        raise ValueError("a set of another dim")
    pb = plan_ref.Problem(dist, shape, origin, step, goals, o["clearance"], o["margin"], o["gain"], o["connectivity"])
    nx, ny = shape
    H, slot, clr = int(o["horizon"]), F64(o["slot"]), F64(o["dyn_clearance"])
    TB = F64(t_begin) - F64(S["epoch"]) if n else F64(0.0)
    ww = (F32(o["wait"]) * pb.step) * pb.c
    assert ww.dtype == F32
    moves = list(pb.edges) + [(WAIT, (0, 0, 0), pb.free, ww)]
    if variant == "wait_first":
        moves = moves[-1:] + moves[:-1]
    px, py = axis_points(origin[0], step, nx), axis_points(origin[1], step, ny)
    P = np.stack(np.broadcast_arrays(px[None, 1:-1], py[1:-1, None]), axis=-1)            # [ny, nx, 2]
    tr = trace if trace is not None else {}

    def count(k, v):
        tr[k] = tr.get(k, 0) + int(v)

    def clear(s, off, cand):
        """[1, ny, nx]: the move by `off` during slot s is clear of every ball (evaluated everywhere; used where cand)."""
        dx, dy = off[0], off[1]
        dp = np.stack(np.broadcast_arrays((px[1 + dx:nx + 1 + dx] - px[1:-1])[None, :], (py[1 + dy:ny + 1 + dy] - py[1:-1])[:, None]), axis=-1)
        k = s + 1 if variant == "slot_off" else s
        e0, e1 = TB + F64(k) * slot, TB + F64(k + 1) * slot
        if variant == "target_only":
            sp, _ = sep_s(P + dp, np.zeros_like(dp), e1, e1, S)
        else:
            sp, _ = sep_s(P, dp, e0, e1, S, variant == "sample_only")
        count("nan_sep", np.isnan(sp)[cand[0]].sum())
        return ~(sp < clr).any(axis=-1)[None]

    h = pb.start_cost()
    pol = np.zeros((H + 1, ny * nx), np.uint8)
    pol[H] = np.where(pb.goal, np.uint8(STAY), np.uint8(NONE)).ravel()
    call = np.zeros((H + 1, ny * nx), F32)
    call[H] = h.ravel()
    with np.errstate(all="ignore"):
        for s in range(H - 1, -1, -1):
            best = np.full(pb.n3, INF, F32)
            bestq = np.full(pb.n3, INF, F32)
            code = np.full(pb.n3, NONE, np.uint8)
            for k, off, e, w in moves:
                cq = plan_ref._nbr(h, off, INF)
                cand = e & np.isfinite(cq) & ~pb.goal
                if n and cand.any():
                    ok = cand & clear(s, off, cand)
                    count("ball_blocked", (cand & ~ok).sum())
                else:
                    ok = cand
                v = cq + w
                assert v.dtype == F32
                tq = ok & (v == best) & (cq < bestq)
                count("tie_q", tq.sum())
                count("tie_code", (ok & (v == best) & (cq == bestq) & np.isfinite(best)).sum())
                take = ok & ((v < best) | tq)
                best = np.where(take, v, best)
                bestq = np.where(take, cq, bestq)
                code = np.where(take, np.uint8(k), code)
            h = np.where(pb.goal, F32(0), best).astype(F32)
            code = np.where(pb.goal, np.uint8(STAY), code)
            count("wait", (code == WAIT).sum())
            pol[s] = code.ravel()
            call[s] = h.ravel()
    cost0 = call[0].copy()
    fin = np.isfinite(cost0)
    return dict(cost0=cost0, policy=pol, c=pb.c.ravel().copy(), cost_all=call, pb=pb, opts=o, t_begin=float(t_begin), n=n,
                goals=pb.goals_given, goals_kept=pb.goals_kept, free=int(pb.free.sum()), finite0=int(fin.sum()),
                max_cost0=float(cost0[fin].max()) if fin.any() else 0.0)


def paths(sol, starts):
    """dict(off i64 [m + 1], points f32 [off[m], 2], arrive i32 [m] (-1 unless status 0), start_cost f32 [m], status u8 [m],
    cells: per path the lattice indices [arrive + 1, 2], starts f32 [m, 2])."""
    pb, pol, cost0 = sol["pb"], sol["policy"], sol["cost0"]
    nx, ny = pb.shape
    H = pol.shape[0] - 1
    starts = np.ascontiguousarray(starts, F32).reshape(-1, 2)
    ok, ijk = plan_ref.snap(starts, pb.shape, pb.origin, pb.step)
    m = ok.size
    status = np.zeros(m, np.uint8)
    sc = np.full(m, np.nan, F32)
    arrive = np.full(m, -1, np.int32)
    free = pb.free.ravel()
    cells = []
    for t in range(m):
        pts = []
        if not ok[t]:
            status[t] = 1
        else:
            i, j = int(ijk[t, 0]), int(ijk[t, 1])
            p = j * nx + i
            sc[t] = cost0[p]
            if not free[p]:
                status[t] = 2
            elif not np.isfinite(cost0[p]):
                status[t] = 3
            else:
                s = 0
                pts.append((i, j))
                while pol[s, j * nx + i] != STAY:
                    k = int(pol[s, j * nx + i])
                    assert k != NONE and s < H
                    if k != WAIT:
                        dx, dy, _ = plan_ref.offset(k)
                        i, j = i + dx, j + dy
                    s += 1
                    pts.append((i, j))
                arrive[t] = s
        cells.append(np.array(pts, np.int64).reshape(-1, 2))
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([c.shape[0] for c in cells])
    allc = np.concatenate(cells) if m else np.zeros((0, 2), np.int64)
    return dict(off=off, points=pb.world(allc).reshape(-1, 2), arrive=arrive, start_cost=sc, status=status, cells=cells, starts=starts)


def check(sol, pa, S, clearance=None):
    """retime_ref.check's dict over the intervals s = 0 .. arrive - 1 of each status-0 path of pa against the set S at the
    solve's t_begin and slot.  clearance None: the solve's dyn_clearance."""
    clearance = sol["opts"]["dyn_clearance"] if clearance is None else clearance
    if not (math.isfinite(float(clearance)) and clearance >= 0):
        raise ValueError("bad arguments")
    n = S["n"]
    if n and S["dim"] != 2:
        raise ValueError("a set of another dim")
    m = pa["status"].size
    slot, clearance = F64(sol["opts"]["slot"]), F64(clearance)
    TB = F64(sol["t_begin"]) - F64(S["epoch"])
    out = dict(min_sep=np.full(m, np.nan, F64), min_time=np.full(m, np.nan, F64), min_obstacle=np.full(m, -1, np.int32),
               first_hit=np.full(m, -1, np.int32), collides=np.zeros(m, np.int32))
    with np.errstate(all="ignore"):
        for r in range(m):
            if pa["status"][r] != 0:
                continue
            out["min_sep"][r] = np.inf
            A = int(pa["arrive"][r])
            if n == 0 or A == 0:
                continue
            p = pa["points"][pa["off"][r]:pa["off"][r + 1]].astype(F64)
            k = np.arange(A)
            tau = F64(0.0) + k.astype(F64) * slot
            sp, s = sep_s(p[:-1], p[1:] - p[:-1], TB + k.astype(F64) * slot, TB + (k + 1).astype(F64) * slot, S)
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


def controls(sol, pa, T, k0=0, w_limit=0.0, min_move=1e-9):
    """dict(U [m, T, 2] f64, heading0 [m, 2], p0 [m, 2], clamped [m] i32): retime_ref.controls_of_positions on the positions
    P(point at slot min(k0 + k, arrive)), k = 0 .. T; a path of status != 0 stands still, p0 the start as given."""
    T, k0 = int(T), int(k0)
    if not (1 <= T <= MAX_T and 0 <= k0 <= 1 << 20 and w_limit >= 0 and np.isfinite(w_limit) and min_move >= 0 and np.isfinite(min_move)):
        raise ValueError("bad arguments")
    m = pa["status"].size
    U = np.zeros((m, T, 2), F64)
    h0 = np.zeros((m, 2), F64)
    h0[:, 0] = 1.0
    p0 = pa["starts"].astype(F64)
    clamped = np.zeros(m, np.int32)
    with np.errstate(all="ignore"):
        for r in range(m):
            if pa["status"][r] != 0:
                continue
            p = pa["points"][pa["off"][r]:pa["off"][r + 1]].astype(F64)
            pos = p[np.minimum(k0 + np.arange(T + 1), int(pa["arrive"][r]))]
            U[r], h0[r], clamped[r] = retime_ref.controls_of_positions(pos, sol["opts"]["slot"], w_limit, min_move)
            p0[r] = pos[0]
    return dict(U=U, heading0=h0, p0=p0, clamped=clamped)


def waits(pa, r):
    """The number of slots path r of pa stands still before it arrives."""
    c = pa["cells"][r]
    return int((c[1:] == c[:-1]).all(axis=1).sum())


__all__ = ["default_opts", "check_opts", "sep_s", "axis_points", "solve", "paths", "check", "controls", "waits", "OPT_KEYS", "VARIANTS",
           "CHECK_KEYS", "MAX_S", "MAX_T", "WAIT", "STAY", "NONE"]
