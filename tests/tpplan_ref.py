"""Reference for the time-pose planner (csrc/tpplan.hip, gpis_tpplan_*): a numpy statement of the contract, written
independently of the product (it imports nothing from gpismap_amd).  It is tplan_ref.solve's layer recursion on pplan_ref's
lattice of poses: the static part (free space, point costs, the directed translations, the two turns, their weights, the goals)
is pplan_ref.Problem, the slot clock tplan_ref's, a body ball's place body_ref.ball_positions (through body_time_ref.ball_tracks)
and its separation from a moving ball over one interval body_time_ref.seps.

Contract (2-D fields only).  States are (i, j, h, s): lattice point, heading index h of the caller's table [H, 2], real slot
s = 0 .. S of `slot` seconds; index within a layer (h ny + j) nx + i; TB = t_begin - epoch in double.
- Moves out of (p, h) during slot s, every one taking one slot: pplan_ref's translations (codes 9 .. 17 without 13) in rising
  code, the turns 27 (h + 1) and 28 (h - 1), then the wait (p, h) -> (p, h), code 29, weight (wait * step) * c[s] in float32.
- Clearance of a move (p, h) -> (q, h') during slot s: body ball j starts at W0 = body_ref.ball_positions at (P(p), (c_h, s_h)),
  ends at W1 = the same at (P(q), h'), dW = W1 - W0; sep = body_time_ref.seps(W0, dW, e0, e1) with e0 = TB + (double)s * slot,
  e1 = TB + (double)(s + 1) * slot.  The move is clear iff no pair (i, j) has sep < dyn_clearance (a NaN is not below it).
- h[S] = 0 at the kept goals, +inf elsewhere; for s = S - 1 .. 0: 0 at goals, +inf where the state is not free, else the minimum
  of fl(h[s+1][s'] + w) over the moves that exist statically, are clear during slot s and have a finite target.
- policy: 13 at goals, else the minimising code (ties: the smaller h[s+1][s'], then the order offered), 255 without a candidate.
- paths(): starts [m, 3] at slot 0, snapped like goals; h = -1: the free heading of least slot-0 cost (ties: the smaller h).
  Status 1 outside / non-finite, 2 no free heading or the given one not free, 3 cost +inf; status 0: the policy is followed
  until code 13, one float32 world point and one int32 heading index per slot: arrive + 1 entries.
- check(): body_time_ref's six outputs over the intervals s = 0 .. arrive - 1 of each status-0 path, against any 2-D set and any
  2-D footprint, at the solve's t_begin, slot and heading table.
- controls(): tplan_ref.controls on the path's points (a turn repeats its point, as a wait does).

The `variant` arguments build the defective variants tests/test_tpplan_ref.py rejects; None is the contract:
  "no_rho" (rho_j not subtracted), "centre_only" (only the reference point tested, as a ball of radius 0), "turn_hold" (a turn
  tested with heading h at both ends), "sample_only" (a move tested at its first sample only), "slot_off" (the balls taken one
  slot late), "wait_first" (the wait offered before the other moves)."""
import math

import numpy as np

import body_ref
import body_time_ref as btr
import obst_ref      # noqa: F401  (the set S is obst_ref.make's dict: dim, n, c, v, r, epoch)
import plan_ref
import pplan_ref
import retime_ref    # noqa: F401  (controls_of_positions, through tplan_ref.controls)
import tplan_ref

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
WAIT, STAY, NONE, TURN_UP, TURN_DOWN = 29, 13, 255, 27, 28
MAX_S = 1024
MAX_T = 256
OPT_KEYS = ("clearance", "margin", "gain", "turn", "slot", "horizon", "dyn_clearance", "wait", "keep_cost")
VARIANTS = ("no_rho", "centre_only", "turn_hold", "sample_only", "slot_off", "wait_first")
CHECK_KEYS = btr.CHECK_KEYS


def default_opts(step, H=16):
    """The library's defaults (gpis_tpplan_default_opts) for a field of lattice step `step` and H headings."""
    if H not in pplan_ref.HS:
        raise ValueError("H outside {8, 16, 32, 64}")
    step = float(F32(step))
    return dict(clearance=0.0, margin=float(F32(4) * F32(step)), gain=4.0, turn=step, slot=0.1, horizon=256, dyn_clearance=step, wait=0.5,
                keep_cost=0)


def check_opts(o, H, step=None, shape=None):
    """ValueError for what the library answers with GPIS_ERR_ARG, OverflowError for GPIS_ERR_LIMIT.  step None: the lattice is not
    known, and turn is only asked to be positive."""
    if H not in pplan_ref.HS:
        raise ValueError("H outside {8, 16, 32, 64}")
    f = {k: float(o[k]) for k in ("clearance", "margin", "gain", "turn", "slot", "dyn_clearance", "wait")}
    if not all(math.isfinite(v) for v in f.values()):
        raise ValueError("a non-finite option")
    if f["margin"] < 0 or f["gain"] < 0 or f["gain"] > 1e4 or not f["turn"] > 0:
        raise ValueError("the pose planner's ranges")
    if step is not None:
        pplan_ref.check_opts(step, H, o["clearance"], o["margin"], o["gain"], o["turn"])
    if not f["slot"] > 0 or f["dyn_clearance"] < 0 or not 0 <= f["wait"] <= 1e4 or o["keep_cost"] not in (0, 1):
        raise ValueError("slot, dyn_clearance, wait or keep_cost outside its range")
    if int(o["horizon"]) != o["horizon"] or not 1 <= int(o["horizon"]) <= MAX_S:
        raise ValueError("horizon outside [1, 1024]")
    if shape is not None and shape[0] * shape[1] * H * (int(o["horizon"]) + 1) > (1 << 28 if o["keep_cost"] else 1 << 30):
        raise OverflowError("too many states")


def balls_at(body, X, Y, headings, h):
    """W [K, m_body, 2]: the body's balls at the world points (X, Y) [K] f64 with the headings of the indices h [K]."""
    Q = np.stack([X, Y, headings[h, 0], headings[h, 1]], axis=1)
    return btr.ball_tracks(body, Q)


def move_seps(body, S, headings, px, py, idx, off, H, e0, e1, variant=None, sample_only=False):
    """(sep, s) [K, n, m_body] of the move by off = (dx, dy, dh) out of the states idx = (h, j, i) (arrays [K]) while the balls of
    S go from their places at e0 to those at e1.  px, py: tplan_ref.axis_points (index i at [i + 1])."""
    hh, jj, ii = idx
    dx, dy, dh = off
    W0 = balls_at(body, px[ii + 1], py[jj + 1], headings, hh)
    h1 = hh if variant == "turn_hold" else (hh + dh) % H
    W1 = balls_at(body, px[ii + 1 + dx], py[jj + 1 + dy], headings, h1)
    K = hh.size
    return btr.seps(W0, W1 - W0, np.full(K, e0, F64), np.full(K, e1, F64), S, body, sample_only or variant == "sample_only",
                    "no_rho" if variant == "no_rho" else None)


def solve(dist, shape, origin, step, body, headings, moves, goals, S=None, t_begin=0.0, opts=None, variant=None, trace=None):
    """The plan: dict(cost0 [H ny nx] f32, policy [S + 1, H ny nx] u8, c f32, cost_all [S + 1, H ny nx] f32 (always kept here),
    pb, body, headings, opts, t_begin, n, goals, goals_kept, free, finite0, max_cost0).  S: an obst_ref set of dim 2, or None.
    trace counts wait (states whose policy waits), ball_blocked, tie_q / tie_code, nan_sep, turn_for_ball (a turn chosen where
    balls close every translation open at heading h and one is clear at the heading turned to), rear_alone (a translation closed by body
    balls j > 0 alone, the reference point and ball 0 clear), turn_swept (a turn closed by a ball that the pose held at either
    end clears), tunnel (a move closed with both its end samples clear)."""
    assert variant is None or variant in VARIANTS, variant
    headings = np.ascontiguousarray(headings, F64).reshape(-1, 2)
    H = headings.shape[0]
    o = dict(default_opts(step, H) if opts is None else opts)
    check_opts(o, H, step, shape)
    if len(shape) != 2:
        raise ValueError("2-D fields only")
    if not math.isfinite(float(t_begin)):
        raise ValueError("a non-finite t_begin")
    n = 0 if S is None else S["n"]
    if n and S["dim"] != 2:
        raise ValueError("a set of another dim")
    pb = pplan_ref.Problem(dist, shape, origin, step, body, headings, moves, goals, o["clearance"], o["margin"], o["gain"], o["turn"])
    nx, ny = pb.shape
    ns = H * ny * nx
    Sn, slot, clr = int(o["horizon"]), F64(o["slot"]), F64(o["dyn_clearance"])
    TB = F64(t_begin) - F64(S["epoch"]) if n else F64(0.0)
    ww = (F32(o["wait"]) * pb.step) * pb.c
    assert ww.dtype == F32
    mvs = list(pb.edges) + [(WAIT, (0, 0, 0), pb.free, ww)]
    if variant == "wait_first":
        mvs = mvs[-1:] + mvs[:-1]
    px, py = tplan_ref.axis_points(origin[0], step, nx), tplan_ref.axis_points(origin[1], step, ny)
    tbody = body_ref.point(2) if variant == "centre_only" else body
    tr = trace if trace is not None else {}

    def count(k, v):
        tr[k] = tr.get(k, 0) + int(v)

    def clear(s, off, cand):
        """[H, ny, nx] bool: the move by `off` during slot s is clear of every ball, evaluated where cand (True elsewhere)."""
        idx = np.nonzero(cand)
        k = s + 1 if variant == "slot_off" else s
        e0, e1 = TB + F64(k) * slot, TB + F64(k + 1) * slot
        sp, _ = move_seps(tbody, S, headings, px, py, idx, off, H, e0, e1, variant)
        count("nan_sep", np.isnan(sp).sum())
        hit = sp < clr
        bad = hit.any(axis=(1, 2))
        if trace is not None and variant is None and bad.any():
            b = tuple(a[bad] for a in idx)
            K = b[0].size
            ee0, ee1 = np.full(K, e0, F64), np.full(K, e1, F64)
            Wa = balls_at(body, px[b[2] + 1], py[b[1] + 1], headings, b[0])
            Wb = balls_at(body, px[b[2] + 1 + off[0]], py[b[1] + 1 + off[1]], headings, (b[0] + off[2]) % H)
            first = ~(btr.seps(Wa, np.zeros_like(Wa), ee0, ee0, S, body)[0] < clr).any(axis=(1, 2))
            last = ~(btr.seps(Wb, np.zeros_like(Wb), ee1, ee1, S, body)[0] < clr).any(axis=(1, 2))
            count("tunnel", (first & last).sum())
            if off[2]:
                ha = ~(btr.seps(Wa, np.zeros_like(Wa), ee0, ee1, S, body)[0] < clr).any(axis=(1, 2))
                hb = ~(btr.seps(Wb, np.zeros_like(Wb), ee0, ee1, S, body)[0] < clr).any(axis=(1, 2))
                count("turn_swept", (ha & hb).sum())
            elif off[0] or off[1]:
                pt = body_ref.point(2)
                ps, _ = move_seps(pt, S, headings, px, py, b, off, H, e0, e1)
                byj = hit[bad].any(axis=1)                                  # [K, m_body]
                count("rear_alone", (~(ps < clr).any(axis=(1, 2)) & ~byj[:, 0] & byj[:, 1:].any(axis=1)).sum())
        out = np.ones(pb.n3, bool)
        out[idx] = ~bad
        return out

    h = pb.start_cost()
    pol = np.zeros((Sn + 1, ns), np.uint8)
    pol[Sn] = np.where(pb.goal, np.uint8(STAY), np.uint8(NONE)).ravel()
    call = np.zeros((Sn + 1, ns), F32)
    call[Sn] = h.ravel()
    with np.errstate(all="ignore"):
        for s in range(Sn - 1, -1, -1):
            best = np.full(pb.n3, INF, F32)
            bestq = np.full(pb.n3, INF, F32)
            code = np.full(pb.n3, NONE, np.uint8)
            shut, fine = {}, {}
            for k, off, e, w in mvs:
                cq = pplan_ref._shift(h, off, INF)
                cand = e & np.isfinite(cq) & ~pb.goal
                if n and cand.any():
                    ok = cand & clear(s, off, cand)
                    count("ball_blocked", (cand & ~ok).sum())
                else:
                    ok = cand
                if trace is not None and k < 18:
                    shut[k], fine[k] = cand & ~ok, ok
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
            if trace is not None and n:
                shut_any = np.logical_or.reduce(list(shut.values()))
                fine_any = np.logical_or.reduce(list(fine.values()))
                for kt, dh in ((TURN_UP, 1), (TURN_DOWN, -1)):
                    why = shut_any & ~fine_any & pplan_ref._shift(fine_any, (0, 0, dh), False)
                    count("turn_for_ball", ((code == kt) & why).sum())
            pol[s] = code.ravel()
            call[s] = h.ravel()
    cost0 = call[0].copy()
    fin = np.isfinite(cost0)
    return dict(cost0=cost0, policy=pol, c=pb.c.ravel().copy(), cost_all=call, pb=pb, body=body, headings=headings, opts=o,
                t_begin=float(t_begin), n=n, goals=pb.goals_given, goals_kept=pb.goals_kept, free=int(pb.free.sum()),
                finite0=int(fin.sum()), max_cost0=float(cost0[fin].max()) if fin.any() else 0.0)


def paths(sol, starts, trace=None):
    """dict(off i64 [m + 1], points f32 [off[m], 2], heading i32 [off[m]], arrive i32 [m] (-1 unless status 0), start_cost f32
    [m], status u8 [m], cells: per path the states [arrive + 1, 3] = (i, j, h), starts f32 [m, 3]).  trace counts any_heading
    (starts with h = -1 that found a free heading)."""
    pb, pol, cost0 = sol["pb"], sol["policy"], sol["cost0"]
    H, ny, nx = pb.n3
    Sn = pol.shape[0] - 1
    st_ = np.ascontiguousarray(starts, F32).reshape(-1, 3)
    sh = pplan_ref.goal_headings(st_[:, 2], H)
    ok, ij = plan_ref.snap(st_[:, :2], pb.shape, pb.origin, pb.step)
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
            i, j, h = int(ij[t, 0]), int(ij[t, 1]), int(sh[t])
            if h < 0:
                h, bc = -1, INF
                for hh in range(H):
                    q = (hh * ny + j) * nx + i
                    if free[q] and (h < 0 or cost0[q] < bc):
                        h, bc = hh, cost0[q]
                if h >= 0 and trace is not None:
                    trace["any_heading"] = trace.get("any_heading", 0) + 1
            if h < 0:
                status[t], sc[t] = 2, INF
            else:
                p = (h * ny + j) * nx + i
                sc[t] = cost0[p]
                if not free[p]:
                    status[t] = 2
                elif not np.isfinite(cost0[p]):
                    status[t] = 3
                else:
                    s = 0
                    pts.append((i, j, h))
                    while pol[s, (h * ny + j) * nx + i] != STAY:
                        k = int(pol[s, (h * ny + j) * nx + i])
                        assert k != NONE and s < Sn
                        if k != WAIT:
                            dx, dy, dh = pplan_ref.move_of(k)
                            i, j, h = i + dx, j + dy, (h + dh) % H
                        s += 1
                        pts.append((i, j, h))
                    arrive[t] = s
        cells.append(np.array(pts, np.int64).reshape(-1, 3))
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([c.shape[0] for c in cells])
    allc = np.concatenate(cells) if m else np.zeros((0, 3), np.int64)
    return dict(off=off, points=pb.world(allc[:, :2]).reshape(-1, 2), heading=allc[:, 2].astype(np.int32), arrive=arrive, start_cost=sc,
                status=status, cells=cells, starts=st_)


def check(sol, pa, S, body=None, clearance=None, variant=None):
    """body_time_ref.check's dict over the intervals s = 0 .. arrive - 1 of each status-0 path of pa against the set S with the
    footprint `body` (None: the solve's) at the solve's t_begin, slot and heading table.  clearance None: the solve's
    dyn_clearance."""
    clearance = sol["opts"]["dyn_clearance"] if clearance is None else clearance
    body = sol["body"] if body is None else body
    if not (math.isfinite(float(clearance)) and clearance >= 0):
        raise ValueError("bad arguments")
    n = S["n"]
    if n and S["dim"] != 2:
        raise ValueError("a set of another dim")
    if body["m"] == 0 or body["dim"] != 2:
        raise RuntimeError("an empty footprint, or one of dimension 3")
    m = pa["status"].size
    slot, clearance = F64(sol["opts"]["slot"]), F64(clearance)
    TB = F64(sol["t_begin"]) - F64(S["epoch"])
    out = btr._blank(m)
    with np.errstate(all="ignore"):
        for r in range(m):
            if pa["status"][r] != 0:
                continue
            out["min_sep"][r] = np.inf
            A = int(pa["arrive"][r])
            if n == 0 or A == 0:
                continue
            p = pa["points"][pa["off"][r]:pa["off"][r + 1]].astype(F64)
            hd = pa["heading"][pa["off"][r]:pa["off"][r + 1]]
            W = balls_at(body, p[:, 0].copy(), p[:, 1].copy(), sol["headings"], hd)
            k = np.arange(A)
            tau = [F64(0.0) + F64(kk) * slot for kk in range(A)]
            sep, s = btr.seps(W[:-1], W[1:] - W[:-1], TB + k.astype(F64) * slot, TB + (k + 1).astype(F64) * slot, S, body, variant=variant)
            btr._reduce(out, r, sep, s, tau, slot, clearance)
    return out


def controls(sol, pa, T, k0=0, w_limit=0.0, min_move=1e-9):
    """tplan_ref.controls on the paths' points: dict(U [m, T, 2] f64, heading0 [m, 2], p0 [m, 2], clamped [m] i32)."""
    return tplan_ref.controls(sol, dict(pa, starts=np.ascontiguousarray(pa["starts"][:, :2])), T, k0, w_limit, min_move)


def waits(pa, r):
    """The number of slots path r of pa holds its pose before it arrives."""
    c = pa["cells"][r]
    return int((c[1:] == c[:-1]).all(axis=1).sum())


def turns(pa, r):
    """The number of slots path r of pa turns on the spot."""
    c = pa["cells"][r]
    return int(((c[1:, :2] == c[:-1, :2]).all(axis=1) & (c[1:, 2] != c[:-1, 2])).sum())


__all__ = ["default_opts", "check_opts", "balls_at", "move_seps", "solve", "paths", "check", "controls", "waits", "turns", "OPT_KEYS",
           "VARIANTS", "CHECK_KEYS", "MAX_S", "MAX_T", "WAIT", "STAY", "NONE", "TURN_UP", "TURN_DOWN"]
