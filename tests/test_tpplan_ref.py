"""The time-pose planner's reference (tests/tpplan_ref.py) against what it must equal without a device: the library's symbols,
defaults and refusals; body_time_ref.seps; a heapq Dijkstra on the explicit time-expanded pose graph; the pose planner with no
balls; the time planner with the one-ball zero footprint; a trace of every branch; defective variants; both certificates; and
the demonstration with body_ref.box(1.0, 0.4, 5): a disc parked on the route, which the point planner with the inscribed radius
drives the body into, the point planner with the circumscribed radius cannot pass, and the time-pose planner slides past."""
import ctypes as C
import functools
import heapq
import os
import re

import numpy as np
import pytest

import body_ref
import body_time_ref as btr
import gpismap_amd
import obst_ref
import pplan_cases
import pplan_ref
import retime_ref
import tplan_cases
import tplan_ref
import tpplan_cases as tc
import tpplan_ref as tp

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_tpplan_default_opts", "gpis_tpplan_check_opts", "gpis_tpplan_create", "gpis_tpplan_destroy", "gpis_tpplan_solve",
         "gpis_tpplan_info", "gpis_tpplan_get", "gpis_tpplan_paths", "gpis_tpplan_path_counts", "gpis_tpplan_get_paths", "gpis_tpplan_check",
         "gpis_tpplan_controls", "gpis_tpplan_set_schedule"}


@functools.lru_cache(maxsize=None)
def _small(name):
    """(case, solution, paths, trace) of a small case by the contract: computed once, left unchanged."""
    c = tc.small_case(name)
    trace = {}
    sol = tc.ref_solve(c, trace=trace)
    return c, sol, tp.paths(sol, c["starts"], trace), trace


@functools.lru_cache(maxsize=None)
def _shape(name):
    c = tc.shape_case(name)
    sol = tc.ref_solve(c)
    return c, sol, tp.paths(sol, c["starts"])


@functools.lru_cache(maxsize=None)
def _demo():
    c = tc.demo_case()
    sol = tc.ref_solve(c)
    return c, sol, tp.paths(sol, c["starts"])


def test_symbols_defaults_and_refusals():
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    assert set(re.findall(r"\b(gpis_tpplan[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_tpplan_default_opts.argtypes = [C.c_float, C.c_int, C.POINTER(gpismap_amd.gpis_tpplan_opts)]
    for step, H in ((0.25, 8), (0.1, 16), (0.2, 64)):
        o = gpismap_amd.gpis_tpplan_opts()
        assert L.gpis_tpplan_default_opts(step, H, C.byref(o)) == 0
        got = {k: getattr(o, k) for k in tp.OPT_KEYS}
        ref = tp.default_opts(step, H)
        assert all(F32(got[k]) == F32(ref[k]) for k in ("clearance", "margin", "gain", "turn", "wait")), (got, ref)
        assert all(got[k] == ref[k] for k in ("slot", "horizon", "dyn_clearance", "keep_cost")), (got, ref)
    assert (o.slot, o.horizon, o.wait, o.keep_cost, o.gain, o.clearance) == (0.1, 256, 0.5, 0, 4.0, 0.0)
    assert L.gpis_tpplan_default_opts(0.0, 16, C.byref(o)) == -1 and L.gpis_tpplan_default_opts(0.1, 16, None) == -1
    assert L.gpis_tpplan_default_opts(float("nan"), 16, C.byref(o)) == -1 and L.gpis_tpplan_default_opts(0.1, 12, C.byref(o)) == -1
    with pytest.raises(ValueError):
        tp.default_opts(0.1, 12)
    p = gpismap_amd.tpplan_opts(0.25, 8, slot=0.5, wait=2.0, horizon=9, turn=0.5)
    assert (p.slot, p.wait, p.horizon, p.dyn_clearance, p.turn) == (0.5, 2.0, 9, 0.25, 0.5)
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.tpplan_opts(0.25, 8, connectivity=1)
    # a plan lives on a handle, which lives on a device: without one the entries answer GPIS_ERR_ARG
    d, vp = C.c_double, C.c_void_p
    L.gpis_tpplan_solve.argtypes = [vp] * 6 + [C.c_int, vp, C.c_int, d, vp, vp]
    L.gpis_tpplan_check.argtypes = [vp, vp, vp, d] + [vp] * 6
    L.gpis_tpplan_controls.argtypes = [vp, C.c_int, C.c_int, d, d] + [vp] * 4
    L.gpis_tpplan_get.argtypes = [vp] * 5
    L.gpis_tpplan_paths.argtypes = [vp, vp, C.c_int, vp]
    assert L.gpis_tpplan_solve(None, None, None, None, None, None, 16, None, 1, 0.0, C.byref(o), None) == -1
    assert L.gpis_tpplan_check(None, None, None, 0.1, None, None, None, None, None, None) == -1
    assert L.gpis_tpplan_controls(None, 4, 0, 0.0, 0.0, None, None, None, None) == -1
    assert L.gpis_tpplan_get(None, None, None, None, None) == -1 and L.gpis_tpplan_paths(None, None, 1, None) == -1


BAD = (dict(slot=0.0), dict(slot=-1.0), dict(slot=float("nan")), dict(slot=float("inf")), dict(horizon=0), dict(horizon=1025),
       dict(dyn_clearance=-0.1), dict(dyn_clearance=float("nan")), dict(wait=-0.5), dict(wait=1.5e4), dict(wait=float("nan")),
       dict(keep_cost=2), dict(keep_cost=-1), dict(margin=-0.1), dict(gain=-1.0), dict(gain=2e4), dict(clearance=float("inf")),
       dict(margin=float("nan")), dict(turn=0.0), dict(turn=-0.1), dict(turn=float("nan")), dict(turn=float("inf")))
GOOD = (dict(), dict(horizon=1), dict(horizon=1024), dict(wait=0.0), dict(wait=1e4), dict(dyn_clearance=0.0), dict(keep_cost=1),
        dict(clearance=-0.3), dict(margin=0.0), dict(gain=1e4), dict(turn=1e-6), dict(turn=1e6))


def test_every_option_is_refused_alike():
    L = gpismap_amd.lib()
    for H in (8, 64):
        for kw, ok in [(k, False) for k in BAD] + [(k, True) for k in GOOD]:
            o = dict(tp.default_opts(0.1, H), **kw)
            rc = L.gpis_tpplan_check_opts(C.byref(gpismap_amd.tpplan_opts(0.1, H, **kw)), H, 0, 0)
            assert rc == (0 if ok else -1), (kw, rc)
            if ok:
                tp.check_opts(o, H)
            else:
                with pytest.raises(ValueError):
                    tp.check_opts(o, H)
    o = gpismap_amd.tpplan_opts(0.1, 16)
    assert L.gpis_tpplan_check_opts(C.byref(o), 12, 0, 0) == -1 and L.gpis_tpplan_check_opts(None, 16, 0, 0) == -1
    with pytest.raises(ValueError):
        tp.check_opts(tp.default_opts(0.1, 16), 12)
    # turn against a known lattice step: [step / 64, 1e4 step], the pose planner's range
    for turn, ok in ((0.1 / 64, True), (0.1 / 65, False), (999.0, True), (1001.0, False)):
        o = dict(tp.default_opts(0.1, 16), turn=turn)
        if ok:
            tp.check_opts(o, 16, 0.1)
        else:
            with pytest.raises(ValueError):
                tp.check_opts(o, 16, 0.1)
    # the sizes: nx ny H (S + 1) <= 2^30, 2^28 with keep_cost
    for shape, H, kw, ok in (((128, 1023), 8, dict(horizon=1023), True), ((128, 1024), 8, dict(horizon=1024), False),
                             ((128, 1024), 8, dict(horizon=1023), True), ((64, 64), 64, dict(horizon=1023, keep_cost=1), True),
                             ((64, 65), 64, dict(horizon=1023, keep_cost=1), False), ((64, 65), 32, dict(horizon=1023, keep_cost=1), True)):
        rc = L.gpis_tpplan_check_opts(C.byref(gpismap_amd.tpplan_opts(0.1, H, **kw)), H, *shape)
        assert rc == (0 if ok else -4), (shape, kw, rc)
        if ok:
            tp.check_opts(dict(tp.default_opts(0.1, H), **kw), H, None, shape)
        else:
            with pytest.raises(OverflowError):
                tp.check_opts(dict(tp.default_opts(0.1, H), **kw), H, None, shape)


def _flags(c, sol, s, off):
    """(sep, sigma) [H ny nx, n, m_body] of the move `off` out of every state during slot s, from body_ref.ball_positions and
    body_time_ref.seps directly (not through tpplan_ref.move_seps)."""
    pb, S, o, body = sol["pb"], c["obst"], sol["opts"], c["body"]
    H, ny, nx = pb.n3
    hd = sol["headings"]
    X = (F32(pb.origin[0]) + np.arange(-1, nx + 1).astype(F32) * pb.step).astype(F64)
    Y = (F32(pb.origin[1]) + np.arange(-1, ny + 1).astype(F32) * pb.step).astype(F64)
    hh, jj, ii = [a.ravel() for a in np.meshgrid(np.arange(H), np.arange(ny), np.arange(nx), indexing="ij")]
    h1 = (hh + off[2]) % H
    W0 = body_ref.ball_positions(body, [X[ii + 1], Y[jj + 1]], hd[hh, 0], hd[hh, 1])
    W1 = body_ref.ball_positions(body, [X[ii + 1 + off[0]], Y[jj + 1 + off[1]]], hd[h1, 0], hd[h1, 1])
    W0 = np.stack([np.stack(w, axis=1) for w in W0], axis=1)
    W1 = np.stack([np.stack(w, axis=1) for w in W1], axis=1)
    TB = F64(c["t_begin"]) - F64(S["epoch"])
    K = hh.size
    e0, e1 = TB + F64(s) * F64(o["slot"]), TB + F64(s + 1) * F64(o["slot"])
    with np.errstate(all="ignore"):
        return btr.seps(W0, W1 - W0, np.full(K, e0), np.full(K, e1), S, body), (hh, jj, ii)


def test_move_seps_is_body_time_refs_expression_bit_for_bit():
    c = tc.shape_case("b")
    sol = _shape("b")[1]
    pb = sol["pb"]
    H, ny, nx = pb.n3
    px, py = tplan_ref.axis_points(pb.origin[0], pb.step, nx), tplan_ref.axis_points(pb.origin[1], pb.step, ny)
    TB = F64(c["t_begin"]) - F64(c["obst"]["epoch"])
    for s, off in ((0, (1, 0, 0)), (3, (-1, 1, 0)), (5, (0, 0, 1)), (6, (0, 0, -1)), (2, (0, 0, 0))):
        (ref, sig), idx = _flags(c, sol, s, off)
        e0, e1 = TB + F64(s) * F64(0.2), TB + F64(s + 1) * F64(0.2)
        with np.errstate(all="ignore"):
            got, gs = tp.move_seps(c["body"], c["obst"], sol["headings"], px, py, idx, off, H, e0, e1)
        assert got.shape == (H * ny * nx, 65, 4)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)) and np.array_equal(gs.view(np.uint64), sig.view(np.uint64))


def _dijkstra(c, sol):
    """h [S + 1, H ny nx] of the explicit time-expanded pose graph: a backward heapq Dijkstra from every (s, goal) with the same
    float32 additions; a move's clearance flag comes from body_time_ref.seps (through _flags)."""
    pb, o = sol["pb"], sol["opts"]
    H, ny, nx = pb.n3
    Sn = int(o["horizon"])
    ww = ((F32(o["wait"]) * pb.step) * pb.c).ravel()
    moves = [(off, e.ravel(), w.ravel()) for k, off, e, w in pb.edges] + [((0, 0, 0), pb.free.ravel(), ww)]
    goal = pb.goal.ravel()
    ns = H * ny * nx

    @functools.lru_cache(maxsize=None)
    def clear(s, m):
        if c["obst"]["n"] == 0:
            return np.ones(ns, bool)
        (sep, _), _ = _flags(c, sol, s, moves[m][0])
        return ~(sep < F64(o["dyn_clearance"])).any(axis=(1, 2))

    h = np.full((Sn + 1, ns), np.inf, F32)
    heap = []
    for s in range(Sn + 1):
        for p in np.flatnonzero(goal):
            h[s, p] = 0
            heap.append((0.0, s, int(p)))
    heapq.heapify(heap)
    while heap:
        dq, s1, q = heapq.heappop(heap)
        if dq > h[s1, q] or s1 == 0:
            continue
        qi, qj, qh = q % nx, (q // nx) % ny, q // (nx * ny)
        for m, ((dx, dy, dh), e, w) in enumerate(moves):
            i, j, hh = qi - dx, qj - dy, (qh - dh) % H
            if not (0 <= i < nx and 0 <= j < ny):
                continue
            p = (hh * ny + j) * nx + i
            if goal[p] or not e[p] or not clear(s1 - 1, m)[p]:
                continue
            nd = F32(h[s1, q] + w[p])
            if nd < h[s1 - 1, p]:
                h[s1 - 1, p] = nd
                heapq.heappush(heap, (float(nd), s1 - 1, p))
    return h


def test_solve_equals_dijkstra_on_the_explicit_graph():
    sc = pplan_cases.shape_scene(12, 10)
    ob = obst_ref.make(2, [[0.1, 1.0], [0.5, 1.6], [-0.2, 1.3]], [[0.3, 0.1], [-0.2, -0.3], [0.0, 0.0]], [0.04, 0.03, 0.05], epoch=0.5, step=0.1)
    goals = np.array([(-0.1, 0.9, -1), (0.6, 1.4, 2), (-0.9, 0.7, -1)], F32)
    wide = dict(name="wide", sc=sc, H=8, moves="any", body=pplan_cases.footprint(3), goals=goals, obst=ob, t_begin=0.75,
                opts=dict(tp.default_opts(0.1, 8), horizon=12, slot=0.2, dyn_clearance=0.03, margin=0.1, turn=0.05))
    for c in (tc.small_case("cross"), dict(wide, moves="forward"), wide):
        sol = tc.ref_solve(c)
        h = _dijkstra(c, sol)
        assert np.array_equal(h.view(np.uint32), sol["cost_all"].view(np.uint32)), c["name"]
        assert np.isfinite(h[0]).sum() > 50
        print("%s %s: %d of %d states finite, equal to the Dijkstra" % (c["name"], c["moves"], np.isfinite(h).sum(), h.size))


@pytest.mark.parametrize("S", (6, 14, 40))
def test_no_balls_is_the_pose_planner_within_the_horizon(S):
    c = dict(tc.shape_case("d"), obst=tc.NO_BALLS, goals=pplan_cases.shape_goals(9, 17, 32))
    c["opts"] = dict(c["opts"], horizon=S)
    sol = tc.ref_solve(c)
    pb = sol["pb"]
    H, ny, nx = pb.n3
    cost = pplan_ref.solve_dijkstra(pb)
    pol = pplan_ref.policy(pb, cost)
    moves = np.full(cost.size, -1, np.int64)             # the length of the static policy walk
    for p in np.argsort(cost, kind="stable"):
        if np.isfinite(cost[p]):
            if pol[p] == pplan_ref.STAY:
                moves[p] = 0
            else:
                dx, dy, dh = pplan_ref.move_of(int(pol[p]))
                h, r = divmod(p, nx * ny)
                moves[p] = moves[((h + dh) % H) * nx * ny + r + dy * nx + dx] + 1
    near = (moves >= 0) & (moves <= S)
    assert np.array_equal(sol["cost0"][near].view(np.uint32), cost[near].view(np.uint32))
    far = np.isfinite(sol["cost0"]) & ~near
    print("S %d: %d states within the horizon equal pplan_ref bit for bit, %d beyond it finite, %d +inf" % (
        S, near.sum(), far.sum(), (~np.isfinite(sol["cost0"])).sum()))
    assert near.sum() > (100 if S == 6 else 1000) and (S != 6 or far.sum() + (~np.isfinite(sol["cost0"]) & np.isfinite(cost)).sum() > 100)
    if S == 40:
        assert not far.any() and np.array_equal(np.isfinite(sol["cost0"]), np.isfinite(cost))


def _point_case():
    """The time planner's own shape case "b" (31 x 33, S = 7, one ball) with diagonals, as the pose lattice's moves "any" has them,
    and margin 0: the body rule samples the field bilinearly, and at a lattice point its float32 value differs from dist[p] in
    the last bits, which a margin would carry into c (without one c is 0 or 1 at both planners)."""
    c = tplan_cases.shape_case("b")
    return dict(c, opts=dict(c["opts"], connectivity=1, margin=0.0))


def test_one_ball_zero_footprint_is_the_time_planner_at_every_heading():
    c = _point_case()
    sc = c["sc"]
    for H in (8, 16):
        o = c["opts"]
        po = dict(tp.default_opts(sc["step"], H), clearance=o["clearance"], margin=o["margin"], gain=o["gain"], slot=o["slot"],
                  horizon=o["horizon"], dyn_clearance=o["dyn_clearance"], wait=o["wait"], turn=0.05)
        sol = tp.solve(sc["dist"], sc["shape"], sc["origin"], sc["step"], body_ref.point(2), pplan_ref.heading_table(H),
                       pplan_ref.heading_moves(H, "any"), tc.poses(c["goals"]), c["obst"], c["t_begin"], po)
        ref = tplan_ref.solve(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["goals"], c["obst"], c["t_begin"], o)
        got = sol["cost0"].reshape(H, -1)
        assert np.array_equal(sol["c"].reshape(H, -1), np.broadcast_to(ref["c"], (H, ref["c"].size)))
        assert np.isfinite(ref["cost0"]).sum() > 100 and (~np.isfinite(ref["cost0"])).sum() > 10
        for h in range(H):
            assert np.array_equal(got[h].view(np.uint32), ref["cost0"].view(np.uint32)), h


def test_every_branch_is_met():
    got = {n: _small(n) for n in tc.SMALL}
    pa = {n: g[2] for n, g in got.items()}
    tr = {n: g[3] for n, g in got.items()}
    assert pa["plain"]["status"][0] == 0 and pa["plain"]["arrive"][0] == 7 and tp.waits(pa["plain"], 0) == 0 and tp.turns(pa["plain"], 0) == 0
    # a wait chosen
    assert pa["cross"]["status"][0] == 0 and tp.waits(pa["cross"], 0) >= 1 and tr["cross"]["wait"] >= 1 and tr["cross"]["ball_blocked"] >= 1
    assert tr["plain"].get("ball_blocked", 0) == 0
    # a turn chosen because a ball closes the translation at heading h but not at h +- 1
    assert tr["side"]["turn_for_ball"] >= 1 and tp.turns(pa["side"], 0) >= 2 and pa["side"]["status"][0] == 0
    # a translation closed by a rear body ball alone, with the reference point clear
    assert tr["rear"]["rear_alone"] >= 1
    # a turn closed by a ball the held pose clears at both ends: the route turns the other way round
    assert tr["turn"]["turn_swept"] >= 1 and pa["turn"]["status"][0] == 0
    assert [int(h) for h in pa["turn"]["cells"][0][:5, 2]] == [4, 3, 2, 1, 0]
    # a tunnelling ball found between two clear samples
    assert tr["tunnel"]["tunnel"] >= 1 and tp.waits(pa["tunnel"], 0) == 1 and pa["tunnel"]["arrive"][0] == 8
    # a start the horizon cannot serve, a ball over the start at slot 0, NaN separations, a start with h = -1
    assert pa["short"]["status"][0] == 3 and pa["on_start"]["status"][0] == 3
    assert tr["nan"]["nan_sep"] > 0 and pa["nan"]["arrive"][0] == 7
    assert tr["any_heading"]["any_heading"] == 1 and pa["any_heading"]["heading"][0] == 0
    # ties by h[s+1] and by the order offered
    assert tr["plain"]["tie_q"] > 0 and tr["plain"]["tie_code"] > 0 and tr["cross"]["tie_code"] > 0
    print({n: (int(pa[n]["status"][0]), int(pa[n]["arrive"][0])) for n in tc.SMALL})
    print({n: tr[n] for n in ("cross", "side", "rear", "turn", "tunnel")})


def test_defective_variants_each_rejected_by_a_named_case():
    def run(name, variant, **kw):
        c = tc.small_case(name)
        c["opts"].update(kw)
        sol = tc.ref_solve(c, variant=variant)
        pa = tp.paths(sol, c["starts"])
        good = tc.ref_solve(c) if kw else _small(name)[1]
        return c, sol, pa, good, tp.check(good, pa, c["obst"])       # (the variant's route under the contract's check)

    # each variant's route fails the contract's certificate where the contract's own passes
    for variant, name in (("no_rho", "cross"), ("centre_only", "cross"), ("turn_hold", "turn"), ("sample_only", "tunnel"), ("slot_off", "cross")):
        c, sol, pa, good, ck = run(name, variant)
        assert not np.array_equal(sol["policy"], good["policy"]), (variant, name)
        assert pa["status"][0] == 0 and ck["collides"][0] == 1 and ck["min_sep"][0] < good["opts"]["dyn_clearance"], (variant, name, ck)
        own = tp.check(good, _small(name)[2], c["obst"])
        assert own["collides"][0] == 0 and own["min_sep"][0] >= good["opts"]["dyn_clearance"]
        print(variant, name, "min_sep %.4f against %.4f" % (ck["min_sep"][0], own["min_sep"][0]))
    assert [int(h) for h in run("turn", "turn_hold")[2]["cells"][0][:5, 2]] == [4, 5, 6, 7, 0]      # through the ball
    # wait 1.0 makes a wait weigh what a step along the row weighs: equal costs, and the order offered decides the policy
    c, first, pa, paced, ck = run("cross", "wait_first", wait=1.0)
    assert np.array_equal(first["cost_all"].view(np.uint32), paced["cost_all"].view(np.uint32))
    assert not np.array_equal(first["policy"], paced["policy"])
    assert (first["policy"] == tp.WAIT).sum() > (paced["policy"] == tp.WAIT).sum()


def _certify(c, sol, pa):
    """Both certificates of every status-0 path: the check with the solve's set, footprint and dyn_clearance; and every (point,
    heading) visited has c > 0 and the body rule's D there gives (float)D >= clearance."""
    ck = tp.check(sol, pa, c["obst"])
    ok = pa["status"] == 0
    assert not ck["collides"][ok].any() and (ck["first_hit"][ok] == -1).all()
    if c["obst"]["n"]:
        assert (ck["min_sep"][ok & (pa["arrive"] > 0)] >= sol["opts"]["dyn_clearance"]).all()
    pb, sc = sol["pb"], c["sc"]
    H, ny, nx = pb.n3
    cells = np.concatenate([pa["cells"][r] for r in np.flatnonzero(ok)]) if ok.any() else np.zeros((0, 3), np.int64)
    if cells.size:
        idx = (cells[:, 2] * ny + cells[:, 1]) * nx + cells[:, 0]
        assert (sol["c"][idx] > 0).all()
        pts = pb.world(cells[:, :2]).astype(F64)
        states = np.concatenate([pts, sol["headings"][cells[:, 2]]], axis=1)
        D = body_ref.clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["body"], states, sol["opts"]["clearance"])["D"]
        assert (D.astype(F32) >= F32(sol["opts"]["clearance"])).all()
    return ck


def test_both_certificates_on_every_status0_path_of_every_case():
    for n in tc.SMALL:
        c, sol, pa, _ = _small(n)
        _certify(c, sol, pa)
    for n in sorted(tc.SHAPES):
        c, sol, pa = _shape(n)
        ck = _certify(c, sol, pa)
        share = sol["finite0"] / max(sol["free"], 1)
        fin = np.isfinite(ck["min_sep"])
        print("%s: finite at slot 0 on %.2f of %d free states, statuses %s, least min_sep %s" % (
            n, share, sol["free"], np.bincount(pa["status"], minlength=4).tolist(), ck["min_sep"][fin].min() if fin.any() else None))
        assert share > 0 and (pa["status"] == 0).any()
    c, sol, pa = _demo()
    _certify(c, sol, pa)


def test_controls_are_the_time_planners_stage_on_the_paths_points():
    c, sol, pa, _ = _small("side")
    A = int(pa["arrive"][0])
    p = pa["points"].astype(F64)
    for T, k0 in ((1, 0), (8, 3), (64, 0), (16, A + 5)):
        got = tp.controls(sol, pa, T, k0, 0.7)
        pos = p[np.minimum(k0 + np.arange(T + 1), A)]
        U, h0, cl = retime_ref.controls_of_positions(pos, sol["opts"]["slot"], 0.7, 1e-9)
        assert np.array_equal(got["U"][0], U) and np.array_equal(got["heading0"][0], h0) and got["clamped"][0] == cl
        assert np.array_equal(got["p0"][0], pos[0])
    # a turn on the spot is a step of zero speed, as a wait is
    U = tp.controls(sol, pa, A, 0)["U"][0]
    cells = pa["cells"][0]
    still = (cells[1:, :2] == cells[:-1, :2]).all(axis=1)
    assert still.sum() >= 2 and (U[still, 0] == 0).all() and (U[~still, 0] > 0).all()
    c, sol, pa, _ = _small("short")
    got = tp.controls(sol, pa, 4)
    assert not got["U"].any() and np.array_equal(got["p0"][0], c["starts"][0, :2].astype(F64)) and tuple(got["heading0"][0]) == (1.0, 0.0)


def test_a_parked_disc_the_point_planners_fail_and_the_time_pose_planner_passes():
    c, sol, pa = _demo()
    ck = _certify(c, sol, pa)
    assert pa["status"][0] == 0 and ck["collides"][0] == 0 and ck["min_sep"][0] >= tc.DEMO["dyn_clearance"]
    # the inscribed radius: a route certified for the point that drives the body into the disc
    s_in, p_in = tc.demo_point(tc.R_IN)
    own = tplan_ref.check(s_in, p_in, c["obst"])
    assert p_in["status"][0] == 0 and own["collides"][0] == 0 and own["min_sep"][0] >= tc.DEMO["dyn_clearance"] + tc.R_IN
    body = tp.check(sol, tc.point_route_as_poses(p_in, tc.DEMO["H"]), c["obst"])
    assert body["collides"][0] == 1 and body["min_sep"][0] < -0.1
    # the circumscribed radius: the start is free, and no arrival
    s_out, p_out = tc.demo_point(tc.R_OUT)
    assert p_out["status"][0] == 3 and p_out["arrive"][0] == -1
    print("time-pose plan: status %d, arrive %d, waits %d, turns %d, cost %.4f, min_sep %.4f against %.2f" % (
        pa["status"][0], pa["arrive"][0], tp.waits(pa, 0), tp.turns(pa, 0), pa["start_cost"][0], ck["min_sep"][0], tc.DEMO["dyn_clearance"]))
    print("point, inscribed radius %.3f: status %d, arrive %d, waits %d, its own min_sep %.4f, the body's min_sep %.4f (ball %d, slot %d)" % (
        tc.R_IN, p_in["status"][0], p_in["arrive"][0], tplan_ref.waits(p_in, 0), own["min_sep"][0], body["min_sep"][0], body["min_ball"][0],
        body["first_hit"][0]))
    print("point, circumscribed radius %.3f: status %d (no arrival within %d slots)" % (tc.R_OUT, p_out["status"][0], tc.DEMO["horizon"]))
