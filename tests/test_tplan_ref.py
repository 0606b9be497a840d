"""The time planner's reference (tests/tplan_ref.py) against what it must equal without a device: the library's symbols, defaults
and refusals; a heapq Dijkstra on the explicit time-expanded graph whose clearance flags come from retime_ref.sep itself; the
static planner with no balls; a trace of every branch; defective variants; the certificate; the control stage; and the
comparison with the re-timing on the Z corridor (a parked disc that waiting cannot pass, a crossing disc that it can)."""
import ctypes as C
import functools
import heapq
import os
import re

import numpy as np
import pytest

import gpismap_amd
import obst_ref
import plan_ref
import pplan_cases
import retime_ref
import timing_ref
import tplan_cases as tc
import tplan_ref as tr
import traj_ref

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_tplan_default_opts", "gpis_tplan_check_opts", "gpis_tplan_create", "gpis_tplan_destroy", "gpis_tplan_solve",
         "gpis_tplan_info", "gpis_tplan_get", "gpis_tplan_device", "gpis_tplan_paths", "gpis_tplan_path_counts", "gpis_tplan_get_paths",
         "gpis_tplan_check", "gpis_tplan_controls", "gpis_tplan_set_schedule"}


@functools.lru_cache(maxsize=None)
def _small(name):
    """(case, solution, paths, trace) of a small case by the contract: computed once, left unchanged."""
    c = tc.small_case(name)
    trace = {}
    sol = tc.ref_solve(c, trace=trace)
    return c, sol, tr.paths(sol, c["starts"]), trace


@functools.lru_cache(maxsize=None)
def _z(kind, speed=0.3):
    c = tc.z_case(kind, speed)
    sol = tc.ref_solve(c)
    return c, sol, tr.paths(sol, c["starts"])


def test_symbols_defaults_and_refusals():
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    assert set(re.findall(r"\b(gpis_tplan[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_tplan_default_opts.argtypes = [C.c_float, C.POINTER(gpismap_amd.gpis_tplan_opts)]
    for step in (0.25, 0.1, 0.2):
        o = gpismap_amd.gpis_tplan_opts()
        assert L.gpis_tplan_default_opts(step, C.byref(o)) == 0
        got = {k: getattr(o, k) for k in tr.OPT_KEYS}
        ref = tr.default_opts(step)
        assert all(F32(got[k]) == F32(ref[k]) for k in ("clearance", "margin", "gain", "wait")), (got, ref)
        assert all(got[k] == ref[k] for k in ("connectivity", "slot", "horizon", "dyn_clearance", "keep_cost")), (got, ref)
    assert (o.slot, o.horizon, o.wait, o.keep_cost, o.connectivity, o.gain, o.clearance) == (0.1, 256, 0.5, 0, 1, 4.0, 0.0)
    assert L.gpis_tplan_default_opts(0.0, C.byref(o)) == -1 and L.gpis_tplan_default_opts(0.1, None) == -1
    assert L.gpis_tplan_default_opts(float("nan"), C.byref(o)) == -1
    p = gpismap_amd.tplan_opts(0.25, slot=0.5, wait=2.0, horizon=9)
    assert (p.slot, p.wait, p.horizon, p.dyn_clearance) == (0.5, 2.0, 9, 0.25)
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.tplan_opts(0.25, pause=1.0)
    # a plan lives on a handle, which lives on a device: without one the entries answer GPIS_ERR_ARG
    d, vp = C.c_double, C.c_void_p
    L.gpis_tplan_solve.argtypes = [vp, vp, vp, vp, C.c_int, d, vp, vp]
    L.gpis_tplan_check.argtypes = [vp, vp, d] + [vp] * 5
    L.gpis_tplan_controls.argtypes = [vp, C.c_int, C.c_int, d, d] + [vp] * 4
    L.gpis_tplan_get.argtypes = [vp] * 5
    L.gpis_tplan_paths.argtypes = [vp, vp, C.c_int, vp]
    assert L.gpis_tplan_solve(None, None, None, None, 1, 0.0, C.byref(o), None) == -1
    assert L.gpis_tplan_check(None, None, 0.1, None, None, None, None, None) == -1
    assert L.gpis_tplan_controls(None, 4, 0, 0.0, 0.0, None, None, None, None) == -1
    assert L.gpis_tplan_get(None, None, None, None, None) == -1 and L.gpis_tplan_paths(None, None, 1, None) == -1


BAD = (dict(slot=0.0), dict(slot=-1.0), dict(slot=float("nan")), dict(slot=float("inf")), dict(horizon=0), dict(horizon=1025),
       dict(dyn_clearance=-0.1), dict(dyn_clearance=float("nan")), dict(wait=-0.5), dict(wait=1.5e4), dict(wait=float("nan")),
       dict(keep_cost=2), dict(keep_cost=-1), dict(connectivity=2), dict(margin=-0.1), dict(gain=-1.0), dict(gain=2e4),
       dict(clearance=float("inf")), dict(margin=float("nan")))
GOOD = (dict(), dict(horizon=1), dict(horizon=1024), dict(wait=0.0), dict(wait=1e4), dict(dyn_clearance=0.0), dict(keep_cost=1),
        dict(connectivity=0), dict(clearance=-0.3), dict(margin=0.0), dict(gain=1e4))


def test_every_option_is_refused_alike():
    L = gpismap_amd.lib()
    for kw, ok in [(k, False) for k in BAD] + [(k, True) for k in GOOD]:
        o = dict(tr.default_opts(0.1), **kw)
        rc = L.gpis_tplan_check_opts(C.byref(gpismap_amd.tplan_opts(0.1, **kw)), 0, 0)
        assert rc == (0 if ok else -1), (kw, rc)
        if ok:
            tr.check_opts(o)
        else:
            with pytest.raises(ValueError):
                tr.check_opts(o)
    # the sizes: nx ny (S + 1) <= 2^30, 2^28 with keep_cost
    for shape, kw, ok in (((1024, 1023), dict(horizon=1024), True), ((1024, 1024), dict(horizon=1024), False),
                          ((1024, 1024), dict(horizon=1023), True), ((512, 512), dict(horizon=1023, keep_cost=1), True),
                          ((512, 513), dict(horizon=1023, keep_cost=1), False)):
        rc = L.gpis_tplan_check_opts(C.byref(gpismap_amd.tplan_opts(0.1, **kw)), *shape)
        assert rc == (0 if ok else -4), (shape, kw, rc)
        if ok:
            tr.check_opts(dict(tr.default_opts(0.1), **kw), shape)
        else:
            with pytest.raises(OverflowError):
                tr.check_opts(dict(tr.default_opts(0.1), **kw), shape)


def test_sep_s_is_retime_sep_bit_for_bit():
    rng = np.random.default_rng(5)
    S = tc.shape_balls(pplan_cases.shape_scene(17, 23), 9, 3)
    TB, slot = F64(1.25) - F64(S["epoch"]), 0.2
    for _ in range(40):
        p0, dp = rng.uniform(-1, 3, 2), rng.uniform(-0.1, 0.1, 2) * rng.integers(0, 2)
        k = rng.integers(0, 1000, 5)
        ref = retime_ref.sep(p0, dp, k, S, TB, slot)
        got, s = tr.sep_s(np.broadcast_to(p0, (5, 2)), np.broadcast_to(dp, (5, 2)), TB + k.astype(F64) * F64(slot),
                          TB + (k + 1).astype(F64) * F64(slot), S)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)) and ((s >= 0) & (s <= 1)).all()


def _dijkstra(c, sol):
    """h [S + 1, np] of the explicit time-expanded graph: a backward heapq Dijkstra from every (s, goal) with the same float32
    additions; a move's clearance flag comes from retime_ref.sep, one interval at a time."""
    pb, o, S = sol["pb"], sol["opts"], c["obst"]
    nx, ny = pb.shape
    H = int(o["horizon"])
    TB = F64(c["t_begin"]) - F64(S["epoch"])
    px, py = tr.axis_points(pb.origin[0], pb.step, nx), tr.axis_points(pb.origin[1], pb.step, ny)
    ww = ((F32(o["wait"]) * pb.step) * pb.c).ravel()
    moves = [(off, e.ravel(), w.ravel()) for k, off, e, w in pb.edges] + [((0, 0, 0), pb.free.ravel(), ww)]
    goal = pb.goal.ravel()

    @functools.lru_cache(maxsize=None)
    def clear(s, i, j, dx, dy):
        if S["n"] == 0:
            return True
        p0 = np.array([px[i + 1], py[j + 1]])
        dp = np.array([px[i + 1 + dx] - px[i + 1], py[j + 1 + dy] - py[j + 1]])
        with np.errstate(all="ignore"):
            return not (retime_ref.sep(p0, dp, np.array([s]), S, TB, o["slot"]) < F64(o["dyn_clearance"])).any()

    h = np.full((H + 1, nx * ny), np.inf, F32)
    heap = []
    for s in range(H + 1):
        for p in np.flatnonzero(goal):
            h[s, p] = 0
            heap.append((0.0, s, int(p)))
    heapq.heapify(heap)
    while heap:
        dq, s1, q = heapq.heappop(heap)
        if dq > h[s1, q] or s1 == 0:
            continue
        qi, qj = q % nx, q // nx
        for (dx, dy, _), e, w in moves:
            i, j = qi - dx, qj - dy
            if not (0 <= i < nx and 0 <= j < ny):
                continue
            p = j * nx + i
            if goal[p] or not e[p] or not clear(s1 - 1, i, j, dx, dy):
                continue
            nd = F32(h[s1, q] + w[p])
            if nd < h[s1 - 1, p]:
                h[s1 - 1, p] = nd
                heapq.heappush(heap, (float(nd), s1 - 1, p))
    return h


def test_solve_equals_dijkstra_on_the_explicit_graph():
    sc = pplan_cases.shape_scene(12, 10)
    ob = obst_ref.make(2, [[0.1, 1.0], [0.5, 1.6], [-0.2, 1.3]], [[0.3, 0.1], [-0.2, -0.3], [0.0, 0.0]], [0.12, 0.08, 0.1], epoch=0.5, step=0.1)
    wide = dict(name="wide", sc=sc, goals=tc.world(sc, [(1, 1), (10, 8), (-3, 0)]), obst=ob, t_begin=0.75,
                opts=dict(tr.default_opts(0.1), horizon=14, slot=0.2, dyn_clearance=0.1, margin=0.2))
    for c in (tc.small_case("plain"), tc.small_case("cross"), wide):
        sol = tc.ref_solve(c)
        h = _dijkstra(c, sol)
        assert np.array_equal(h.view(np.uint32), sol["cost_all"].view(np.uint32)), c["name"]
        print("%s: %d of %d states finite, equal to the Dijkstra" % (c["name"], np.isfinite(h).sum(), h.size))


@pytest.mark.parametrize("S", (58, 78, 84))
def test_no_balls_is_the_static_planner_within_the_horizon(S):
    c = tc.z_case("static")
    c["opts"]["horizon"] = S
    sol = tc.ref_solve(c)
    pb = sol["pb"]
    cost = plan_ref.solve_sweep(pb)
    pol = plan_ref.policy(pb, cost)
    nx = pb.shape[0]
    moves = np.full(cost.size, -1, np.int64)             # the length of the static policy walk
    for p in np.argsort(cost, kind="stable"):
        if np.isfinite(cost[p]):
            if pol[p] == plan_ref.STAY:
                moves[p] = 0
            else:
                dx, dy, _ = plan_ref.offset(int(pol[p]))
                moves[p] = moves[p + dy * nx + dx] + 1
    near = (moves >= 0) & (moves <= S)
    assert np.array_equal(sol["cost0"][near].view(np.uint32), cost[near].view(np.uint32))
    far = np.isfinite(sol["cost0"]) & ~near
    print("S %d: %d points within the horizon equal plan_ref bit for bit, %d beyond it finite, %d +inf" % (
        S, near.sum(), far.sum(), (~np.isfinite(sol["cost0"])).sum()))
    assert near.sum() > 1000
    if S == 84:
        assert not far.any()


def test_every_branch_is_met():
    got = {n: _small(n) for n in tc.SMALL}
    pa = {n: g[2] for n, g in got.items()}
    assert pa["plain"]["status"][0] == 0 and pa["plain"]["arrive"][0] == 8 and tr.waits(pa["plain"], 0) == 0
    # a wait chosen, translations closed by a ball alone
    assert pa["cross"]["status"][0] == 0 and tr.waits(pa["cross"], 0) >= 1 and got["cross"][3]["wait"] >= 1
    assert got["cross"][3]["ball_blocked"] >= 1 and got["plain"][3].get("ball_blocked", 0) == 0
    # a ball that tunnels between two clear samples of a move
    assert tr.waits(pa["tunnel"], 0) == 1 and pa["tunnel"]["arrive"][0] == 9
    # a goal not free, a start on a goal, a start the horizon cannot serve, a ball over the start at slot 0, NaN separations
    assert got["goal_blocked"][1]["goals_kept"] == 0 and pa["goal_blocked"]["status"][0] == 3
    assert pa["at_goal"]["status"][0] == 0 and pa["at_goal"]["arrive"][0] == 0 and len(pa["at_goal"]["cells"][0]) == 1
    assert pa["short"]["status"][0] == 3 and pa["on_start"]["status"][0] == 3
    assert got["nan"][3]["nan_sep"] > 0 and pa["nan"]["arrive"][0] == 8
    # ties by h[s+1][q] and by the order offered
    t = {}
    tc.ref_solve(tc.shape_case("c"), trace=t)
    assert t["tie_q"] > 0 and t["tie_code"] > 0 and t["wait"] > 0
    print({n: (int(pa[n]["status"][0]), int(pa[n]["arrive"][0])) for n in tc.SMALL}, t)


def test_defective_variants_each_change_a_named_case():
    def arrive(name, variant, **kw):
        c = tc.small_case(name)
        c["opts"].update(kw)
        sol = tc.ref_solve(c, variant=variant)
        pa = tr.paths(sol, c["starts"])
        return int(pa["status"][0]), int(pa["arrive"][0]), tr.waits(pa, 0) if pa["status"][0] == 0 else -1, sol

    good = {n: arrive(n, None) for n in ("tunnel", "cross")}
    assert arrive("tunnel", "sample_only")[:3] == (0, 8, 0) != good["tunnel"][:3]          # walks through the ball
    off = arrive("cross", "slot_off")
    assert not np.array_equal(off[3]["policy"], good["cross"][3]["policy"])
    # wait 1.0 makes a wait weigh what a step along the corridor weighs: standing still ties with pacing back and forth, and
    # the order offered decides
    paced, first = arrive("cross", None, wait=1.0), arrive("cross", "wait_first", wait=1.0)
    assert not np.array_equal(first[3]["policy"], paced[3]["policy"])                       # equal-cost ties go to the wait
    assert np.array_equal(first[3]["cost_all"], paced[3]["cost_all"]) and first[2] > paced[2]
    tgt = arrive("tunnel", "target_only")
    assert tgt[:3] == (0, 8, 0)
    # and each variant's route fails the contract's certificate where the contract's own passes
    c = tc.small_case("tunnel")
    for v in ("sample_only", "target_only"):
        sol = tc.ref_solve(c, variant=v)
        assert tr.check(sol, tr.paths(sol, c["starts"]), c["obst"])["collides"][0] == 1, v
    print("tunnel", good["tunnel"][:3], "cross", good["cross"][:3], "slot_off", off[:3], "wait_first", first[:3])


def _certify(c, sol, pa):
    ck = tr.check(sol, pa, c["obst"])
    ok = pa["status"] == 0
    assert not ck["collides"][ok].any() and (ck["first_hit"][ok] == -1).all()
    if c["obst"]["n"]:
        assert (ck["min_sep"][ok & (pa["arrive"] > 0)] >= sol["opts"]["dyn_clearance"]).all()
    return ck


def test_certificate_on_every_status0_path_of_every_case():
    for n in tc.SMALL:
        c, sol, pa, _ = _small(n)
        _certify(c, sol, pa)
    for n in ("a", "b", "c", "d", "e"):
        c = tc.shape_case(n)
        sol = tc.ref_solve(c)
        pa = tr.paths(sol, c["starts"])
        ck = _certify(c, sol, pa)
        share = sol["finite0"] / max(sol["free"], 1)
        print("%s: finite at slot 0 on %.2f of the free points, statuses %s, least min_sep %.4f" % (
            n, share, np.bincount(pa["status"], minlength=4).tolist(), np.nanmin(np.where(np.isfinite(ck["min_sep"]), ck["min_sep"], np.nan))
            if np.isfinite(ck["min_sep"]).any() else np.inf))
        assert share > 0 and (pa["status"] == 0).any()


def test_controls_are_retime_refs_stage_on_the_slots_points():
    c, sol, pa, _ = _small("cross")
    A = int(pa["arrive"][0])
    p = pa["points"].astype(F64)
    for T, k0 in ((1, 0), (8, 3), (64, 0), (16, A + 5)):
        got = tr.controls(sol, pa, T, k0, 0.7)
        pos = p[np.minimum(k0 + np.arange(T + 1), A)]
        U, h0, cl = retime_ref.controls_of_positions(pos, sol["opts"]["slot"], 0.7, 1e-9)
        assert np.array_equal(got["U"][0], U) and np.array_equal(got["heading0"][0], h0) and got["clamped"][0] == cl
        assert np.array_equal(got["p0"][0], pos[0])
    # a wait is a step of zero speed, a move one of step / slot
    U = tr.controls(sol, pa, A, 0)["U"][0]
    still = (pa["cells"][0][1:] == pa["cells"][0][:-1]).all(axis=1)
    assert (U[still, 0] == 0).all() and np.allclose(U[~still, 0], 0.1 / 0.2)
    c, sol, pa, _ = _small("short")
    got = tr.controls(sol, pa, 4)
    assert not got["U"].any() and np.array_equal(got["p0"][0], c["starts"][0].astype(F64)) and tuple(got["heading0"][0]) == (1.0, 0.0)


@functools.lru_cache(maxsize=None)
def _static_timed():
    """The static route of the Z corridor by the references: plan_ref -> traj_ref -> timing_ref."""
    c, sol, pa = _z("static")
    sc, pb = c["sc"], sol["pb"]
    cost = plan_ref.solve_sweep(pb)
    off, pts, _, st = plan_ref.paths(pb, cost, plan_ref.policy(pb, cost), c["starts"], 10 ** 6)
    lat = (sc["dist"], sc["shape"], sc["origin"], sc["step"])
    x0, ist = traj_ref.resample(off, pts, st, 128)
    res = traj_ref.optimize(*lat, x0, ist, dict(traj_ref.default_opts(2, sc["step"]), iters=5, clearance=F32(0.1)))
    tm = timing_ref.time(res["x"], res["status"], timing_ref.default_opts(2, sc["step"]), lat)
    assert st[0] == 0 and tm["status"][0] == 0
    return res["x"], tm, int(off[1]) - 1, float(cost[pplan_cases.lattice_index(sc, sc["start"])])


def test_parked_disc_waiting_fails_and_the_time_plan_goes_round():
    x, tm, moves, cost = _static_timed()
    c0, sol0, pa0 = _z("static")
    assert pa0["arrive"][0] == moves and F32(pa0["start_cost"][0]) == F32(cost)
    t_half = 0.5 * float(tm["t"][0, -1])
    at = timing_ref.position(x[0].astype(F64), tm["v"][0].astype(F64), tm["t"][0].astype(F64), F64(t_half))
    c = tc.z_case("parked", at=at)
    ro = dict(retime_ref.default_opts(2, 0.1), slot=0.2, clearance=0.2, max_pause=255)
    rt = retime_ref.solve(x, tm["v"], tm["t"], tm["status"], c["obst"], 0.0, ro)
    assert rt["status"][0] == 3                                     # waiting cannot pass a parked disc
    sol = tc.ref_solve(c)
    pa = tr.paths(sol, c["starts"])
    ck = _certify(c, sol, pa)
    cells = pa["cells"][0]
    assert pa["status"][0] == 0 and tr.waits(pa, 0) == 0 and pa["arrive"][0] > moves
    assert (cells[:, 1] * 0.1 > 4.5).any()                          # by the bypass above y = 4.5
    print("static route: %d moves, cost %.4f, duration %.2f s; disc parked at (%.2f, %.2f): retime status 3; time plan: %d moves, "
          "cost %.4f, no waits, min_sep %.4f" % (moves, cost, 2 * t_half, at[0], at[1], pa["arrive"][0], pa["start_cost"][0], ck["min_sep"][0]))


@pytest.mark.parametrize("speed", (0.3, 0.1))
def test_crossing_disc_keeps_to_the_corridor_and_waits(speed):
    c, sol, pa = _z("crossing", speed)
    ck = _certify(c, sol, pa)
    cells = pa["cells"][0]
    assert pa["status"][0] == 0 and tr.waits(pa, 0) >= 1
    assert (cells[:, 1] * 0.1 < 4.5).all()                          # never by the bypass
    print("disc crossing at %.1f m/s: %d waits, arrival at slot %d, cost %.4f, closest approach %.4f against 0.2" % (
        speed, tr.waits(pa, 0), pa["arrive"][0], pa["start_cost"][0], ck["min_sep"][0]))
