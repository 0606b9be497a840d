"""CPU tests of the body smoother's contract (tests/traj_body_ref.py): the public surface is declared and
exported, the reference reduces to §7i's with the zero footprint, its fused body result is body_ref.traj_clearance's, the cases
of the device tests reach every branch, the defective variants are told apart by bits, and -- the reference alone -- the chosen
defaults carry the 1.0 x 0.4 robot through the 0.7 door where no point clearance does."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import body_cases as bc
import body_ref
import pplan_cases
import pplan_ref
import traj_body_cases as tbc
import traj_body_ref as tb
import traj_cases
import traj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
POINT_KEYS = ("x", "status", "iterations", "length", "smooth", "obstacle", "min_dist", "nonfinite", "collides")
BODY_KEYS = ("D_min", "waypoint", "ball", "body_collides")
NEW_SYMBOLS = ("gpis_smooth_body_optimize", "gpis_smooth_body_default_opts", "gpis_smooth_body_get", "gpis_smooth_from_pose_paths")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U32) if a.dtype == F32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _same(a, b, keys):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


@functools.lru_cache(maxsize=None)
def _dists():
    return tbc.ref_dists()


def _run(c, variant=None, trace=None, **kw):
    f = tbc.fields()[c["scene"]]
    return tb.optimize(_dists()[c["scene"]], f["shape"], f["origin"], f["step"], c["body"], c["x"], None, dict(c["opts"], **kw), c["w_turn"],
                       variant=variant, trace=trace)


def test_new_symbols_are_declared_exported_and_wrapped():
    import gpismap_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpismap_amd.h")).read(), flags=re.S)
    L = C.CDLL(gpismap_amd.LIB_PATH)         # loads without a GPU
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(L, n), n
    for n in ("from_pose_paths", "body_result"):
        assert callable(getattr(gpismap_amd.Trajectories, n))
    assert callable(gpismap_amd.PosePlanner.trajectories) and callable(gpismap_amd.traj_body_opts)
    # the defaults: the point's, with w_obs shared among the balls; gpis_traj_opts keeps its layout
    L.gpis_smooth_body_default_opts.argtypes = [C.c_int, C.c_float, C.c_int, C.POINTER(gpismap_amd.gpis_traj_opts), C.POINTER(C.c_float)]
    for dim, step, balls in ((2, 0.1, 5), (3, 0.2, 1), (2, 0.25, 16)):
        o, wt = gpismap_amd.gpis_traj_opts(), C.c_float(7)
        assert L.gpis_smooth_body_default_opts(dim, step, balls, C.byref(o), C.byref(wt)) == 0
        ref, rwt = tb.default_opts(dim, F32(step), balls)
        assert all(F32(getattr(o, k)) == F32(ref[k]) for k in traj_ref.OPT_NAMES) and wt.value == rwt == 1
    o = gpismap_amd.gpis_traj_opts()
    assert L.gpis_smooth_body_default_opts(2, 0.1, 0, C.byref(o), None) == -1 and L.gpis_smooth_body_default_opts(2, 0.1, 17, C.byref(o), None) == -1


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("w_turn", [0, 1])
def test_zero_footprint_has_the_point_optimisers_bits(dim, w_turn):
    sc = traj_cases.scene(dim)
    dist = _dists()["balls%d" % dim]
    x, o, names = traj_cases.hand_made(sc, dist, 33)
    o = dict(o, iters=25)
    a = traj_ref.optimize(dist, sc["shape"], sc["origin"], sc["step"], x, None, o)
    b = tb.optimize(dist, sc["shape"], sc["origin"], sc["step"], body_ref.point(dim), x, None, dict(o, w_obs=traj_ref.default_opts(dim, sc["step"])["w_obs"]), w_turn)
    assert _same(a, b, POINT_KEYS)
    assert set(a["status"].tolist()) == {0, 1, 2} and a["iterations"].max() == 25
    # the defaults for one ball are the point's
    assert tb.default_opts(dim, sc["step"], 1)[0] == traj_ref.default_opts(dim, sc["step"])


def test_fused_body_result_is_the_trajectory_check_on_the_result():
    saw = dict(off=0, all_off=0, status2=0, collides=0, free=0)
    for c in tbc.all_cases(_dists()):
        if "N64" not in c["name"] and "N3_" not in c["name"] and not c["name"].startswith(("leaving", "repeated", "door_mix")):
            continue
        f = tbc.fields()[c["scene"]]
        r = _run(c)
        ref = body_ref.traj_clearance(_dists()[c["scene"]], f["shape"], f["origin"], f["step"], c["body"], r["x"], r["status"], float(F32(r_opts(c)["clearance"])))
        got = dict(D_min=r["D_min"], waypoint=r["waypoint"], ball=r["ball"], collides=r["body_collides"])
        assert _same(got, ref, ("D_min", "waypoint", "ball", "collides")), c["name"]
        saw["status2"] += int((r["status"] == 2).sum())
        saw["all_off"] += int(((r["status"] != 2) & np.isnan(r["D_min"])).sum())
        saw["collides"] += int(r["body_collides"].sum())
        saw["free"] += int(((r["status"] != 2) & (r["body_collides"] == 0)).sum())
        saw["off"] += int(((r["body_collides"] == 1) & (r["D_min"] >= float(F32(r_opts(c)["clearance"])))).sum())
    assert all(v > 0 for v in saw.values()), saw


def r_opts(c):
    f = tbc.fields()[c["scene"]]
    o, _ = tb.default_opts(len(f["shape"]), f["step"], c["body"]["m"])
    o.update(c["opts"])
    return o


def test_cases_reach_every_branch():
    tot = {k: 0 for k in tb.TRACE_KEYS}
    stops = set()
    for c in tbc.all_cases(_dists()) + [tbc.batch_case(_dists()["balls2"])]:
        tr = {}
        r = _run(c, trace=tr)
        for k in tb.TRACE_KEYS:
            tot[k] += int(tr[k].sum())
        if c["name"] == "door_mix":
            stops = set(r["iterations"].tolist())
            assert r["status"].tolist()[3] == 2 and len(stops) >= 4, r["iterations"]
    assert all(v > 0 for v in tot.values()), tot


def test_defective_variants_differ_by_bits():
    cases = {c["name"]: c for c in tbc.all_cases(_dists())}
    pick = [cases[n] for n in ("hand2_N64_sixteen_w1", "hand3_N64_asym_w1", "hand2_N4_two_w1", "door_N32", "door_N128")]
    base = [_run(c, iters=8) for c in pick]
    for v in tb.VARIANTS:
        differs = [not _same(_run(c, variant=v, iters=8), b, ("x",)) for c, b in zip(pick, base)]
        assert any(differs), v
        if v not in ("last_alone", "q_double"):              # (a double q differs where e - margin rounds: the door, clearance 0)
            assert sum(differs) >= 2, (v, differs)
    c = pick[0]
    assert not _same(base[0], _run(dict(c, w_turn=F32(0)), iters=8), ("x",))          # (w_turn is not inert)


def test_overflowing_step_keeps_its_nan_and_status_1():
    sc = traj_cases.scene(2)
    dist = _dists()["balls2"]
    x, o, names = traj_cases.hand_made(sc, dist, 16)
    r = tb.optimize(dist, sc["shape"], sc["origin"], sc["step"], bc.traj_body(2), x[:6], None, dict(o, iters=3, w_smooth=F32(3e38), rate=F32(3e38)), 1)
    assert np.all(r["status"][1:] == 1) and np.all(r["iterations"][1:] == 3) and not np.isfinite(r["x"][1:, 1:-1]).all()


# ---- resampling of pose paths ------------------------------------------------------------------------------------------------
def test_pose_paths_with_turns_in_place_resample_with_w_zero():
    off, pts, hd, st = tbc.turn_paths_ref()
    tbc.check_turn_paths(off, pts, st)
    for N in (3, 5, 64):
        x, ist = tb.resample(off, pts, st, N)
        with np.errstate(all="ignore"):
            old, ost = traj_ref.resample(off, pts, st, N)
        assert np.array_equal(ist, ost) and ist.tolist() == [0, 0, 0, 0, 2]
        for k in tbc.TURN_ENDS + (tbc.TURN_POINT,):                               # a path that ends in a turn keeps §7i's bits
            assert np.array_equal(x[k].view(U32), old[k].view(U32)) and np.isfinite(x[k]).all()
        only = pts[off[tbc.TURN_ONLY]]
        assert np.all(x[tbc.TURN_ONLY] == only) and np.isnan(old[tbc.TURN_ONLY][1:-1]).all()      # 0 / 0 under §7i's rule
        assert np.isnan(x[tbc.TURN_NONE]).all()
    # a turn inside a path is skipped by the search: the waypoints are those of the path without the repeated points
    q = pts[off[3]:off[4]]
    keep = np.concatenate([[True], np.abs(np.diff(q, axis=0)).sum(axis=1) > 0])
    assert keep.sum() < len(q)
    assert np.array_equal(tb.resample_one(q, 33).view(U32), traj_ref.resample_one(q[keep], 33).view(U32))
    # Planner paths (no repeated points): the rule changes nothing
    sc = traj_cases.scene(2)
    _, _, _, poff, ppts, _, pst = traj_cases.plan(sc, _dists()["balls2"])
    for p in np.flatnonzero(pst == 0)[:8]:
        assert np.array_equal(tb.resample_one(ppts[poff[p]:poff[p + 1]], 64).view(U32), traj_ref.resample_one(ppts[poff[p]:poff[p + 1]], 64).view(U32))


# ---- geometry: the reference alone -----------------------------------------------------------------------------------------------
def _clear(sc, robot, x, status):
    return body_ref.traj_clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], robot, x, status, 0.0)


@pytest.mark.parametrize("N", tbc.DOOR_NS)
def test_door_polyline_defaults_clear_the_body_where_the_point_smoother_collides(N, capsys):
    sc = bc.door_scene()
    robot = pplan_cases.robot()
    x = traj_ref.resample_one(tbc.DOOR_POLYLINE, N)[None]
    r = tb.optimize(sc["dist"], sc["shape"], sc["origin"], sc["step"], robot, x)
    p = traj_ref.optimize(sc["dist"], sc["shape"], sc["origin"], sc["step"], x, None, dict(clearance=bc.R_IN))
    d_in, d_pt = _clear(sc, robot, x, [0])["D_min"][0], _clear(sc, robot, p["x"], p["status"])["D_min"][0]
    with capsys.disabled():
        print("\n[door N=%d] body D_min: input %+.4f, point smoother (clearance %.1f) %+.4f, body smoother %+.4f; length %.4f, largest bend %.5f, "
              "status %d after %d iterations" % (N, d_in, bc.R_IN, d_pt, r["D_min"][0], r["length"][0], traj_ref.max_bend(r["x"])[0], r["status"][0],
                                                 r["iterations"][0]))
    assert d_in < 0 and d_pt < 0
    assert r["D_min"][0] >= 0 and r["body_collides"][0] == 0


def test_pose_planned_door_routes_stay_clear_after_smoothing(capsys):
    """Pose routes through the door from a handful of starts, resampled by the pose-path rule and smoothed for the body with the
    defaults: every start that has a pose path is counted, and at least half of the starts must have one."""
    sc, pb, cost, pol, _ = pplan_cases.solved("door", 16)
    robot = pplan_cases.robot()
    starts = np.array([(3.4, 4.6, -1), (2.0, 3.0, -1), (1.0, 1.0, -1), (3.0, 5.5, -1), (2.5, 0.8, -1), (0.5, 3.0, -1)], F32)
    off, pts, hd, _, st = pplan_ref.paths(pb, cost, pol, starts, cost.size)
    have = st == 0
    assert 2 * have.sum() >= len(starts), st
    x, ist = tb.resample(off, pts, st, 64)
    r = tb.optimize(sc["dist"], sc["shape"], sc["origin"], sc["step"], robot, x, ist)
    p = traj_ref.optimize(sc["dist"], sc["shape"], sc["origin"], sc["step"], x, ist, dict(clearance=bc.R_IN))
    d_pt = _clear(sc, robot, p["x"], p["status"])["D_min"]
    with capsys.disabled():
        print("\n[door pose routes] body D_min after the body smoother %s, after the point smoother %s; lengths %s; largest bends %s"
              % (np.round(r["D_min"], 4), np.round(d_pt, 4), np.round(r["length"], 3), np.round(traj_ref.max_bend(r["x"]), 4)))
    assert np.all(r["D_min"][have] >= 0) and not r["body_collides"][have].any()
    assert (d_pt[have] < 0).any()
