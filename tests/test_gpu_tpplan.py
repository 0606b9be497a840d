"""The time-pose planner on the GPU (csrc/tpplan.hip, gpis_tpplan_*) against the numpy reference (tests/tpplan_ref.py) on the shared
cases (tests/tpplan_cases.py).  Every field comes from DistanceField.from_grid and the reference runs on the device's own dist.
Every output is compared exactly: the bits of cost0, c and cost_all, every policy byte of every layer, the paths' offsets,
points, heading indices, arrivals, start costs and statuses, the check's two doubles as bits (a NaN equals a NaN) with its four
integers, and U, heading0, p0 as bits with clamped -- with the broad phase off and on, which the results must not depend on."""
import ctypes as C

import numpy as np
import pytest

import body_ref
import obst_ref
import pplan_cases
import tplan_cases
import tpplan_cases as tc
import tpplan_ref as tr
from test_gpu_body import device_body
from test_gpu_obst import device_set
from test_gpu_plan import _dev, _field

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U32 = np.uint32
U64 = np.uint64
_REF = {}


def _status_of(err):
    return int(str(err.value).rsplit(" ", 1)[1])


def _case_field(c, df=None):
    sc = c["sc"]
    return _field(sc["f"], sc["shape"], sc["origin"], sc["step"], df=df)


def _ref(c, dist):
    """(solution, paths) of the reference on the device's own dist: computed once per case, left unchanged."""
    key = (c["name"], dist.tobytes())
    if key not in _REF:
        sol = tc.ref_solve(c, dist)
        _REF[key] = (sol, tr.paths(sol, c["starts"]))
    return _REF[key]


def _solve(c, df, tp=None, cull=None, stream=0, ob=None, fp=None):
    import gpismap_amd
    tp = tp if tp is not None else gpismap_amd.TimePosePlanner()
    if cull is not None:
        tp.set_schedule(cull)
    ob = ob if ob is not None else device_set(c["obst"], c["sc"]["step"])
    fp = fp if fp is not None else device_body(c["body"])
    if stream == 0:
        assert df.plan_poses_timed(c["goals"], fp, ob, H=c["H"], moves=c["moves"], t_begin=c["t_begin"], time_pose_planner=tp, **c["opts"]) is tp
    else:
        assert tp.solve(df, c["goals"], fp, ob, H=c["H"], moves=c["moves"], t_begin=c["t_begin"], stream=stream, **c["opts"]) is tp
    return tp, ob, fp


def _plan_equal(tp, sol, what):
    keep = bool(sol["opts"]["keep_cost"])
    g = tp.get(cost_all=keep)
    for k in ("cost0", "c") + (("cost_all",) if keep else ()):
        u, v = g[k].ravel(), sol[k].ravel()
        assert u.shape == v.shape and np.array_equal(u.view(U32), v.view(U32)), (what, k, np.flatnonzero(u.view(U32) != v.view(U32))[:6])
    u, v = g["policy"].reshape(sol["policy"].shape), sol["policy"]
    assert np.array_equal(u, v), (what, "policy", np.argwhere(u != v)[:6].tolist(), u[u != v][:6], v[u != v][:6])
    i = tp.info()
    pb = sol["pb"]
    assert (i["valid"], i["nx"], i["ny"], i["H"], i["horizon"], i["slot"], i["balls"], i["body_balls"], i["goals"], i["goals_kept"], i["free"],
            i["finite0"], i["t_begin"], i["keep_cost"], i["launches"]) == (
        1, pb.shape[0], pb.shape[1], pb.H, int(sol["opts"]["horizon"]), sol["opts"]["slot"], sol["n"], sol["body"]["m"], sol["goals"],
        sol["goals_kept"], sol["free"], sol["finite0"], sol["t_begin"], int(keep), int(sol["opts"]["horizon"])), (what, i)
    assert F32(i["max_cost0"]) == F32(sol["max_cost0"]), (what, i["max_cost0"], sol["max_cost0"])
    return i


def _bits(u, v, what):
    u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    assert u.dtype == v.dtype and u.shape == v.shape, (what, u.dtype, v.dtype, u.shape, v.shape)
    if u.dtype.kind == "f":
        w = U64 if u.dtype == F64 else U32
        ok = (u.view(w) == v.view(w)) | (np.isnan(u) & np.isnan(v))
    else:
        ok = u == v
    assert ok.all(), (what, np.argwhere(~ok)[:6].tolist(), u[~ok][:4], v[~ok][:4])


def _paths_equal(tp, c, rpa, what, stream=0):
    got = tp.paths(c["starts"], stream=stream)
    for k in ("off", "points", "heading", "arrive", "start_cost", "status"):
        _bits(got[k], rpa[k], (what, "paths", k))
    return got


def _static_certificate(df, fp, sol, got, what):
    """Every (point, heading) a status-0 path visits has c > 0 and Footprint.clearance there gives (float)D >= clearance."""
    ok = got["status"] == 0
    if not ok.any():
        return
    rows = np.concatenate([np.arange(got["off"][r], got["off"][r + 1]) for r in np.flatnonzero(ok)])
    pts, hd = got["points"][rows], got["heading"][rows]
    H, ny, nx = sol["pb"].n3
    ij = np.rint((pts.astype(F64) - np.array(sol["pb"].origin, F64)) / float(sol["pb"].step)).astype(np.int64)
    assert (sol["c"][(hd * ny + ij[:, 1]) * nx + ij[:, 0]] > 0).all(), what
    states = np.concatenate([pts.astype(F64), sol["headings"][hd]], axis=1)
    D = fp.clearance(df, states, sol["opts"]["clearance"])["D"]
    assert (D.astype(F32) >= F32(sol["opts"]["clearance"])).all(), what


def _consumers(tp, ob, fp, df, c, sol, rpa, what):
    """check against the solve's own set and footprint, a newer set and another footprint, controls at the case's (T, k0), at
    k0 = 0 and past every arrival, and both certificates path by path."""
    got = _paths_equal(tp, c, rpa, what)
    newer = tc.shape_balls(c["sc"], 5, 99)
    other = pplan_cases.footprint(3)
    for S, dev in ((c["obst"], ob), (newer, None)):
        dev = device_set(S, c["sc"]["step"]) if dev is None else dev
        for body, dbody in ((None, None), (other, device_body(other))):
            for clr in (None, 0.4):
                ck = tp.check(dev, dbody, clr)
                ref = tr.check(sol, rpa, S, body, clr)
                for k in tr.CHECK_KEYS:
                    _bits(ck[k], ref[k], (what, "check", S["n"], body is not None, clr, k))
    ck = tp.check(ob)
    ok = got["status"] == 0
    assert not ck["collides"][ok].any() and (ck["first_hit"][ok] == -1).all(), what
    if c["obst"]["n"]:
        assert (ck["min_sep"][ok & (got["arrive"] > 0)] >= sol["opts"]["dyn_clearance"]).all(), what
    if df is not None:
        _static_certificate(df, fp, sol, got, what)
    past = int(max(got["arrive"].max(), 0)) + 3
    for T, k0, wl in ((c["T"], c["k0"], 0.0), (c["T"], 0, 0.7), (min(c["T"], 64), past, 0.0)):
        u = tp.controls(T, k0, wl)
        ref = tr.controls(sol, rpa, T, k0, wl, 1e-9)
        for k in ("U", "heading0", "p0", "clamped"):
            _bits(u[k], ref[k], (what, "controls", T, k0, wl, k))
    return got, ck


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_every_shape_with_the_broad_phase_off_and_on_against_the_reference(name):
    import gpismap_amd
    c = tc.shape_case(name)
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    share = sol["finite0"] / max(sol["free"], 1)
    print("%s: %s H %d S %d n %d body %d: finite at slot 0 on %.2f of %d free states; reference statuses %s" % (
        name, c["sc"]["shape"], c["H"], c["opts"]["horizon"], c["obst"]["n"], c["body"]["m"], share, sol["free"],
        np.bincount(rpa["status"], minlength=4).tolist()))
    assert share > 0
    tp, ob, fp, skipped = gpismap_amd.TimePosePlanner(), None, None, {}
    for cull in (0, 1):
        tp, ob, fp = _solve(c, df, tp, cull, ob=ob, fp=fp)
        i = _plan_equal(tp, sol, (name, cull))
        assert cull == 1 or i["skipped"] == 0, i
        skipped[cull] = i["skipped"]
    print("   triples skipped by the broad phase:", skipped, "solve %.2f ms" % i["solve_ms"])
    _consumers(tp, ob, fp, df, c, sol, rpa, name)


def test_horizon_1024_and_1025_refused():
    import gpismap_amd
    c = tc.long_case()
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    assert sol["finite0"] > 0
    for cull in (1, 0):
        tp, ob, fp = _solve(c, df, None, cull)
        _plan_equal(tp, sol, ("long", cull))
    _consumers(tp, ob, fp, df, c, sol, rpa, "long")
    with pytest.raises(gpismap_amd.GpisError) as e:
        tp.solve(df, c["goals"], fp, ob, H=c["H"], **dict(c["opts"], horizon=1025))
    assert _status_of(e) == -1
    _plan_equal(tp, sol, "after the refusal")


def test_broad_phase_skips_far_balls_and_only_those():
    c = tc.shape_case("f")                               # 256 balls over a box wider than the lattice, 3 x 2 tiles
    df, dist = _case_field(c)
    sol, _ = _ref(c, dist)
    tp, ob, fp = _solve(c, df, None, 1)
    some = _plan_equal(tp, sol, "f cull")["skipped"]
    tp, _, _ = _solve(c, df, tp, 0, ob=ob, fp=fp)
    assert some > 0 and _plan_equal(tp, sol, "f no cull")["skipped"] == 0
    # one ball in the middle of a single tile: never skipped
    c = dict(tc.shape_case("c"), name="c_mid")
    sc = c["sc"]
    mid = np.array(sc["origin"], F64) + 3.5 * sc["step"]
    c["obst"] = obst_ref.make(2, [mid], [[0.1, -0.1]], [0.02], epoch=0.0, step=sc["step"])
    df, dist = _case_field(c)
    sol, _ = _ref(c, dist)
    tp, _, _ = _solve(c, df, None, 1)
    assert _plan_equal(tp, sol, "c_mid")["skipped"] == 0
    print("case f: %d (tile, layer, ball) triples skipped; a ball amid one tile: 0" % some)


@pytest.mark.parametrize("name", tc.SMALL)
def test_small_scenes_one_branch_each(name):
    c = tc.small_case(name)
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    for cull in (0, 1):
        tp, ob, fp = _solve(c, df, None, cull)
        _plan_equal(tp, sol, (name, cull))
    got, _ = _consumers(tp, ob, fp, df, c, sol, rpa, name)
    print(name, "status", got["status"].tolist(), "arrive", got["arrive"].tolist())
    assert rpa["status"][0] == (3 if name in ("on_start", "short") else 0)       # (the scene on the device's own dist, by the reference)


def test_no_balls_is_the_devices_own_pose_planner():
    import gpismap_amd
    c = dict(tc.shape_case("d"), name="d_static", obst=tc.NO_BALLS, goals=pplan_cases.shape_goals(9, 17, 32))
    c["opts"] = dict(c["opts"], horizon=40, keep_cost=0)
    df, dist = _case_field(c)
    sol, _ = _ref(c, dist)
    tp, ob, fp = _solve(c, df)
    _plan_equal(tp, sol, "d_static")
    o = c["opts"]
    pp = df.plan_poses(fp, c["goals"], H=c["H"], moves=c["moves"], pose_planner=gpismap_amd.PosePlanner(), clearance=o["clearance"],
                       margin=o["margin"], gain=o["gain"], turn=o["turn"])
    cost, _, cc = pp.get()
    g = tp.get()
    assert np.isfinite(cost).sum() > 1000 and np.array_equal(g["cost0"].view(U32), cost.view(U32)) and np.array_equal(g["c"].view(U32), cc.view(U32))
    # no set at all is the empty set
    tp2 = gpismap_amd.TimePosePlanner().solve(df, c["goals"], fp, None, H=c["H"], moves=c["moves"], t_begin=5.0, **o)
    assert np.array_equal(tp2.get()["policy"], g["policy"]) and tp2.info()["balls"] == 0


def test_one_ball_zero_footprint_is_the_devices_own_time_planner():
    import gpismap_amd
    c = tplan_cases.shape_case("b")                      # 31 x 33, S = 7, one ball; margin 0: c is 0 or 1 at both planners
    o = dict(c["opts"], connectivity=1, margin=0.0, keep_cost=0)
    df, dist = _case_field(c)
    ob = device_set(c["obst"], c["sc"]["step"])
    t = df.plan_timed(c["goals"], ob, c["t_begin"], time_planner=gpismap_amd.TimePlanner(), **o)
    ref = t.get()["cost0"]
    fp = device_body(body_ref.point(2))
    po = {k: o[k] for k in ("clearance", "margin", "gain", "slot", "horizon", "dyn_clearance", "wait")}
    tp = df.plan_poses_timed(c["goals"], fp, ob, H=8, moves="any", t_begin=c["t_begin"], time_pose_planner=gpismap_amd.TimePosePlanner(),
                             turn=0.05, **po)
    got = tp.get()["cost0"]
    assert np.isfinite(ref).sum() > 100 and (~np.isfinite(ref)).sum() > 10
    for h in range(8):
        assert np.array_equal(got[h].view(U32), ref.view(U32)), h


def test_the_parked_disc_as_the_reference_routes_it_and_follow():
    import gpismap_amd
    c = tc.demo_case()
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    tp, ob, fp = _solve(c, df)
    _plan_equal(tp, sol, "demo")
    got, ck = _consumers(tp, ob, fp, df, c, sol, rpa, "demo")
    cells = rpa["cells"][0]
    w = int((np.diff(got["paths"][0], axis=0) == 0).all(axis=1).sum())
    assert got["status"][0] == 0 and got["arrive"][0] == rpa["arrive"][0] == 20 and w == tr.waits(rpa, 0) + tr.turns(rpa, 0) == 0
    assert ck["collides"][0] == 0 and ck["min_sep"][0] >= tc.DEMO["dyn_clearance"] and (cells[:, 1] <= 10).all() and (cells[:, 1] == 5).any()
    # the point planner of the device with the inscribed radius: its route, faced where it goes, drives the body into the disc
    o = c["opts"]
    t = df.plan_timed(c["goals"][:, :2], ob, 0.0, time_planner=gpismap_amd.TimePlanner(), clearance=tc.R_IN, margin=0.0, slot=o["slot"],
                      horizon=o["horizon"], dyn_clearance=o["dyn_clearance"] + tc.R_IN)
    s_in, p_in = tc.demo_point(tc.R_IN)
    assert np.array_equal(t.paths(c["starts"][:, :2])["points"], p_in["points"])
    t.solve(df, c["goals"][:, :2], ob, 0.0, clearance=tc.R_OUT, margin=0.0, slot=o["slot"], horizon=o["horizon"],
            dyn_clearance=o["dyn_clearance"] + tc.R_OUT)
    assert t.paths(c["starts"][:, :2])["status"][0] == 3
    print("demo: arrive %d, waits %d, cost %.4f, min_sep %.4f, solve %.2f ms" % (got["arrive"][0], w, got["start_cost"][0], ck["min_sep"][0],
                                                                           tp.info()["solve_ms"]))
    # follow: the controller's nominal sequence is controls' U
    T = 32
    ctl = gpismap_amd.Controller(dt=o["slot"])
    ctl.init(2, 64, T, seed=3)
    p0, h0 = tp.follow(ctl, 0, k0=2, w_limit=0.9)
    u = tp.controls(T, 2, 0.9)
    assert np.array_equal(ctl.get()["U"].view(U64), u["U"][0].view(U64)) and np.array_equal(p0, u["p0"][0]) and np.array_equal(h0, u["heading0"][0])
    assert np.array_equal(p0, got["paths"][0][2].astype(F64))


def test_result_outlives_field_set_and_footprint_on_one_handle_through_changing_problems():
    import torch
    import gpismap_amd
    tp = gpismap_amd.TimePosePlanner()
    ca, cb, cc = tc.shape_case("c"), tc.shape_case("d"), tc.shape_case("b")
    for c in (ca, cb, cc, ca):                            # the lattice, H, S, n and the body change on one handle, up and down
        df, dist = _case_field(c)
        sol, rpa = _ref(c, dist)
        tp, ob, fp = _solve(c, df, tp, 1)
        _plan_equal(tp, sol, c["name"])
        _paths_equal(tp, c, rpa, c["name"])
    # the field recomputed on other data, the set emptied, the footprint changed, all three closed: the plan and its paths stay
    sc = pplan_cases.shape_scene(50, 50)
    _field(sc["f"], sc["shape"], sc["origin"], sc["step"], df=df)
    ref_ck = tr.check(sol, rpa, ca["obst"])
    keep = device_set(ca["obst"], ca["sc"]["step"])
    ob.set(np.zeros((0, 2)), np.zeros((0, 2)), [])
    fp.set([(0.3, 0.3)], [0.2])
    _plan_equal(tp, sol, "field, set and footprint changed")
    _paths_equal(tp, ca, rpa, "field, set and footprint changed")
    ck = tp.check(keep)                                  # (the solve's own footprint, as the handle copied it)
    for k in tr.CHECK_KEYS:
        _bits(ck[k], ref_ck[k], ("check after the change", k))
    df.close()
    ob.close()
    fp.close()
    _plan_equal(tp, sol, "field, set and footprint closed")
    u = tp.controls(8)
    ref = tr.controls(sol, rpa, 8)
    _bits(u["U"], ref["U"], "controls after the close")
    ck = tp.check(keep)
    _bits(ck["min_sep"], ref_ck["min_sep"], "check after the close")
    # a caller's stream
    df, dist = _case_field(cb)
    sol, rpa = _ref(cb, dist)
    s = torch.cuda.Stream()
    tp, ob, fp = _solve(cb, df, tp, 1, stream=s.cuda_stream)
    _plan_equal(tp, sol, "stream")
    _paths_equal(tp, cb, rpa, "stream", stream=s.cuda_stream)


def test_errors_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    c = tc.shape_case("b")
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    tp, ob, fp = _solve(c, df)
    _paths_equal(tp, c, rpa, "first")
    ref_ck = tr.check(sol, rpa, c["obst"])

    def unchanged(what):
        _plan_equal(tp, sol, what)
        m, tot = C.c_longlong(0), C.c_longlong(0)
        assert L.gpis_tpplan_path_counts(tp.h, C.byref(m), C.byref(tot)) == 0 and (m.value, tot.value) == (rpa["status"].size, rpa["off"][-1])
        _bits(tp.check(ob)["min_sep"], ref_ck["min_sep"], what)

    def code(fn):
        with pytest.raises(gpismap_amd.GpisError) as e:
            fn()
        return _status_of(e)

    def go(field=df, goals=c["goals"], obst=ob, body=fp, t=c["t_begin"], H=c["H"], moves=c["moves"], headings=None, **kw):
        return tp.solve(field, goals, body, obst, H=H, moves=moves, t_begin=t, headings=headings, **dict(c["opts"], **kw))

    for kw in (dict(slot=0.0), dict(horizon=0), dict(horizon=1025), dict(wait=-1.0), dict(dyn_clearance=-0.1), dict(keep_cost=2), dict(gain=2e4),
               dict(turn=0.0), dict(turn=0.1 / 65), dict(turn=1001.0), dict(t=float("nan")), dict(goals=[(0.0, 1.0, 16.0)]),
               dict(goals=[(0.0, 1.0, 0.5)]), dict(moves=np.full(16, 0x10, np.uint16)), dict(headings=np.zeros((16, 2)))):
        assert code(lambda: go(**kw)) == -1, kw
    assert L.gpis_tpplan_solve(tp.h, df.h, ob.h, fp.h, None, None, 12, None, 1, 0.0, None, None) == -1
    unchanged("bad options, tables and goals")
    g3 = np.ones(5 * 4 * 3, F32)
    df3 = gpismap_amd.DistanceField()
    df3.from_grid(_dev(g3).data_ptr(), (5, 4, 3), (0.0, 0.0, 0.0), 0.5, 0.0)
    ob3 = gpismap_amd.Obstacles(3, 0.1).set([[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [0.1])
    fp3 = gpismap_amd.Footprint(3).set([(0.0, 0.0, 0.0)], [0.1])
    empty = gpismap_amd.Footprint(2).set(np.zeros((0, 2)), [])
    assert code(lambda: go(field=df3)) == -1                                                           # a 3-D field
    assert code(lambda: go(obst=ob3)) == -1                                                            # 3-D balls
    assert code(lambda: go(body=fp3)) == -3 and code(lambda: go(body=empty)) == -3                     # as gpis_pplan_solve
    hd, mv = gpismap_amd.heading_table(16), gpismap_amd.heading_moves(16)
    args = (hd.ctypes.data_as(C.POINTER(C.c_double)), mv.ctypes.data_as(C.POINTER(C.c_ushort)), 16, c["goals"].ctypes.data_as(C.POINTER(C.c_float)))
    assert L.gpis_tpplan_solve(tp.h, gpismap_amd.DistanceField().h, None, fp.h, *args, 1, 0.0, None, None) == -3
    assert L.gpis_tpplan_solve(tp.h, df.h, None, None, *args, 1, 0.0, None, None) == -1 and L.gpis_tpplan_solve(tp.h, df.h, None, fp.h, *args, 0, 0.0, None, None) == -1
    big = pplan_cases.balls_f((300, 300), 0.1, [((150.0, 150.0), 20.0)])
    dfb, _ = _field(big, (300, 300), (0.0, 0.0), 0.1)
    assert code(lambda: go(field=dfb, horizon=1024, keep_cost=1)) == -4                                # 300 x 300 x 16 x 1025 > 2^28
    unchanged("bad fields, sets and footprints")
    st3 = c["starts"].ctypes.data_as(C.POINTER(C.c_float))
    assert L.gpis_tpplan_paths(tp.h, None, 1, None) == -1 and L.gpis_tpplan_paths(tp.h, st3, 0, None) == -1
    assert L.gpis_tpplan_paths(tp.h, st3, (1 << 24) + 1, None) == -4
    assert code(lambda: tp.paths([(0.0, 1.0, 16.0)])) == -1 and code(lambda: tp.paths([(0.0, 1.0, -2.0)])) == -1
    assert code(lambda: tp.check(ob, None, -0.1)) == -1 and code(lambda: tp.check(ob, None, float("nan"))) == -1
    assert code(lambda: tp.check(ob3)) == -1 and code(lambda: tp.check(ob, fp3)) == -3 and code(lambda: tp.check(ob, empty)) == -3
    for kw in (dict(T=0), dict(T=257), dict(k0=-1), dict(k0=(1 << 20) + 1), dict(w_limit=-1.0), dict(min_move=float("inf"))):
        assert code(lambda: tp.controls(**dict(dict(T=4), **kw))) == -1, kw
    assert code(lambda: tp.set_schedule(2)) == -1
    unchanged("bad paths, checks and controls")
    # a handle without a solve, a solve without paths
    t2 = gpismap_amd.TimePosePlanner()
    assert L.gpis_tpplan_paths(t2.h, st3, 1, None) == -3 and t2.info()["valid"] == 0
    assert L.gpis_tpplan_get(t2.h, None, None, None, None) == -3
    t2.solve(df, c["goals"], fp, ob, H=c["H"], moves=c["moves"], t_begin=c["t_begin"], **dict(c["opts"], keep_cost=0))
    assert code(lambda: t2.check(ob)) == -3 and code(lambda: t2.controls(4)) == -3 and code(lambda: t2.get(cost_all=True)) == -3
    _plan_equal(t2, dict(sol, opts=dict(sol["opts"], keep_cost=0)), "without keep_cost")
