"""The time planner on the GPU (csrc/tplan.hip, gpis_tplan_*) against the numpy reference (tests/tplan_ref.py) on the shared cases
(tests/tplan_cases.py).  Every field comes from DistanceField.from_grid and the reference runs on the device's own dist.  Every
output is compared exactly: the bits of cost0, c and cost_all, every policy byte of every layer, the paths' offsets, points,
arrivals, start costs and statuses, the check's two doubles as bits (a NaN equals a NaN) with its three integers, and U,
heading0, p0 as bits with clamped -- for every schedule (layers per launch, broad phase), which the results must not depend on."""
import ctypes as C

import numpy as np
import pytest

import obst_ref
import pplan_cases
import tplan_cases as tc
import tplan_ref as tr
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


def _case_field(c):
    sc = c["sc"]
    return _field(sc["f"], sc["shape"], sc["origin"], sc["step"])


def _ref(c, dist):
    """(solution, paths) of the reference on the device's own dist: computed once per case, left unchanged."""
    key = (c["name"], dist.tobytes())
    if key not in _REF:
        sol = tc.ref_solve(c, dist)
        _REF[key] = (sol, tr.paths(sol, c["starts"]))
    return _REF[key]


def _solve(c, df, tp=None, sched=None, stream=0, ob=None):
    import gpismap_amd
    tp = tp if tp is not None else gpismap_amd.TimePlanner()
    if sched is not None:
        tp.set_schedule(*sched)
    ob = ob if ob is not None else device_set(c["obst"], c["sc"]["step"])
    assert df.plan_timed(c["goals"], ob, c["t_begin"], time_planner=tp, **c["opts"]) is tp if stream == 0 else \
        tp.solve(df, c["goals"], ob, c["t_begin"], stream=stream, **c["opts"]) is tp
    return tp, ob


def _plan_equal(tp, sol, what):
    keep = bool(sol["opts"]["keep_cost"])
    g = tp.get(cost_all=keep)
    for k in ("cost0", "c") + (("cost_all",) if keep else ()):
        u, v = g[k].ravel(), sol[k].ravel()
        assert u.shape == v.shape and np.array_equal(u.view(U32), v.view(U32)), (what, k, np.flatnonzero(u.view(U32) != v.view(U32))[:6])
    u, v = g["policy"].reshape(sol["policy"].shape), sol["policy"]
    assert np.array_equal(u, v), (what, "policy", np.argwhere(u != v)[:6].tolist(), u[u != v][:6], v[u != v][:6])
    i = tp.info()
    S = int(sol["opts"]["horizon"])
    assert (i["valid"], i["nx"], i["ny"], i["horizon"], i["slot"], i["balls"], i["goals"], i["goals_kept"], i["free"], i["finite0"],
            i["t_begin"], i["keep_cost"]) == (1,) + tuple(sol["pb"].shape) + (S, sol["opts"]["slot"], sol["n"], sol["goals"],
                                                                               sol["goals_kept"], sol["free"], sol["finite0"],
                                                                               sol["t_begin"], int(keep)), (what, i)
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
    for k in ("off", "points", "arrive", "start_cost", "status"):
        _bits(got[k], rpa[k], (what, "paths", k))
    return got


def _consumers(tp, ob, c, sol, rpa, what):
    """check against the solve's own set and a newer one, controls at the case's (T, k0), at k0 = 0 and past every arrival, and
    the certificate path by path."""
    got = _paths_equal(tp, c, rpa, what)
    newer = tc.shape_balls(c["sc"], 5, 99)
    for S, dev in ((c["obst"], ob), (newer, None)):
        dev = device_set(S, c["sc"]["step"]) if dev is None else dev
        for clr in (None, 0.4):
            ck = tp.check(dev, clr)
            ref = tr.check(sol, rpa, S, clr)
            for k in tr.CHECK_KEYS:
                _bits(ck[k], ref[k], (what, "check", S["n"], clr, k))
    ck = tp.check(ob)
    ok = got["status"] == 0
    assert not ck["collides"][ok].any() and (ck["first_hit"][ok] == -1).all(), what
    if c["obst"]["n"]:
        assert (ck["min_sep"][ok & (got["arrive"] > 0)] >= sol["opts"]["dyn_clearance"]).all(), what
    past = int(max(got["arrive"].max(), 0)) + 3
    for T, k0, wl in ((c["T"], c["k0"], 0.0), (c["T"], 0, 0.7), (min(c["T"], 64), past, 0.0)):
        u = tp.controls(T, k0, wl)
        ref = tr.controls(sol, rpa, T, k0, wl, 1e-9)
        for k in ("U", "heading0", "p0", "clamped"):
            _bits(u[k], ref[k], (what, "controls", T, k0, wl, k))
    return got, ck


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_every_shape_and_schedule_against_the_reference(name):
    import gpismap_amd
    c = tc.shape_case(name)
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    share = sol["finite0"] / max(sol["free"], 1)
    print("%s: %s S %d n %d: finite at slot 0 on %.2f of %d free points; reference statuses %s" % (
        name, c["sc"]["shape"], c["opts"]["horizon"], c["obst"]["n"], share, sol["free"], np.bincount(rpa["status"], minlength=4).tolist()))
    assert share > 0
    tp, ob, skipped = gpismap_amd.TimePlanner(), None, {}
    for sched in tc.SCHEDULES + ((0, 1),):
        tp, ob = _solve(c, df, tp, sched, ob=ob)
        i = _plan_equal(tp, sol, (name, sched))
        S, L = c["opts"]["horizon"], sched[0] or (4 if c["obst"]["n"] == 0 else 1)
        assert i["layer_launches"] == -(-S // L) and (sched[1] == 1 or i["skipped"] == 0), (sched, i)
        skipped[sched] = i["skipped"]
    print("   triples skipped by the broad phase:", skipped)
    _consumers(tp, ob, c, sol, rpa, name)


def test_horizon_1024_and_1025_refused():
    import gpismap_amd
    c = tc.long_case()
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    assert sol["finite0"] > 0
    for sched in ((16, 1), (1, 0)):
        tp, ob = _solve(c, df, None, sched)
        _plan_equal(tp, sol, ("long", sched))
    _consumers(tp, ob, c, sol, rpa, "long")
    with pytest.raises(gpismap_amd.GpisError) as e:
        tp.solve(df, c["goals"], ob, **dict(c["opts"], horizon=1025))
    assert _status_of(e) == -1
    _plan_equal(tp, sol, "after the refusal")


def test_broad_phase_skips_far_balls_and_only_those():
    c = tc.shape_case("d")                               # 256 balls over a box 1.5 times the lattice, 2 x 3 tiles
    df, dist = _case_field(c)
    sol, _ = _ref(c, dist)
    tp, ob = _solve(c, df, None, (1, 1))
    some = _plan_equal(tp, sol, "d cull")["skipped"]
    tp, _ = _solve(c, df, tp, (1, 0), ob=ob)
    assert some > 0 and _plan_equal(tp, sol, "d no cull")["skipped"] == 0
    # one ball in the middle of a single tile: never skipped
    c = dict(tc.shape_case("c"), name="c_mid")
    sc = c["sc"]
    mid = np.array(sc["origin"], F64) + 16 * sc["step"]
    c["obst"] = obst_ref.make(2, [mid], [[0.1, -0.1]], [0.2], epoch=0.0, step=sc["step"])
    df, dist = _case_field(c)
    sol, _ = _ref(c, dist)
    for L in (1, 8):
        tp, _ = _solve(c, df, None, (L, 1))
        assert _plan_equal(tp, sol, ("c_mid", L))["skipped"] == 0
    print("case d: %d (tile, batch, ball) triples skipped at L = 1; a ball amid one tile: 0" % some)


@pytest.mark.parametrize("name", tc.SMALL)
def test_small_scenes_one_branch_each(name):
    c = tc.small_case(name)
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    for sched in ((1, 0), (8, 1)):
        tp, ob = _solve(c, df, None, sched)
        _plan_equal(tp, sol, (name, sched))
    got, _ = _consumers(tp, ob, c, sol, rpa, name)
    print(name, "status", got["status"].tolist(), "arrive", got["arrive"].tolist())


def _z_on_device(kind, speed=0.3, **kw):
    c = tc.z_case(kind, speed)
    c["opts"].update(kw)
    df, dist = _case_field(c)
    sol, rpa = _ref(dict(c, name="%s %s %s" % (c["name"], speed, sorted(kw.items()))), dist)
    tp, ob = _solve(c, df)
    _plan_equal(tp, sol, c["name"])
    return c, df, dist, tp, ob, sol, rpa


def test_no_balls_is_the_devices_own_planner():
    import gpismap_amd
    c, df, dist, tp, ob, sol, rpa = _z_on_device("static", horizon=84)
    o = c["opts"]
    pl = df.plan(c["goals"], planner=gpismap_amd.Planner(), clearance=o["clearance"], margin=o["margin"], gain=o["gain"],
                 connectivity=o["connectivity"])
    cost, _ = pl.get()
    cost0 = tp.get()["cost0"]
    assert np.isfinite(cost).sum() > 1000 and np.array_equal(cost0.view(U32), cost.view(U32))
    # no set at all is the empty set
    tp2 = gpismap_amd.TimePlanner().solve(df, c["goals"], None, 5.0, **o)
    assert np.array_equal(tp2.get()["policy"], tp.get()["policy"]) and tp2.info()["balls"] == 0


def test_parked_and_crossing_discs_as_the_reference_routes_them():
    import gpismap_amd
    for kind, speed in (("parked", 0.3), ("crossing", 0.3), ("crossing", 0.1)):
        c, df, dist, tp, ob, sol, rpa = _z_on_device(kind, speed)
        got, ck = _consumers(tp, ob, c, sol, rpa, (kind, speed))
        w = int((got["paths"][0][1:] == got["paths"][0][:-1]).all(axis=1).sum())
        assert got["status"][0] == 0 and w == tr.waits(rpa, 0) and got["arrive"][0] == rpa["arrive"][0]
        assert (w == 0 and got["paths"][0][:, 1].max() > 4.5) if kind == "parked" else (w >= 1 and got["paths"][0][:, 1].max() < 4.5)
        print("%s %.1f: arrive %d, waits %d, cost %.4f, min_sep %.4f, solve %.2f ms" % (
            kind, speed, got["arrive"][0], w, got["start_cost"][0], ck["min_sep"][0], tp.info()["solve_ms"]))
    # follow: the controller's nominal sequence is controls' U
    T = 48
    ctl = gpismap_amd.Controller(dt=c["opts"]["slot"])
    ctl.init(2, 64, T, seed=3)
    p0, h0 = tp.follow(ctl, 0, k0=2, w_limit=0.9)
    u = tp.controls(T, 2, 0.9)
    assert np.array_equal(ctl.get()["U"].view(U64), u["U"][0].view(U64)) and np.array_equal(p0, u["p0"][0]) and np.array_equal(h0, u["heading0"][0])
    assert np.array_equal(p0, got["paths"][0][2].astype(F64))


def test_result_outlives_field_and_set_on_one_handle_through_changing_problems():
    import torch
    import gpismap_amd
    tp = gpismap_amd.TimePlanner()
    ca, cb, cc = tc.shape_case("c"), tc.shape_case("e"), tc.shape_case("b")
    for c in (ca, cb, cc, ca):                            # the lattice, S and n change on one handle, up and down
        df, dist = _case_field(c)
        sol, rpa = _ref(c, dist)
        tp, ob = _solve(c, df, tp, (2, 1))
        _plan_equal(tp, sol, c["name"])
        _paths_equal(tp, c, rpa, c["name"])
    # the field recomputed on other data, the set emptied, both closed: the plan and its paths stay
    sc = pplan_cases.shape_scene(50, 50)
    _field(sc["f"], sc["shape"], sc["origin"], sc["step"], df=df)
    ob.set(np.zeros((0, 2)), np.zeros((0, 2)), [])
    _plan_equal(tp, sol, "field and set changed")
    _paths_equal(tp, ca, rpa, "field and set changed")
    df.close()
    ob.close()
    _plan_equal(tp, sol, "field and set closed")
    u = tp.controls(8)
    ref = tr.controls(sol, rpa, 8)
    _bits(u["U"], ref["U"], "controls after the close")
    # a caller's stream
    df, dist = _case_field(cb)
    sol, rpa = _ref(cb, dist)
    s = torch.cuda.Stream()
    tp, ob = _solve(cb, df, tp, (0, 1), stream=s.cuda_stream)
    _plan_equal(tp, sol, "stream")
    _paths_equal(tp, cb, rpa, "stream", stream=s.cuda_stream)


def test_errors_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    c = tc.shape_case("b")
    df, dist = _case_field(c)
    sol, rpa = _ref(c, dist)
    tp, ob = _solve(c, df)
    _paths_equal(tp, c, rpa, "first")

    def unchanged(what):
        _plan_equal(tp, sol, what)
        m, tot = C.c_longlong(0), C.c_longlong(0)
        assert L.gpis_tplan_path_counts(tp.h, C.byref(m), C.byref(tot)) == 0 and (m.value, tot.value) == (rpa["status"].size, rpa["off"][-1])
        ck = tp.check(ob)
        _bits(ck["min_sep"], tr.check(sol, rpa, c["obst"])["min_sep"], what)

    def code(fn):
        with pytest.raises(gpismap_amd.GpisError) as e:
            fn()
        return _status_of(e)

    go = lambda field=df, goals=c["goals"], obst=ob, t=c["t_begin"], **kw: tp.solve(field, goals, obst, t, **dict(c["opts"], **kw))
    for kw in (dict(slot=0.0), dict(horizon=0), dict(horizon=1025), dict(wait=-1.0), dict(dyn_clearance=-0.1), dict(keep_cost=2),
               dict(connectivity=3), dict(gain=2e4), dict(t=float("nan"))):
        assert code(lambda: go(**kw)) == -1, kw
    unchanged("bad options")
    g3 = np.ones(5 * 4 * 3, F32)
    df3 = gpismap_amd.DistanceField()
    df3.from_grid(_dev(g3).data_ptr(), (5, 4, 3), (0.0, 0.0, 0.0), 0.5, 0.0)
    ob3 = gpismap_amd.Obstacles(3, 0.1).set([[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [0.1])
    assert L.gpis_tplan_solve(tp.h, df3.h, None, c["goals"].ctypes.data_as(C.POINTER(C.c_float)), 1, 0.0, None, None) == -1   # a 3-D field
    assert code(lambda: go(obst=ob3)) == -1                                                            # 3-D balls
    assert L.gpis_tplan_solve(tp.h, gpismap_amd.DistanceField().h, None, c["goals"].ctypes.data_as(C.POINTER(C.c_float)), 1, 0.0, None, None) == -3
    assert L.gpis_tplan_solve(tp.h, df.h, None, None, 1, 0.0, None, None) == -1 and L.gpis_tplan_solve(tp.h, df.h, None, c["goals"].ctypes.data_as(C.POINTER(C.c_float)), 0, 0.0, None, None) == -1
    big = pplan_cases.balls_f((600, 600), 0.1, [((300.0, 300.0), 20.0)])
    dfb, _ = _field(big, (600, 600), (0.0, 0.0), 0.1)
    assert code(lambda: go(field=dfb, horizon=1024, keep_cost=1)) == -4                                # 600 x 600 x 1025 > 2^28
    unchanged("bad fields and sets")
    assert L.gpis_tplan_paths(tp.h, None, 1, None) == -1 and L.gpis_tplan_paths(tp.h, c["starts"].ctypes.data_as(C.POINTER(C.c_float)), 0, None) == -1
    assert L.gpis_tplan_paths(tp.h, c["starts"].ctypes.data_as(C.POINTER(C.c_float)), (1 << 24) + 1, None) == -4
    assert code(lambda: tp.check(ob, -0.1)) == -1 and code(lambda: tp.check(ob, float("nan"))) == -1 and code(lambda: tp.check(ob3)) == -1
    for kw in (dict(T=0), dict(T=257), dict(k0=-1), dict(k0=(1 << 20) + 1), dict(w_limit=-1.0), dict(min_move=float("inf"))):
        assert code(lambda: tp.controls(**dict(dict(T=4), **kw))) == -1, kw
    assert code(lambda: tp.set_schedule(17, 1)) == -1 and code(lambda: tp.set_schedule(1, 2)) == -1
    unchanged("bad paths, checks and controls")
    # a handle without a solve, a solve without paths
    t2 = gpismap_amd.TimePlanner()
    assert code(lambda: t2.paths(c["starts"])) == -3 and t2.info()["valid"] == 0
    assert L.gpis_tplan_get(t2.h, None, None, None, None) == -3
    t2.solve(df, c["goals"], ob, c["t_begin"], **dict(c["opts"], keep_cost=0))
    assert code(lambda: t2.check(ob)) == -3 and code(lambda: t2.controls(4)) == -3 and code(lambda: t2.get(cost_all=True)) == -3
    _plan_equal(t2, dict(sol, opts=dict(sol["opts"], keep_cost=0)), "without keep_cost")
