"""The footprint in the moving-obstacle check and in re-timing on the GPU (traj_body_time_check_kernel, traj_body_retime_kernel
and traj_body_states_kernel of csrc/traj.hip, gpis_timed_body_*) against the numpy reference (tests/body_time_ref.py) on the
shared cases (tests/body_time_cases.py).  The device's timing is held to the reference's bits before it is used
(tests/test_gpu_obst.py's _timed); then every output is compared exactly: the schedule's integers and its whole own table, the
checks' two doubles and the timed poses as bits (a NaN equals a NaN), the checks' four integers."""
import ctypes as C

import numpy as np
import pytest

import body_ref
import body_time_cases as bc
import body_time_ref as btr
import obst_cases as oc
import retime_cases as rc
import retime_ref as rr
import timing_cases as tc
import timing_ref
from test_gpu_mppi import env
from test_gpu_obst import _timed, device_set
from test_gpu_retime import _bits_equal, _rows, _sched_equal, _tile

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U64 = np.uint64
SKEYS = rr.RES_KEYS + ("own",)
CKEYS = ("U", "heading0", "p0", "clamped")
POINT_KEYS = ("min_sep", "min_time", "min_obstacle", "first_hit", "collides")


def device_body(b):
    """A Footprint holding the reference's footprint b, read back and compared."""
    import gpismap_amd
    fp = gpismap_amd.Footprint(b["dim"]).set(b["b"], b["rho"])
    g = fp.get()
    assert np.array_equal(g["offset"].view(U64), b["b"].view(U64)) and np.array_equal(g["radius"].view(U64), b["rho"].view(U64))
    return fp


def _same(got, ref, keys, what):
    for k in keys:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype, u.shape, v.shape)
        ok = (u.view(U64) == v.view(U64)) | (np.isnan(u) & np.isnan(v)) if u.dtype == F64 else u == v
        assert ok.all(), (what, k, np.argwhere(~ok)[:6].tolist(), u[~ok][:4], v[~ok][:4])


def _solve(tj, ob, fp, c, stream=0):
    got = tj.retime(ob, t_begin=c["t_begin"], stream=stream, footprint=fp, **c["opts"])
    assert (got["slot"], got["max_pause"], got["clearance"], got["press_on"], got["t_begin"]) == (
        c["opts"]["slot"], c["opts"]["max_pause"], c["opts"]["clearance"], c["opts"]["press_on"], c["t_begin"])
    assert tj.retimed_body_balls() == c["body"]["m"]
    return got


def _run(c, what, tj=None, stream=0, horizon=(64, 0)):
    """The body solve, the body check along it at the longest arrival, the poses along it, the controls along it and the
    certificate, against the reference on the case's distinct rows."""
    if tj is None:
        tj = _timed(c)
    ob, fp = device_set(c["obst"]), device_body(c["body"])
    small, idx = _rows(c)
    a = (small["x"], small["v"], small["t"], small["status"])
    ref_small = bc.ref_solve(small)
    got = _solve(tj, ob, fp, c, stream)
    _sched_equal(got, _tile(ref_small, idx, SKEYS), what)
    _sched_equal(tj.retimed(), got, (what, "the getter"))
    steps = int(max(1, min(4096, got["arrive"].max() + 3)))
    k = tj.retimed_check(ob, steps, footprint=fp)
    ref = btr.sched_check(*a, ref_small, c["obst"], c["body"], steps, None)
    _same(k, _tile(ref, idx, btr.CHECK_KEYS), btr.CHECK_KEYS, (what, "check", steps))
    ns = min(steps, 80)
    _same(dict(s=tj.timed_states(0.0, ns, retimed=True)), dict(s=btr.states(*a, 0.0, ns, sched=ref_small)[idx]), ("s",), (what, "states"))
    T, k0 = horizon
    ctl = dict(zip(CKEYS, tj.retimed_controls(T, k0=k0, w_limit=0.7)))
    _bits_equal(ctl, _tile(rr.controls(*a, ref_small, T, k0, 0.7, 1e-9), idx, CKEYS), CKEYS, (what, "controls"))
    clr = c["opts"]["clearance"]
    for r in np.flatnonzero((ref_small["status"] <= 1) & (ref_small["arrive"] >= 1)):
        kk = tj.retimed_check(ob, min(int(got["arrive"][r]), 4096), clearance=clr, footprint=fp)
        assert kk["collides"][r] == 0 and kk["first_hit"][r] == -1 and (c["obst"]["n"] == 0 or kk["min_sep"][r] >= clr), (what, r, kk["min_sep"][r])
    return tj, ob, fp, got


@pytest.mark.parametrize("shape", bc.SHAPES)
def test_solve_check_and_states_2d_every_shape(shape):
    _, _, _, got = _run(bc.shape_case(*shape), shape)
    print("m %d N %d P %d n %d A %d body %d:" % shape, "statuses", np.bincount(got["status"], minlength=5).tolist(), "pauses up to", got["pauses"].max())


@pytest.mark.parametrize("shape", bc.SHAPES3)
def test_solve_check_and_states_3d(shape):
    _run(bc.shape_case(*shape, dim=3), (3,) + shape, horizon=(65, 9))


def test_one_row_of_1024_own_slots():
    _, _, _, got = _run(bc.shape_case(*bc.LONG), bc.LONG, horizon=(256, 900))
    assert got["own_slots"][0] == 1024


@pytest.mark.parametrize("name", sorted(bc.special_cases()))
def test_special_case(name):
    c = bc.special_cases()[name]
    _, _, _, got = _run(c, name)
    expect = dict(table=1, parked_beside=0, turn_knot=3).get(name, c.get("expect", {}).get("status"))
    if expect is not None:
        assert int(got["status"][0]) == expect, (name, got["status"])


def _run_check(c, what):
    tj = _timed(c)
    ob, fp = device_set(c["obst"]), device_body(c["body"])
    got = tj.check(ob, c["dt"], c["steps"], t0=c["t0"], t_begin=c["t_begin"], clearance=c["clearance"], footprint=fp)
    _same(got, bc.ref_check(c), btr.CHECK_KEYS, what)
    ns = min(c["steps"], 1025)
    _same(dict(s=tj.timed_states(c["dt"], ns, t0=c["t0"])), dict(s=btr.states(c["x"], c["v"], c["t"], c["status"], c["dt"], ns, c["t0"])), ("s",),
          (what, "states"))
    return tj, ob, fp, got


@pytest.mark.parametrize("shape", bc.CHECK_SHAPES)
def test_check_and_states_2d_every_shape(shape):
    _run_check(bc.check_shape_case(*shape), shape)


@pytest.mark.parametrize("shape", bc.CHECK_SHAPES3)
def test_check_and_states_3d(shape):
    _run_check(bc.check_shape_case(*shape, dim=3), (3,) + shape)


@pytest.mark.parametrize("name", ("rear_only", "knot_case", "dup_end"))
def test_special_check_case(name):
    c = getattr(bc, name)()
    _, _, _, got = _run_check(c, name)
    if name == "rear_only":
        assert got["collides"][0] == 1 and got["min_ball"][0] == 1


def test_zero_footprint_has_the_point_entries_bits():
    c = oc.check_shape_case(*oc.CHECK_SHAPES[2])
    tj, ob, zero = _timed(c), device_set(c["obst"]), device_body(body_ref.point(2))
    a = (ob, c["dt"], c["steps"])
    kw = dict(t0=c["t0"], t_begin=c["t_begin"], clearance=c["clearance"])
    pt, bd = tj.check(*a, **kw), tj.check(*a, footprint=zero, **kw)
    _same(bd, pt, POINT_KEYS, "check")
    c = rc.special_cases()["batch"]
    tj, ob = _timed(c), device_set(c["obst"])
    pt = tj.retime(ob, t_begin=c["t_begin"], **c["opts"])
    assert tj.retimed_body_balls() == 0
    kp = tj.retimed_check(ob, 90)
    bd = tj.retime(ob, t_begin=c["t_begin"], footprint=zero, **c["opts"])
    assert tj.retimed_body_balls() == 1
    _sched_equal(bd, pt, "solve")
    _same(tj.retimed_check(ob, 90, footprint=zero), kp, POINT_KEYS, "retimed_check")
    _same(tj.retimed_check(ob, 90), kp, POINT_KEYS, "the point's check of the body's schedule")


def test_errors_leave_the_schedule_and_the_footprint_may_change():
    import gpismap_amd
    L = gpismap_amd.lib()
    c = bc.special_cases()["table"]
    tj, ob, fp, got = _run(c, "table")
    o = gpismap_amd.retime_opts(2, 0.25, **c["opts"])
    h = lambda x: x.h if x is not None else None
    empty, fp3, ob3 = gpismap_amd.Footprint(2).set(np.zeros((0, 2)), []), device_body(bc.body(3, 2)), device_set(oc.balls(3, 2, 0.2))
    solve = lambda t=tj, s=ob, b=fp, tb=0.0, opts=o: L.gpis_timed_body_retime(h(t), h(s), h(b), tb, C.byref(opts) if opts is not None else None, None)
    assert solve(t=None) == -1 and solve(s=None) == -1 and solve(b=None) == -1 and solve(opts=None) == -1 and solve(tb=np.nan) == -1
    assert solve(b=empty) == -1 and solve(b=fp3) == -1 and solve(s=ob3) == -1
    for kw in (dict(slot=0.0), dict(slot=np.nan), dict(max_pause=256), dict(clearance=-0.1), dict(press_on=2)):
        assert solve(opts=gpismap_amd.retime_opts(2, 0.25, **dict(c["opts"], **kw))) == -1, kw
    out = np.full(1, 7.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    chk = lambda s=ob, b=fp, steps=8, clr=0.1: L.gpis_timed_body_retime_check(tj.h, h(s), h(b), steps, clr, dp, None, None, None, None, None)
    for kw in (dict(s=None), dict(b=None), dict(b=empty), dict(b=fp3), dict(s=ob3), dict(steps=0), dict(steps=4097), dict(clr=-0.1), dict(clr=np.nan)):
        assert chk(**kw) == -1 and out[0] == 7.0, kw
    plain = lambda s=ob, b=fp, dt=0.25, steps=8, t0=0.0, tb=0.0, clr=0.1: L.gpis_timed_body_check(tj.h, h(s), h(b), dt, steps, t0, tb, clr, dp, None, None,
                                                                                                 None, None, None)
    for kw in (dict(s=None), dict(b=None), dict(b=empty), dict(b=fp3), dict(s=ob3), dict(dt=0.0), dict(steps=0), dict(steps=4097), dict(t0=-1.0),
               dict(tb=np.inf), dict(clr=-0.1)):
        assert plain(**kw) == -1 and out[0] == 7.0, kw
    st = np.full((1, 9, 4), 7.0)
    sp = st.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((0.0, 8, 0.0, 0), (0.25, 0, 0.0, 0), (0.25, 4097, 0.0, 0), (0.25, 8, -1.0, 0), (0.25, 8, 0.0, 2), (np.nan, 8, 0.0, 0)):
        assert L.gpis_timed_body_states(tj.h, *args, sp) == -1 and np.all(st == 7.0), args
    assert L.gpis_timed_body_states(tj.h, 0.25, 8, 0.0, 0, None) == -1
    _sched_equal(tj.retimed(), got, "after the errors")
    assert tj.retimed_body_balls() == 5
    # the footprint changes between the solve and the check: the check takes what it is given, the schedule stays
    a = (c["x"], c["v"], c["t"], c["status"])
    ref = bc.ref_solve(c)
    steps = int(got["arrive"][0])
    for nb in (2, 16):
        b2 = bc.body(2, nb)
        fp.set(b2["b"], b2["rho"])
        _same(tj.retimed_check(ob, steps, clearance=0.25, footprint=fp), btr.sched_check(*a, ref, c["obst"], b2, steps, 0.25), btr.CHECK_KEYS, ("changed", nb))
        assert tj.retimed_body_balls() == 5
    # a new timing drops the schedule; handles without one answer GPIS_ERR_STATE
    sc, df, dist, pl, _ = env(2)
    tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
    assert chk() == -3 and L.gpis_timed_body_states(tj.h, 0.25, 8, 0.0, 1, sp) == -3 and L.gpis_timed_body_info(tj.h, dp, 1) == -3
    assert L.gpis_timed_body_states(tj.h, 0.25, 8, 0.0, 0, sp) == 0 and plain() == 0
    fresh = gpismap_amd.Trajectories()
    assert solve(t=fresh) == -3 and plain() == 0 and L.gpis_timed_body_check(fresh.h, ob.h, fp.h, 0.25, 8, 0.0, 0.0, 0.1, *[None] * 6) == -3


def test_follow_a_body_schedule_and_the_static_field_at_its_poses():
    import gpismap_amd
    c = bc.special_cases()["table"]
    tj, ob, fp, got = _run(c, "table")
    ref = bc.ref_solve(c)
    a = (c["x"], c["v"], c["t"], c["status"])
    want = rr.controls(*a, ref, 8, 3, 0.5, 1e-9)
    ctl = gpismap_amd.Controller()
    ctl.init(2, 64, 8, seed=5)
    p0, h0 = ctl.follow(tj, 0, w_limit=0.5, retimed=True, k0=3)
    _bits_equal(dict(U=ctl.get()["U"], heading0=h0, p0=p0), dict(U=want["U"][0], heading0=want["heading0"][0], p0=want["p0"][0]),
                ("U", "heading0", "p0"), "follow")
    # Footprint.clearance on the timed poses: the static field at the samples the schedule visits
    sc, df, dist, pl, _ = env(2)
    S = tj.timed_states(0.0, int(got["arrive"][0]), retimed=True)[0]
    k = fp.clearance(df, S, clearance=0.25)
    want = body_ref.clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["body"], S, 0.25)
    _same(k, want, ("D", "ball"), "clearance at the poses")
    assert (k["below"], k["off"], k["least"]) == (want["below"], want["off"], want["least"])


def test_one_handle_through_changing_m_n_and_footprint():
    import gpismap_amd
    tj = gpismap_amd.Trajectories()
    sc, df, dist, pl, _ = env(2)
    for shape in ((11, 64, 63, 2, 64, 5), (1, 3, 1, 2, 1, 2), (600, 64, 1, 2, 64, 1), (11, 256, 63, 2, 64, 16), (1, 64, 0, 1, 0, 2), (11, 3, 255, 1, 63, 15)):
        c = bc.shape_case(*shape)
        df.smooth(c["x"], trajectories=tj, iters=0)
        tm = tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
        for k in ("v", "t"):                             # the device's timing is the reference's
            u, w = tm[k], np.ascontiguousarray(c[k], F32)
            assert ((u.view(np.uint32) == w.view(np.uint32)) | (np.isnan(u) & np.isnan(w))).all(), (shape, k)
        _run(c, ("one handle",) + shape, tj=tj)
        ob, fp = device_set(c["obst"]), device_body(c["body"])
        got = tj.check(ob, 0.5, 33, t_begin=oc.T_NOW, footprint=fp)
        small, idx = _rows(c)
        ref = btr.check(small["x"], small["v"], small["t"], small["status"], c["obst"], c["body"], 0.5, 33, 0.0, oc.T_NOW, None)
        _same(got, _tile(ref, idx, btr.CHECK_KEYS), btr.CHECK_KEYS, ("one handle", "check") + shape)


def test_same_schedule_on_a_callers_stream():
    import torch
    c = bc.special_cases()["batch"]
    tj, ob, fp, got = _run(c, "own stream")
    s = torch.cuda.Stream(device=0)
    _sched_equal(_solve(tj, ob, fp, c, stream=s.cuda_stream), got, "a caller's stream")
    _run(c, "a caller's stream", tj=tj, stream=s.cuda_stream, horizon=(65, 4))


def test_the_tables_scene_on_the_device():
    """DESIGN.md §7x's table on the device: the reference's statuses and pause counts for the body and the three points, and
    the body's check of each schedule."""
    ts = bc.table_scene()
    c = ts["case"]
    tj, ob, fp = _timed(c), device_set(c["obst"]), device_body(c["body"])
    a = (c["x"], c["v"], c["t"], c["status"])
    for name, extra in (("body", None), ("inscribed", bc.R_IN), ("disc", bc.R_DISC), ("circumscribed", bc.R_OUT)):
        ref, ref_k = ts["rows"][name]
        if extra is None:
            got = tj.retime(ob, footprint=fp, **bc.BASE)
        else:
            got = tj.retime(ob, **dict(bc.BASE, clearance=bc.BASE["clearance"] + extra))
        _sched_equal(got, ref, name)
        k = tj.retimed_check(ob, int(got["arrive"][0]), clearance=bc.BASE["clearance"], footprint=fp)
        _same(k, ref_k, btr.CHECK_KEYS, (name, "check"))
        print(name, "status", got["status"][0], "pauses", got["pauses"][0], "the body's least separation", k["min_sep"][0], "collides", k["collides"][0])
        assert k["collides"][0] == (1 if name in ("inscribed", "disc") else 0)
