"""Re-timing on the GPU (traj_retime_kernel and the schedule-reading kernels of csrc/traj.hip, gpis_retime_*) against the numpy
reference (tests/retime_ref.py) on the shared cases (tests/retime_cases.py).  The device's timing is held to the reference's bits
before it is used (tests/test_gpu_obst.py's _timed); then every output is compared exactly: the schedule's status, its four
integers and the whole own table as integers, U, heading0, p0 as bits, clamped, and the check's two doubles as bits (a NaN equals
a NaN) with its three integers."""
import ctypes as C
import functools

import numpy as np
import pytest

import obst_cases as oc
import obst_ref
import retime_cases as rc
import retime_ref as rr
import timing_cases as tc
import timing_ref
from test_gpu_mppi import env
from test_gpu_obst import _check_equal, _timed, device_set

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
SKEYS = rr.RES_KEYS + ("own",)
CKEYS = ("U", "heading0", "p0", "clamped")
UNIQUE = len(tc.NAMES)                                   # a batch of more rows repeats the curves


def _rows(c):
    """(the case cut to its distinct rows, the index that tiles them back)."""
    m = c["x"].shape[0]
    if m <= UNIQUE:
        return c, np.arange(m)
    return dict(c, **{k: c[k][:UNIQUE] for k in ("x", "v", "t", "status")}), np.arange(m) % UNIQUE


def _tile(d, idx, keys):
    return {k: np.ascontiguousarray(d[k][idx]) for k in keys}


def _sched_equal(got, ref, what):
    for k in SKEYS:
        u, v = np.asarray(got[k]), np.asarray(ref[k])
        assert u.dtype == np.int32 and v.dtype == np.int32 and u.shape == v.shape, (what, k, u.dtype, u.shape, v.shape)
        assert np.array_equal(u, v), (what, k, np.argwhere(u != v)[:6].tolist(), u[u != v][:6], v[u != v][:6])


def _bits_equal(got, ref, keys, what):
    for k in keys:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype, u.shape, v.shape)
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (what, k, np.argwhere(u != v)[:6].tolist())


def _solve(tj, ob, c, stream=0):
    got = tj.retime(ob, t_begin=c["t_begin"], stream=stream, **c["opts"])
    assert (got["slot"], got["max_pause"], got["clearance"], got["press_on"], got["t_begin"]) == (
        c["opts"]["slot"], c["opts"]["max_pause"], c["opts"]["clearance"], c["opts"]["press_on"], c["t_begin"])
    return got


def _consumers(tj, ob, c, sched, ref_small, idx, what, horizons):
    """controls at the given (T, k0) and the check at the longest arrival, against the reference on the distinct rows."""
    small, _ = _rows(c)
    for T, k0 in horizons:
        for wl in (0.0, 0.7):
            got = dict(zip(CKEYS, tj.retimed_controls(T, k0=k0, w_limit=wl)))
            ref = rr.controls(small["x"], small["v"], small["t"], small["status"], ref_small, T, k0, wl, 1e-9)
            _bits_equal(got, _tile(ref, idx, CKEYS), CKEYS, (what, "controls", T, k0, wl))
    steps = int(max(1, min(4096, sched["arrive"].max() + 3)))
    for S, dev in ((c["obst"], ob), (oc.balls(c["x"].shape[2], 3, 0.25), None)):     # its own set, and a newer detection
        dev = device_set(S) if dev is None else dev
        got = tj.retimed_check(dev, steps)
        ref = rr.check(small["x"], small["v"], small["t"], small["status"], ref_small, S, steps, None)
        _check_equal(got, _tile(ref, idx, tuple(ref)), (what, "check", steps, S["n"]))
    # the certificate, row by row of the distinct rows: clear up to its own arrival
    clr = c["opts"]["clearance"]
    for r in np.flatnonzero((ref_small["status"] <= 1) & (ref_small["arrive"] >= 1)):
        k = tj.retimed_check(ob, min(int(sched["arrive"][r]), 4096), clearance=clr)
        assert k["collides"][r] == 0 and k["first_hit"][r] == -1 and (c["obst"]["n"] == 0 or k["min_sep"][r] >= clr), (what, r, k["min_sep"][r])


def _run(c, what, horizons, tj=None, stream=0):
    import gpismap_amd
    if tj is None:
        tj = _timed(c)
    ob = device_set(c["obst"])
    small, idx = _rows(c)
    ref_small = rc.ref_solve(small)
    ref = dict(_tile(ref_small, idx, SKEYS))
    got = _solve(tj, ob, c, stream)
    _sched_equal(got, ref, what)
    _sched_equal(tj.retimed(), ref, (what, "the getter"))
    _consumers(tj, ob, c, got, ref_small, idx, what, horizons)
    return tj, ob, got


# (T, k0) paired with the shapes: T in {1, 64, 65, 256}; k0 zero, inside the schedule and past the arrival
HORIZONS = (((1, 0),), ((64, 0),), ((65, 7), (1, 300)), ((256, 0),), ((64, 31),), ((65, 0), (64, 2000)), ((1, 5),), ((256, 3),), ((64, 40),))


@pytest.mark.parametrize("shape,horizons", tuple(zip(rc.SHAPES, HORIZONS)))
def test_solve_controls_and_check_2d_every_shape(shape, horizons):
    c = rc.shape_case(*shape)
    _, _, got = _run(c, shape, horizons)
    print("m %d N %d P %d n %d A %d: statuses %s, pauses up to %d" % (shape + (np.bincount(got["status"], minlength=5).tolist(), got["pauses"].max())))


@pytest.mark.parametrize("shape", rc.SHAPES3)
def test_solve_controls_and_check_3d(shape):
    _run(rc.shape_case(*shape, dim=3), (3,) + shape, ((65, 0), (64, 9)))


def test_one_row_of_1024_own_slots():
    c = rc.shape_case(*rc.LONG)
    _, _, got = _run(c, rc.LONG, ((256, 900),))
    assert got["own_slots"][0] == 1024


@pytest.mark.parametrize("name", sorted(rc.special_cases()))
def test_special_case(name):
    c = rc.special_cases()[name]
    _, _, got = _run(c, name, ((64, 0), (65, 28)))
    if c["expect"]["status"] is not None:
        assert int(got["status"][0]) == c["expect"]["status"], (name, got["status"])


def test_the_schedule_dies_with_the_timing_and_errors_leave_it():
    import gpismap_amd
    L = gpismap_amd.lib()
    c = rc.special_cases()["crossing"]
    tj, ob, got = _run(c, "crossing", ((8, 0),))
    sc, df, dist, pl, _ = env(2)
    ob3 = device_set(oc.balls(3, 2, 0.2))
    o = gpismap_amd.retime_opts(2, 0.25, **c["opts"])
    solve = lambda t=tj, s=ob, tb=0.0, opts=o: L.gpis_retime_solve(t.h if t is not None else None, s.h if s is not None else None, tb,
                                                                    C.byref(opts) if opts is not None else None, None)
    bad = [gpismap_amd.retime_opts(2, 0.25, **dict(c["opts"], **kw)) for kw in (
        dict(slot=0.0), dict(slot=-1.0), dict(slot=np.nan), dict(slot=np.inf), dict(max_pause=-1), dict(max_pause=256), dict(clearance=-0.1),
        dict(clearance=np.nan), dict(press_on=2), dict(press_on=-1))]
    for k, b in enumerate(bad):
        assert solve(opts=b) == -1, k
    assert solve(t=None) == -1 and solve(s=None) == -1 and solve(opts=None) == -1 and solve(tb=np.nan) == -1 and solve(s=ob3) == -1
    U = np.full((1, 8, 2), 7.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ctrl = lambda T=8, k0=0, wl=0.0, mm=0.0: L.gpis_retime_controls(tj.h, T, k0, wl, mm, dp(U), None, None, None)
    for kw in (dict(T=0), dict(T=257), dict(k0=-1), dict(k0=(1 << 20) + 1), dict(wl=-1.0), dict(wl=np.nan), dict(mm=-1.0), dict(mm=np.inf)):
        assert ctrl(**kw) == -1 and np.all(U == 7.0), kw
    chk = lambda s=ob, steps=8, clr=0.1: L.gpis_retime_check(tj.h, s.h if s is not None else None, steps, clr, None, None, None, None, None)
    assert chk(s=None) == -1 and chk(steps=0) == -1 and chk(steps=4097) == -1 and chk(clr=-0.1) == -1 and chk(clr=np.nan) == -1 and chk(s=ob3) == -1
    ctl = gpismap_amd.Controller()
    follow = lambda cc=ctl, i=0, k0=0, wl=0.0, mm=0.0: L.gpis_retime_follow(cc.h, tj.h, i, k0, wl, mm, None, None)
    assert follow() == -3                                 # not initialised
    ctl.init(2, 64, 8, seed=5)
    A = np.random.default_rng(1).uniform(-0.1, 0.1, (8, 2))
    ctl.set_nominal(A)
    assert follow(i=-1) == -1 and follow(i=1) == -1 and follow(k0=-1) == -1 and follow(wl=-1.0) == -1 and follow(mm=-1.0) == -1
    assert follow(cc=gpismap_amd.Controller().init(3, 64, 8)) == -1
    assert np.array_equal(ctl.get()["U"], A)
    _sched_equal(tj.retimed(), got, "after the errors")
    # follow writes the schedule's sequence into the nominal one
    ref = rr.controls(c["x"], c["v"], c["t"], c["status"], rc.ref_solve(c), 8, 3, 0.5, 1e-9)
    p0, h0 = ctl.follow(tj, 0, w_limit=0.5, retimed=True, k0=3)
    _bits_equal(dict(U=ctl.get()["U"], heading0=h0, p0=p0), dict(U=ref["U"][0], heading0=ref["heading0"][0], p0=ref["p0"][0]),
                ("U", "heading0", "p0"), "follow")
    with pytest.raises(gpismap_amd.GpisError):
        ctl.follow(tj, 0, 0.25, retimed=True)
    # a row without a schedule is not followed
    pk = rc.special_cases()["parked"]
    tp, _, gp = _run(pk, "parked", ((8, 0),))
    assert gp["status"][0] == 3 and L.gpis_retime_follow(ctl.h, tp.h, 0, 0, 0.0, 0.0, None, None) == -3
    # a new timing, a new result and a new input each drop the schedule
    get = lambda t: L.gpis_retime_get(t.h, *[None] * 8)
    assert get(tj) == 0
    tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
    assert get(tj) == -3 and ctrl() == -3 and chk() == -3 and follow() == -3
    with pytest.raises(gpismap_amd.GpisError):
        tj.retimed()
    _sched_equal(_solve(tj, ob, c), got, "again")
    tj.optimize(df, iters=0)
    assert get(tj) == -3 and solve() == -3               # a result without a timing
    tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
    _sched_equal(_solve(tj, ob, c), got, "and again")
    tj.set(c["x"])
    assert get(tj) == -3
    fresh = gpismap_amd.Trajectories()
    assert get(fresh) == -3 and solve(t=fresh) == -3


def test_one_handle_through_changing_m_and_n():
    import gpismap_amd
    tj = gpismap_amd.Trajectories()
    for shape in ((11, 64, 63, 2, 64), (1, 3, 1, 2, 1), (600, 64, 1, 2, 64), (11, 256, 63, 2, 64), (1, 64, 0, 1, 0), (11, 3, 255, 1, 63)):
        c = rc.shape_case(*shape)
        sc, df, dist, pl, _ = env(2)
        df.smooth(c["x"], trajectories=tj, iters=0)
        tm = tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
        for k in ("v", "t"):                             # the device's timing is the reference's
            u, w = tm[k], np.ascontiguousarray(c[k], F32)
            assert ((u.view(np.uint32) == w.view(np.uint32)) | (np.isnan(u) & np.isnan(w))).all(), (shape, k)
        _run(c, ("one handle",) + shape, ((64, 0),), tj=tj)


def test_same_schedule_on_a_callers_stream():
    import torch
    c = rc.special_cases()["batch"]
    tj, ob, got = _run(c, "own stream", ((64, 0),))
    s = torch.cuda.Stream(device=0)
    _sched_equal(_solve(tj, ob, c, stream=s.cuda_stream), got, "a caller's stream")
    _run(c, "a caller's stream", ((65, 4),), tj=tj, stream=s.cuda_stream)


def test_closed_loop_2d_on_the_device():
    """The CPU scenario of tests/test_retime_ref.py on the device: the planner's paths smoothed and timed there (four of them, as
    the reference takes), the disc aimed by the reference at the reference's trajectory; the device gives the reference's
    statuses and step counts, on its own timing the reference's every integer."""
    import gpismap_amd
    import traj_cases
    from test_retime_ref import closed_loop_input, crossing_disc
    sc, dist, x, tm = closed_loop_input()
    r = int(np.argmax(np.where(tm["status"] == 0, tm["duration"], -1)))
    disc = crossing_disc(x, tm, r)
    from test_gpu_traj import _scene
    _, df, _, pl, _ = _scene(2)
    pl.paths(traj_cases.starts(sc))
    tj = pl.trajectories(64)
    live = np.flatnonzero(tj.optimize(df, iters=0).get()["status"] != 2)[:4]
    g = df.smooth(tj.get()["x"][live], trajectories=tj).get()
    dev = tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
    ob = device_set(disc, sc["step"])
    o = dict(rc.BASE)
    got = tj.retime(ob, **o)
    mine = rr.solve(g["x"], dev["v"], dev["t"], dev["status"], disc, 0.0, o)
    _sched_equal(got, mine, "the device's own timing")
    ref = rr.solve(x, tm["v"], tm["t"], tm["status"], disc, 0.0, o)
    print("device: statuses %s arrive %s pauses %s; reference: %s %s %s" % (got["status"].tolist(), got["arrive"].tolist(), got["pauses"].tolist(),
                                                                          ref["status"].tolist(), ref["arrive"].tolist(), ref["pauses"].tolist()))
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["arrive"], ref["arrive"]) and got["status"][r] == 1
    T = int(got["arrive"][r])
    plain = tj.check(ob, o["slot"], int(got["own_slots"][r]), clearance=o["clearance"])
    k = tj.retimed_check(ob, T, clearance=o["clearance"])
    assert plain["collides"][r] == 1 and k["collides"][r] == 0 and k["min_sep"][r] >= o["clearance"]
    ctl = gpismap_amd.Controller(dt=o["slot"])
    ctl.init(2, 64, T, seed=3)
    p0, h0 = ctl.follow(tj, r, retimed=True)
    U = tj.retimed_controls(T)[0][r]
    assert np.array_equal(ctl.get()["U"].view(np.uint64), U.view(np.uint64)) and np.array_equal(p0, g["x"][r, 0].astype(F64))
