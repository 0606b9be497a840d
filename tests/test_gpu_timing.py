"""Time parametrisation and control sequences on the GPU (csrc/traj.hip, gpis_timing_*): speeds, times, limiter codes, control
sequences and the controller's seed against the numpy reference (tests/timing_ref.py), bit for bit -- every sum has one order
and a minimum has none, so there are no tolerances (a NaN equals a NaN) -- at every wavefront edge of N and T, for every option,
with and without a field, alone and at any batch position, and the error paths."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
import timing_cases as tc
import timing_ref as tr
import traj_cases
from test_gpu_traj import _dev, _field, _scene

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
TKEYS = ("v", "t", "limiter", "status", "duration", "max_speed", "max_curvature", "limiter_counts")
CKEYS = ("U", "heading0", "p0", "clamped")


def _equal(got, ref, keys, what=""):
    for k in keys:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype, u.shape, v.shape)
        if u.dtype in (F32, F64):
            w = np.uint32 if u.dtype == F32 else np.uint64
            ok = (u.view(w) == v.view(w)) | (np.isnan(u) & np.isnan(v))
        else:
            ok = u == v
        assert ok.all(), (what, k, np.argwhere(~ok)[:6].tolist(), u[~ok][:4], v[~ok][:4])


def _load(df, tj, x):
    """x as the handle's result (iters = 0: the evaluation alone); returns the result's waypoints and status."""
    g = df.smooth(x, trajectories=tj, iters=0).get()
    assert np.array_equal(g["x"].view(np.uint32), np.ascontiguousarray(x, F32).view(np.uint32))
    return g["x"], g["status"]


def _fld(sc, dist):
    return (dist, sc["shape"], sc["origin"], sc["step"])


def _cdict(c):
    return dict(zip(CKEYS, c))


def _kw(o):
    return {k: float(o[k]) for k in tr.OPT_NAMES}


# ---- time ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_time_at_every_waypoint_count(dim):
    """Every N around the wavefront edges on the shared curves -- every limiter code, a status-2 trajectory, N coincident points,
    duplicates (N = 3: status 3), waypoints inside the ball and off the lattice -- with and without the field."""
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(dim)
    tj = gpismap_amd.Trajectories()
    codes, stats = set(), set()
    for N in tc.NS:
        x, st = _load(df, tj, tc.curves(sc, N))
        for n, kw in enumerate(tc.OPT_SETS if N == 64 else (tc.OPT_SETS[0], tc.OPT_SETS[1 + tc.NS.index(N)])):
            o = tc.opts(sc, **kw)
            for field in ((df, _fld(sc, dist)), (None, None)) if n < 2 else ((df, _fld(sc, dist)),):
                got = tj.time(field[0], **_kw(o))
                _equal(got, tr.time(x, st, o, field[1]), TKEYS, (dim, N, kw, field[0] is not None))
                _equal(tj.timing(), got, TKEYS, "the getter")
            codes |= set(int(c) for c in np.unique(got["limiter"][got["status"] != 2]))
            stats |= set(int(s) for s in got["status"])
        assert tj.timing_info()["timed"] == 1
    assert codes == set(range(8)) and stats == {0, 2, 3}


@pytest.mark.parametrize("dim", [2, 3])
def test_a_trajectory_has_the_same_bits_alone_and_at_any_batch_position(dim):
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(dim)
    tj = gpismap_amd.Trajectories()
    N = 65
    base = tc.curves(sc, N)
    big = np.repeat(base[:10], 60, axis=0)
    big[:, 1:-1] += np.random.default_rng(7).normal(0, 0.3 * sc["step"], big[:, 1:-1].shape).astype(F32)
    big[::60] = base[:10]
    o = tc.opts(sc)
    x, st = _load(df, tj, big)
    whole = tj.time(df, **_kw(o))
    _equal(whole, tr.time(x, st, o, _fld(sc, dist)), TKEYS, "m=600")
    cw = _cdict(tj.controls(0.25, 33, 0.5, 0.7))
    for lo, hi in ((61, 62), (300, 307), (599, 600), (0, 1)):
        _load(df, tj, big[lo:hi])
        part = tj.time(df, **_kw(o))
        _equal(part, {k: whole[k][lo:hi] for k in TKEYS}, TKEYS, (lo, hi))
        _equal(_cdict(tj.controls(0.25, 33, 0.5, 0.7)), {k: cw[k][lo:hi] for k in CKEYS}, CKEYS, (lo, hi))


def test_planner_input_unknown_cells_and_a_field_without_sites():
    """The planner's trajectories (status 2 among them, and a path of one point: N copies) after two iterations; a field whose f
    has NaN cells; a field without sites (every distance +inf: no limit anywhere)."""
    import gpismap_amd
    for dim in (2, 3):
        sc, df, dist, pl, _ = _scene(dim)
        paths, scost, pst = pl.paths(traj_cases.starts(sc))
        off = pl.last_off.copy()
        assert ((off[1:] - off[:-1])[pst == 0] == 1).any()
        tj = pl.trajectories(64)
        o = tc.opts(sc)
        for iters in (0, 2):
            g = tj.optimize(df, iters=iters).get()
            assert (g["status"] == 2).sum() >= 3
            got = tj.time(df, **_kw(o))
            _equal(got, tr.time(g["x"], g["status"], o, _fld(sc, dist)), TKEYS, ("planner", dim, iters))
            assert np.array_equal(got["status"] == 2, g["status"] == 2) and np.isnan(got["v"][got["status"] == 2]).all()
            assert iters or (got["duration"][got["status"] == 0] == 0).any()
    sc = traj_cases.scene(2)
    f = sc["f"].copy().reshape(sc["shape"][::-1])
    f[5:20, 3:30] = np.nan
    f[30:40, 40:60] = np.nan
    df2, dist2 = _field(f.ravel(), sc["shape"], sc["origin"], sc["step"])
    tj = gpismap_amd.Trajectories()
    x, st = _load(df2, tj, tc.curves(sc, 128))
    _equal(tj.time(df2, **_kw(tc.opts(sc))), tr.time(x, st, tc.opts(sc), _fld(sc, dist2)), TKEYS, "NaN cells")
    df3, dist3 = _field(np.ones(sc["f"].size, F32), sc["shape"], sc["origin"], sc["step"])
    assert np.all(dist3 == np.inf)
    x, st = _load(df3, tj, tc.curves(sc, 129))
    got = tj.time(df3, **_kw(tc.opts(sc)))
    _equal(got, tr.time(x, st, tc.opts(sc), _fld(sc, dist3)), TKEYS, "no sites")
    _equal(got, tj.time(None, **_kw(tc.opts(sc))), TKEYS, "no sites: as without a field")
    assert not (got["limiter"] == 3).any()


def test_status_3_keeps_its_times():
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(2)
    x3, kw = tc.status3()
    tj = gpismap_amd.Trajectories()
    x, st = _load(df, tj, x3)
    o = tc.opts(sc, **kw)
    got = tj.time(df, **_kw(o))
    _equal(got, tr.time(x, st, o, _fld(sc, dist)), TKEYS, "status 3")
    assert got["status"][0] == 3 and np.isinf(got["duration"][0]) and got["t"][0, 1] == 0
    c = _cdict(tj.controls(0.5, 5))
    _equal(c, tr.controls(x, got["v"], got["t"], got["status"], 0.5, 5), CKEYS, "controls of status 3")
    assert not c["U"].any() and c["heading0"].tolist() == [[1.0, 0.0]]


# ---- controls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_controls_at_every_horizon(dim):
    """T around the wavefront edges; t0 zero, inside and past the duration; tau_k exactly on a knot (dt from the device's own
    t); the exact reversal (den = 0), the vertical first leg in 3-D, a step that does not move before the first that does,
    w_limit on and off."""
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(dim)
    tj = gpismap_amd.Trajectories()
    x, st = _load(df, tj, tc.curves(sc, 64))
    tm = tj.time(df, **_kw(tc.opts(sc)))
    _equal(tm, tr.time(x, st, tc.opts(sc), _fld(sc, dist)), TKEYS, "time")
    configs = [(0.25, 0.0, 0.0, 1e-9), (0.25, 2.0, 0.5, 1e-9), (0.25, 1000.0, 0.0, 1e-9), (0.25, 0.0, 0.5, 0.05), (0.05, 0.0, 0.0, 0.0),
               (0.5, 0.125, 2.0, 1e-9), (1.0, 0.0, 0.0, 1e-9)]
    trace = {}
    for n, T in enumerate(tc.TS):
        for dt, t0, wl, mm in (configs if T == 64 else (configs[n], configs[(n + 3) % len(configs)])):
            got = _cdict(tj.controls(dt, T, t0, wl, mm))
            ref = tr.controls(x, tm["v"], tm["t"], tm["status"], dt, T, t0, wl, mm, trace=trace)
            _equal(got, ref, CKEYS, (dim, T, dt, t0, wl, mm))
            assert np.isfinite(got["U"]).all()
    k = tc.NAMES.index("reversal")
    got = _cdict(tj.controls(0.25, 64))
    assert got["clamped"][k] >= 1 and got["clamped"].sum() == got["clamped"][k]
    assert _cdict(tj.controls(0.25, 64, 0.0, 0.5))["clamped"].sum() > got["clamped"][k]
    knots = {}
    for dt in tc.knot_dts(tm["t"], tm["status"]):
        _equal(_cdict(tj.controls(dt, 64)), tr.controls(x, tm["v"], tm["t"], tm["status"], dt, 64, trace=knots), CKEYS, ("knot", dt))
    assert knots.get("on_knot", 0) >= 4
    assert trace["past"] > 0 and trace["reversal"] > 0 and trace["still"] > 0 and trace["before_first"] > 0
    assert dim == 2 or trace["vertical"] > 0
    assert tj.timing_info()["controls_ms"] > 0


# ---- the controller's seed -----------------------------------------------------------------------------------------------------
def _peek(ptr, n):
    import gpismap_amd
    L = gpismap_amd.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(n, F64)
    assert L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 8 * n, 2) == 0              # (2: device to host)
    return out


@pytest.mark.parametrize("dim,K,T", [(2, 192, 12), (3, 128, 65)])
def test_follow_seeds_the_controller(dim, K, T):
    """follow() leaves the reference's U in the current half of the nominal sequence and nothing else: the other half, the tick and
    the seed stay (the next step equals the reference's from that Ubar at tick 1 with the same seed; q within 1 of the reference,
    everything after it exact from the device's own q)."""
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(dim)
    tj = gpismap_amd.Trajectories()
    x, st = _load(df, tj, tc.curves(sc, 64))
    tm = tj.time(df, **_kw(tc.opts(sc)))
    nu = mppi_ref.ncontrols(dim)
    seed = 11
    ctl = gpismap_amd.Controller().init(dim, K, T, seed=seed)
    A = np.random.default_rng(3).uniform(-0.2, 0.2, (T, nu))
    ctl.set_nominal(A)
    ctl.shift()
    other = ctl.device_ptrs()["U"]
    ctl.shift()
    assert ctl.device_ptrs()["U"] != other
    k, dt = tc.NAMES.index("arc"), 0.2
    ref = tr.controls(x, tm["v"], tm["t"], tm["status"], dt, T, 0.4, 0.0, 1e-9)
    p0, h0 = ctl.follow(tj, k, dt, t0=0.4)
    g = ctl.get()
    _equal(dict(U=g["U"], heading0=h0, p0=p0), dict(U=ref["U"][k], heading0=ref["heading0"][k], p0=ref["p0"][k]), ("U", "heading0", "p0"), "follow")
    assert g["U"].any() and ctl.info()["tick"] == 0 and ctl.info()["steps"] == 0 and not g["stats"]["have_step"]
    _equal(dict(U=_peek(other, T * nu).reshape(T, nu)), dict(U=mppi_ref.shift(A)), ("U",), "the other half")
    # the next step, against the reference from that Ubar
    o = mppi_ref.default_opts(dim, sc["step"])
    o["dt"] = dt
    pose = mppi_ref.pose_of_state(np.concatenate([p0, h0]), dim)
    goal = x[k, -1].astype(F64)
    u0, info = df.control(ctl, pose, goal=goal, **o)
    g2 = ctl.get()
    args = (dist, sc["shape"], sc["origin"], sc["step"], pose, g["U"], seed, 1)
    r = mppi_ref.roll(*args, K, o, None, goal)
    _equal(dict(J=g2["J"]), dict(J=r["J"]), ("J",), "J")
    dq = np.abs(g2["q"].astype(np.int64) - r["q"].astype(np.int64))
    assert dq.max() <= 1 and np.array_equal(g2["hits"], r["hits"])
    f = mppi_ref.finish(r, g2["q"], *args, o, None, goal)
    _equal(dict(U=g2["U"], u0=u0, ns=g2["nominal_states"]), dict(U=f["U"], u0=f["u0"], ns=f["nominal_states"]), ("U", "u0", "ns"), "step")
    assert ctl.info()["tick"] == 1


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_timing_and_nominal_sequence():
    import gpismap_amd
    L = gpismap_amd.lib()
    sc, df, dist, pl, _ = _scene(2)
    sc3, df3, _, _, _ = _scene(3)
    tj = gpismap_amd.Trajectories()
    x, st = _load(df, tj, tc.curves(sc, 20))
    o = tc.opts(sc)
    ref = tr.time(x, st, o, _fld(sc, dist))
    _equal(tj.time(df, **_kw(o)), ref, TKEYS, "first")

    def time(traj=None, field=df, **kw):
        oo = gpismap_amd.timing_opts(2, F32(sc["step"]), **kw)
        return L.gpis_timing_time(tj.h if traj is None else traj, field.h if field is not None else None, C.byref(oo), None)

    nan, inf = float("nan"), float("inf")
    for kw in [dict(v_max=0.0), dict(v_max=-1.0), dict(v_max=nan), dict(v_max=inf), dict(v_min=0.0), dict(v_min=1.5), dict(v_min=nan),
               dict(a_max=0.0), dict(a_max=inf), dict(d_max=0.0), dict(d_max=nan), dict(a_lat=-0.1), dict(a_lat=inf), dict(w_max=-0.1),
               dict(w_max=nan), dict(v_start=-0.1), dict(v_start=inf), dict(v_end=-0.1), dict(v_end=nan), dict(clearance=nan),
               dict(clearance=inf), dict(slow_dist=-0.1), dict(slow_dist=inf)]:
        assert time(**kw) == -1, kw
    assert L.gpis_timing_time(tj.h, df.h, None, None) == -1 and L.gpis_timing_time(None, df.h, C.byref(gpismap_amd.timing_opts(2, 0.25)), None) == -1
    assert time(field=df3) == -1                          # a field of another dim
    assert time(field=gpismap_amd.DistanceField()) == -3  # a field without a result
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    U = np.zeros((len(st), 4, 2), F64)
    for a in [(0.0, 4, 0.0, 0.0, 0.0), (-1.0, 4, 0.0, 0.0, 0.0), (nan, 4, 0.0, 0.0, 0.0), (inf, 4, 0.0, 0.0, 0.0), (0.1, 0, 0.0, 0.0, 0.0),
              (0.1, 257, 0.0, 0.0, 0.0), (0.1, -3, 0.0, 0.0, 0.0), (0.1, 4, -0.5, 0.0, 0.0), (0.1, 4, nan, 0.0, 0.0), (0.1, 4, 0.0, -1.0, 0.0),
              (0.1, 4, 0.0, inf, 0.0), (0.1, 4, 0.0, 0.0, -1.0), (0.1, 4, 0.0, 0.0, nan)]:
        assert L.gpis_timing_controls(tj.h, a[0], a[1], a[2], a[3], a[4], dp(U), None, None, None) == -1, a
    assert not U.any()
    # the controller's seed
    ctl = gpismap_amd.Controller()
    follow = lambda c=ctl, t=tj, i=0, dt=0.1, t0=0.0, wl=0.0, mm=0.0: L.gpis_timing_follow(c.h, t.h, i, dt, t0, wl, mm, None, None)
    assert follow() == -3                                 # not initialised
    ctl.init(2, 64, 8, seed=5)
    A = np.random.default_rng(1).uniform(-0.1, 0.1, (8, 2))
    ctl.set_nominal(A)
    assert L.gpis_timing_follow(None, tj.h, 0, 0.1, 0.0, 0.0, 0.0, None, None) == -1
    assert L.gpis_timing_follow(ctl.h, None, 0, 0.1, 0.0, 0.0, 0.0, None, None) == -1
    assert follow(i=-1) == -1 and follow(i=len(st)) == -1 and follow(dt=0.0) == -1 and follow(dt=nan) == -1 and follow(t0=-1.0) == -1
    assert follow(wl=-1.0) == -1 and follow(mm=-1.0) == -1
    assert follow(i=tc.NAMES.index("nan")) == -3          # timing status 2
    ctl3 = gpismap_amd.Controller().init(3, 64, 8)
    assert follow(c=ctl3) == -1                           # another dim
    fresh = gpismap_amd.Trajectories()
    assert follow(t=fresh) == -3 and fresh.timing_info()["timed"] == 0
    assert L.gpis_timing_get(fresh.h, *[None] * 8) == -3 and L.gpis_timing_controls(fresh.h, 0.1, 4, 0.0, 0.0, 0.0, None, None, None, None) == -3
    fresh.set(x)
    assert L.gpis_timing_time(fresh.h, df.h, C.byref(gpismap_amd.timing_opts(2, 0.25)), None) == -3     # an input, but no result
    with pytest.raises(gpismap_amd.GpisError):
        fresh.timing()
    with pytest.raises(gpismap_amd.GpisError):
        fresh.controls(0.1, 4)
    _equal(dict(U=ctl.get()["U"]), dict(U=A), ("U",), "the nominal sequence after the errors")
    _equal(tj.timing(), ref, TKEYS, "the timing after the errors")
    # status 3 cannot seed either
    x3, kw = tc.status3()
    t3 = gpismap_amd.Trajectories()
    _load(df, t3, x3)
    assert t3.time(df, **kw)["status"][0] == 3 and follow(t=t3) == -3
    _equal(dict(U=ctl.get()["U"]), dict(U=A), ("U",), "the nominal sequence after status 3")
    assert follow() == 0 and ctl.get()["U"].any()
    # a new result drops the timing
    tj.optimize(df, iters=1)
    assert tj.timing_info()["timed"] == 0 and L.gpis_timing_get(tj.h, *[None] * 8) == -3 and follow() == -3
    _load(df, tj, x)
    _equal(tj.time(df, **_kw(o)), ref, TKEYS, "again")


# ---- one long-lived handle ------------------------------------------------------------------------------------------------------
def test_one_handle_through_changing_shapes():
    """(dim, N, m, T) small -> larger in every capacity -> the degenerate branch (m = 1, N = 3, T = 1) -> the other dimension ->
    the first again: after every call every output equals that of a fresh handle given only that call, and the last call equals
    the first."""
    import gpismap_amd
    old = gpismap_amd.Trajectories()
    outs = []
    for dim, N, m, T in ((2, 8, 3, 4), (2, 200, 40, 100), (2, 3, 1, 1), (3, 64, 7, 16), (2, 8, 3, 4)):
        sc, df, dist, pl, _ = _scene(dim)
        base = tc.curves(sc, N)
        x = np.concatenate([base] * (m // len(base) + 1))[:m]
        o = tc.opts(sc, v_start=0.2)
        res = []
        for tj in (old, gpismap_amd.Trajectories()):
            _load(df, tj, x)
            tm = tj.time(df, **_kw(o))
            res.append((tm, _cdict(tj.controls(0.3, T, 0.1, 0.8)), tj.get()))
        _equal(res[0][0], res[1][0], TKEYS, (dim, N, m, T))
        _equal(res[0][1], res[1][1], CKEYS, (dim, N, m, T))
        assert res[0][0]["v"].shape == (m, N) and res[0][1]["U"].shape == (m, T, 4 if dim == 3 else 2)
        assert np.array_equal(res[0][2]["x"].view(np.uint32), res[1][2]["x"].view(np.uint32))
        outs.append(res[0])
    _equal(outs[-1][0], outs[0][0], TKEYS, "the last call equals the first")
    _equal(outs[-1][1], outs[0][1], CKEYS, "the last call equals the first")
