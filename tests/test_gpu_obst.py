"""Moving obstacles on the GPU (csrc/obst.hip, the OBST kernels of csrc/mppi.hip, traj_obst_check_kernel of csrc/traj.hip,
gpis_obst_*) against the numpy reference (tests/obst_ref.py), stage by stage as tests/test_gpu_mppi.py does: after every call the
reference is fed the device's state from before that call.  J, hits, dyn_hits, min_sep and the nominal states are compared as
bits; the weights q may differ by 1 (the one exp); everything after q is computed from the device's q and compared exactly.
The check of timed trajectories is compared on the device's own timing: its two doubles as bits (a NaN equals a NaN), its three
integers as integers."""
import ctypes as C

import numpy as np
import pytest

import mppi_cases as mc
import mppi_ref
import obst_cases as oc
import obst_ref
import timing_cases as tc
import timing_ref
from test_gpu_mppi import _b, _dev, _same_bits, env
from test_mppi_ref import LOOP2

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U64 = np.uint64


def device_set(S, step=None):
    """An Obstacles holding the reference's set S, read back and compared."""
    import gpismap_amd
    ob = gpismap_amd.Obstacles(S["dim"], mc.scene(S["dim"])["step"] if step is None else step, **S["opts"])
    ob.set(S["c"], S["v"], S["r"], epoch=S["epoch"])
    g, i = ob.get(), ob.info()
    _same_bits(g["centre"], S["c"], "centres")
    _same_bits(g["velocity"], S["v"], "velocities")
    _same_bits(g["radius"], S["r"], "radii")
    assert (i["inited"], i["dim"], i["n"], i["epoch"]) == (1, S["dim"], S["n"], S["epoch"]) and g["opts"] == S["opts"]
    return ob


class Checked:
    """A Controller whose every step with a set is checked against obst_ref fed with the device's state from before the call."""

    def __init__(self, c, stream=None, ctl=None, env_=None):
        import gpismap_amd
        self.c, self.dim, self.K, self.T, self.seed, self.tick = c, c["dim"], c["K"], c["T"], c["seed"], 0
        # env_: (lattice dict, field, its dist flat, planner, its cost flat) of another scene in env(dim)'s place
        self.sc, self.df, self.dist, self.pl, self.cost = env(self.dim) if env_ is None else env_
        self.stream = stream
        self.ctl = ctl if ctl is not None else gpismap_amd.Controller()
        self.ctl.init(self.dim, self.K, self.T, seed=self.seed)
        assert self.ctl.obstacle_stats() == dict(dyn_hit_rollouts=0, nominal_dyn_hits=0, nominal_min_sep=np.inf, n=0)
        self.ob = device_set(c["obst"], self.sc["step"])
        self.q_off = 0

    def step(self, t_now=None):
        c = self.c
        S = c["obst"]
        t_now = c["t_now"] if t_now is None else t_now
        o = c["opts"]
        plan = c["terminal"] == "plan"
        cost, goal = (self.cost, None) if plan else (None, self.sc["goal_point"])
        before = self.ctl.get()
        u0, info = self.df.control(self.ctl, c["pose"], goal=goal, planner=self.pl if plan else None, stream=self.stream, obstacles=self.ob,
                                   t=t_now, **o)
        self.tick += 1
        g, go, so = self.ctl.get(), self.ctl.get_obstacle(), self.ctl.obstacle_stats()
        what = "dim %d K %d T %d n %d tick %d" % (self.dim, self.K, self.T, S["n"], self.tick)
        args = (self.dist, self.sc["shape"], self.sc["origin"], self.sc["step"], c["pose"], before["U"], self.seed, self.tick)
        r = obst_ref.roll(*args, self.K, o, cost, goal, obst=S, t_now=t_now)
        _same_bits(g["J"], r["J"], "J, " + what)
        assert np.array_equal(g["hits"], r["hits"]), what
        assert np.array_equal(go["dyn_hits"], r["dyn_hits"]), what
        _same_bits(go["min_sep"], r["min_sep"], "min_sep, " + what)
        assert _b(info["Jmin"]) == _b(r["Jmin"]) and info["best"] == r["best"], (what, info, r["Jmin"], r["best"])
        q = g["q"]
        dq = np.abs(q.astype(np.int64) - r["q"].astype(np.int64))
        self.q_off += int(np.count_nonzero(dq))
        assert dq.max() <= 1, "%s: q differs from the reference's at %d of %d rollouts, by up to %d" % (what, np.count_nonzero(dq), self.K, dq.max())
        f = obst_ref.finish(r, q, *args, o, cost, goal, obst=S, t_now=t_now)
        assert (info["T"], info["Th"], info["S2"], info["hits"]) == (f["T"], f["Th"], f["S2"], f["nhit"]), (what, info)
        assert _b(info["neff"]) == _b(f["neff"]), (what, info["neff"], f["neff"])
        _same_bits(g["U"], f["U"], "the new sequence, " + what)
        _same_bits(u0, f["u0"], "u0, " + what)
        _same_bits(g["nominal_states"], f["nominal_states"], "nominal states, " + what)
        assert _b(info["nominal_cost"]) == _b(f["nominal_cost"]) and info["nominal_hits"] == f["nominal_hits"], (what, info, f["nominal_cost"])
        assert (so["dyn_hit_rollouts"], so["nominal_dyn_hits"], so["n"]) == (f["ndyn"], f["nominal_dyn_hits"], S["n"]), (what, so, f["ndyn"])
        assert _b(so["nominal_min_sep"]) == _b(f["nominal_min_sep"]), (what, so, f["nominal_min_sep"])
        i = self.ctl.info()
        assert i["tick"] == self.tick and i["steps"] == self.tick
        return u0, info, r

    def shift(self):
        before = self.ctl.get()["U"]
        self.ctl.shift()
        _same_bits(self.ctl.get()["U"], mppi_ref.shift(before), "shift")


def _two_steps(c):
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    _, _, r = ck.step()
    ck.shift()
    ck.step(c["t_now"] + c["opts"]["dt"])
    return ck, r


# ---- the set itself -------------------------------------------------------------------------------------------------------------
def test_set_get_at_and_its_errors():
    import gpismap_amd
    L = gpismap_amd.lib()
    S = oc.balls(3, 65, 0.2)
    ob = device_set(S)
    for t in (S["epoch"], 0.0, 7.3, -2.0e9):
        _same_bits(ob.at(t), obst_ref.at(S, t), "at %r" % t)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))

    def still_there(what):
        g = ob.get()
        _same_bits(g["centre"], S["c"], what)
        _same_bits(g["velocity"], S["v"], what)
        _same_bits(g["radius"], S["r"], what)
        assert ob.info()["n"] == 65 and ob.info()["epoch"] == S["epoch"] and g["opts"] == S["opts"], what

    c, v, r = S["c"][:4].copy(), S["v"][:4].copy(), S["r"][:4].copy()
    bad = lambda a, idx, val: (lambda b: (b.__setitem__(idx, val), b)[1])(a.copy())
    calls = dict(null=(None, 3, 4, c, v, r, 0.0), dim=(ob.h, 4, 4, c, v, r, 0.0), neg_n=(ob.h, 3, -1, c, v, r, 0.0),
                 nan_c=(ob.h, 3, 4, bad(c, (2, 1), np.nan), v, r, 0.0), inf_v=(ob.h, 3, 4, c, bad(v, (0, 0), np.inf), r, 0.0),
                 neg_r=(ob.h, 3, 4, c, v, bad(r, 3, -1e-9), 0.0), nan_r=(ob.h, 3, 4, c, v, bad(r, 0, np.nan), 0.0),
                 inf_epoch=(ob.h, 3, 4, c, v, r, np.inf), no_c=(ob.h, 3, 4, None, v, r, 0.0))
    for name, (h, dim, n, cc, vv, rr, ep) in calls.items():
        assert L.gpis_obst_set(h, dim, n, dp(cc), dp(vv), dp(rr), ep) == -1, name
        still_there(name)
    z = np.zeros((257, 3))
    assert L.gpis_obst_set(ob.h, 3, 257, dp(z), dp(z), dp(z[:, 0]), 0.0) == -4
    still_there("n > 256")
    for kw in (dict(clearance=-0.1), dict(margin=np.nan), dict(w_obs=-1.0), dict(w_col=np.inf)):
        o = gpismap_amd.gpis_obst_opts(**dict(S["opts"], **kw))
        assert L.gpis_obst_set_opts(ob.h, C.byref(o)) == -1 and L.gpis_obst_set_opts(None, C.byref(o)) == -1
        still_there(str(kw))
    assert L.gpis_obst_set_opts(ob.h, None) == -1 and L.gpis_obst_at(ob.h, np.nan, dp(np.zeros(195))) == -1
    assert L.gpis_obst_info(None, dp(np.zeros(5)), 5) == -1 and L.gpis_obst_get(None, None, None, None, None) == -1
    # n = 0 empties the set; 256 balls fit
    ob.set(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), epoch=1.0)
    assert ob.info()["n"] == 0 and ob.at(2.0).shape == (0, 3)
    device_set(oc.balls(2, 256, 0.25))


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,n", oc.SHAPES)
def test_stages_2d_every_shape(K, T, n):
    """Two steps with a shift between them, the clock moved on by dt."""
    ck, r = _two_steps(oc.shape_case(K, T, n))
    if K >= 63 and T >= 33:
        br = r["branches"]
        assert br["dyn_col"] and br["dyn_band"] and (n > 2 or br["dyn_free"]), br      # (among many balls one is always near)
    print("K %d T %d n %d: q off by one at %d rollout-steps of %d" % (K, T, n, ck.q_off, 2 * K))


@pytest.mark.parametrize("K,T,n", oc.SHAPES3)
def test_stages_3d(K, T, n):
    _two_steps(oc.shape_case(K, T, n, 3))


# ---- identity -------------------------------------------------------------------------------------------------------------------
def test_no_set_and_an_empty_set_are_the_plain_step():
    """obstacles=None through gpis_mppi_step, a NULL set and a set with n = 0 through gpis_obst_mppi_step: every output of get()
    has the bits of a second controller of the same seed stepped without obstacles, over two steps."""
    import gpismap_amd
    L = gpismap_amd.lib()
    c = mc.shape_case(1000, 33)
    sc, df, dist, pl, cost = env(2)
    empty = gpismap_amd.Obstacles(2, sc["step"])
    empty.set(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
    never = gpismap_amd.Obstacles(2, sc["step"])          # never set at all
    dp = lambda a: np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))

    def run(how):
        ctl = gpismap_amd.Controller()
        ctl.init(2, c["K"], c["T"], seed=c["seed"])
        ctl.set_nominal(mc.nominal_of(c))
        out = []
        for n in range(2):
            if how == "plain":
                u0, info = df.control(ctl, c["pose"], planner=pl, **c["opts"])
            elif how == "null":
                u0 = np.zeros(2)
                o = gpismap_amd.mppi_opts(2, sc["step"], **c["opts"])
                assert L.gpis_obst_mppi_step(ctl.h, df.h, pl.h, None, 3.0 + n, dp(c["pose"]), None, C.byref(o), dp(u0), None) == 0
                info = ctl.stats()
            else:
                u0, info = df.control(ctl, c["pose"], planner=pl, obstacles=how, t=3.0 + n, **c["opts"])
            g = ctl.get()
            go, so = ctl.get_obstacle(), ctl.obstacle_stats()
            assert not go["dyn_hits"].any() and np.all(np.isposinf(go["min_sep"]))
            assert so == dict(dyn_hit_rollouts=0, nominal_dyn_hits=0, nominal_min_sep=np.inf, n=0)
            out.append(dict(g, u0=u0, tick=ctl.info()["tick"]))
            ctl.shift()
        return out

    base = run("plain")
    for how in ("null", empty, never):
        for a, b in zip(base, run(how)):
            assert a["stats"] == b["stats"] and a["tick"] == b["tick"]
            for k in ("U", "J", "nominal_states", "u0"):
                _same_bits(a[k], b[k], k)
            assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["hits"], b["hits"])


def test_a_plain_step_after_a_step_with_balls_reports_none():
    c = oc.branch_cases()["crossing"]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    ck.step()
    assert ck.ctl.obstacle_stats()["n"] == 1 and ck.ctl.get_obstacle()["dyn_hits"].any()
    ck.df.control(ck.ctl, c["pose"], planner=ck.pl, **c["opts"])
    assert ck.ctl.obstacle_stats() == dict(dyn_hit_rollouts=0, nominal_dyn_hits=0, nominal_min_sep=np.inf, n=0)
    assert not ck.ctl.get_obstacle()["dyn_hits"].any()


# ---- branches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(oc.branch_cases()))
def test_branch(name):
    c = oc.branch_cases()[name]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    _, info, r = ck.step()
    for e in c["expect"]:
        assert r["branches"].get(e, 0) > 0, (name, e, r["branches"])      # asserted, not assumed
    assert ck.ctl.obstacle_stats()["dyn_hit_rollouts"] > 0 and ck.ctl.get_obstacle()["dyn_hits"].max() > 0
    ck.shift()
    ck.step(c["t_now"] + c["opts"]["dt"])


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
def _run(c, stream=None):
    import gpismap_amd
    sc, df, dist, pl, cost = env(c["dim"])
    ob = device_set(c["obst"])
    ctl = gpismap_amd.Controller()
    ctl.init(c["dim"], c["K"], c["T"], seed=c["seed"])
    ctl.set_nominal(mc.nominal_of(c))
    out = []
    for n in range(2):
        u0, info = df.control(ctl, c["pose"], planner=pl, stream=stream, obstacles=ob, t=c["t_now"] + n * c["opts"]["dt"], **c["opts"])
        g = ctl.get()
        g.pop("stats")
        g.update(ctl.get_obstacle())
        out.append(dict(g, u0=u0, cost=np.float64(info["nominal_cost"]), sep=np.float64(ctl.obstacle_stats()["nominal_min_sep"])))
        ctl.shift()
    return out


def test_same_bits_on_a_callers_stream_and_on_the_own_stream():
    import torch
    c = oc.shape_case(1000, 33, 65)
    a = _run(c)
    eq = lambda x, y: all(np.array_equal(np.ascontiguousarray(p[k]).view(np.uint8), np.ascontiguousarray(q[k]).view(np.uint8)) for p, q in zip(x, y) for k in p)
    assert eq(a, _run(c))
    s = torch.cuda.Stream(device=0)
    assert eq(a, _run(c, stream=C.c_void_p(s.cuda_stream)))
    assert not eq(a, _run(dict(c, seed=6)))


def test_rollouts_depend_on_seed_tick_and_index_alone():
    a, b = Checked(oc.shape_case(257, 33, 65)), Checked(oc.shape_case(1000, 33, 65))
    for ck in (a, b):
        ck.ctl.set_nominal(mc.nominal_of(ck.c))
        ck.step()
    _same_bits(a.ctl.get()["J"], b.ctl.get()["J"][:257], "the first 257 of 1000")
    _same_bits(a.ctl.get_obstacle()["min_sep"], b.ctl.get_obstacle()["min_sep"][:257], "min_sep of the first 257 of 1000")


# ---- lifetime and errors ----------------------------------------------------------------------------------------------------------
def test_a_set_changed_and_destroyed_between_steps():
    import gpismap_amd
    c = oc.branch_cases()["crossing"]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    ck.step()
    ck.shift()
    # another set in the same handle
    S2 = oc.balls(2, 64, 0.25, w_col=50.0)
    ck.ob.set(S2["c"], S2["v"], S2["r"], epoch=S2["epoch"])
    ck.ob.set_opts(**S2["opts"])
    ck.c = dict(c, obst=S2)
    ck.step()
    ck.shift()
    # the handle destroyed, a new one in its place
    ck.ob.close()
    S3 = oc.balls(2, 2, 0.25)
    ck.ob = device_set(S3)
    ck.c = dict(c, obst=S3)
    ck.step()
    ck.ob.close()
    ck.df.control(ck.ctl, c["pose"], planner=ck.pl, **c["opts"])      # and on without one
    assert ck.ctl.info()["tick"] == 4


def test_errors_leave_the_state():
    import gpismap_amd
    L = gpismap_amd.lib()
    sc, df, dist, pl, cost = env(2)
    sc3, df3, _, pl3, _ = env(3)
    c = oc.branch_cases()["crossing"]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    ck.step()
    ctl, ob = ck.ctl, ck.ob
    ob3 = device_set(oc.balls(3, 2, 0.2))
    a, ia, ga, sa = ctl.get(), ctl.info(), ctl.get_obstacle(), ctl.obstacle_stats()
    dp = lambda a: None if a is None else np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))

    def step(ctl_h=ctl, f=df, p=pl, o=ob, t=3.5, pose=c["pose"], g=None, **kw):
        mo = gpismap_amd.mppi_opts(2, sc["step"], **kw)
        return L.gpis_obst_mppi_step(ctl_h.h if ctl_h is not None else None, f.h if f is not None else None, p.h if p is not None else None,
                                     o.h if o is not None else None, t, dp(pose), dp(g), C.byref(mo), None, None)

    def still_there(what):
        b = ctl.get()
        assert ctl.info() == ia and b["stats"] == a["stats"] and ctl.obstacle_stats() == sa, what
        for k in ("U", "J", "nominal_states"):
            _same_bits(b[k], a[k], what + ": " + k)
        assert np.array_equal(b["q"], a["q"]) and np.array_equal(b["hits"], a["hits"]), what
        go = ctl.get_obstacle()
        assert np.array_equal(go["dyn_hits"], ga["dyn_hits"]), what
        _same_bits(go["min_sep"], ga["min_sep"], what + ": min_sep")

    bad_pose = c["pose"].copy(); bad_pose[1] = np.nan
    arg = dict(other_dim=dict(o=ob3), t_nan=dict(t=np.nan), t_inf=dict(t=-np.inf), t_nan_no_set=dict(o=None, t=np.nan), no_field=dict(f=None),
               nan_pose=dict(pose=bad_pose), both=dict(g=sc["goal_point"]), neither=dict(p=None), dim_field=dict(f=df3), dim_plan=dict(p=pl3),
               dt0=dict(dt=0.0), lam0=dict(lam=0.0), w_neg=dict(w_obs=-1.0), margin_neg=dict(margin=-0.1))
    for name, kw in arg.items():
        assert step(**kw) == -1, name
        still_there(name)
    assert step(ctl_h=None) == -1 and step(f=gpismap_amd.DistanceField()) == -3 and step(p=gpismap_amd.Planner()) == -3
    still_there("a field and a planner without a result")
    fresh = gpismap_amd.Controller()
    assert step(ctl_h=fresh) == -3 and L.gpis_obst_mppi_get(fresh.h, None, None, None) == -3 and L.gpis_obst_mppi_get(None, None, None, None) == -1
    # the set offered to a handle of another dim is untouched, and so is that handle
    ctl3 = gpismap_amd.Controller()
    ctl3.init(3, 64, 4, seed=2)
    df3.control(ctl3, mc.FREE3, planner=pl3)
    b3 = ctl3.get()
    with pytest.raises(gpismap_amd.GpisError):
        df3.control(ctl3, mc.FREE3, planner=pl3, obstacles=ob, t=1.0)
    assert ctl3.info()["tick"] == 1
    _same_bits(ctl3.get()["U"], b3["U"], "the 3-D controller's sequence")
    _same_bits(ob.get()["centre"], c["obst"]["c"], "the set")
    # after the errors both work
    ck.shift()
    ck.step(4.0)
    df3.control(ctl3, mc.FREE3, planner=pl3, obstacles=ob3, t=1.0)
    assert ctl3.info()["tick"] == 2 and ctl3.obstacle_stats()["n"] == 2


# ---- timed trajectories against a set ---------------------------------------------------------------------------------------
CHECK_KEYS = ("min_sep", "min_time", "min_obstacle", "first_hit", "collides")


def _check_equal(got, ref, what):
    for k in CHECK_KEYS:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype, u.shape, v.shape)
        ok = (u.view(U64) == v.view(U64)) | (np.isnan(u) & np.isnan(v)) if u.dtype == F64 else u == v
        assert ok.all(), (what, k, np.argwhere(~ok)[:6].tolist(), u[~ok][:4], v[~ok][:4])


def _timed(c):
    """The case's trajectories in a handle, timed on the device with the case's own options; the device's timing is held to the
    reference's bits (the case's v and t), which the sets of the special cases were aimed with."""
    import gpismap_amd
    dim = c["x"].shape[2]
    sc, df, dist, pl, _ = env(dim)
    tj = gpismap_amd.Trajectories()
    g = df.smooth(c["x"], trajectories=tj, iters=0).get()
    assert np.array_equal(g["x"].view(np.uint32), np.ascontiguousarray(c["x"], F32).view(np.uint32))
    tm = tj.time(df, **{k: float(tc.opts(sc)[k]) for k in timing_ref.OPT_NAMES})
    assert np.array_equal(tm["status"], c["status"])
    for k in ("v", "t"):
        u, v = tm[k], np.ascontiguousarray(c[k], F32)
        assert ((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all(), k
    return tj


def _run_check(c, what):
    tj = _timed(c)
    ob = device_set(c["obst"])
    got = tj.check(ob, c["dt"], c["steps"], t0=c["t0"], t_begin=c["t_begin"], clearance=c["clearance"])
    ref = oc.ref_check(c)
    _check_equal(got, ref, what)
    return got, tj, ob


@pytest.mark.parametrize("m,N,steps,n", oc.CHECK_SHAPES + (oc.CHECK_LONG,))
def test_check_2d_every_shape(m, N, steps, n):
    got, _, _ = _run_check(oc.check_shape_case(m, N, steps, n), (m, N, steps, n))
    print("m %d N %d steps %d n %d: %d collide, least separation %.3f" % (m, N, steps, n, got["collides"].sum(), np.nanmin(got["min_sep"])))


@pytest.mark.parametrize("m,N,steps,n", oc.CHECK_SHAPES3)
def test_check_3d(m, N, steps, n):
    _run_check(oc.check_shape_case(m, N, steps, n, dim=3), (3, m, N, steps, n))


@pytest.mark.parametrize("name", sorted(oc.special_check_cases()))
def test_check_special(name):
    import gpismap_amd
    c = oc.special_check_cases()[name]
    got, tj, ob = _run_check(c, name)
    for k in ("collides", "first_hit"):
        if k in c["expect"]:
            assert int(got[k][0]) == c["expect"][k], (name, k, got[k])
    if name == "status23":
        assert set(c["status"].tolist()) == {0, 2, 3}
        ob.set(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        _check_equal(tj.check(ob, c["dt"], c["steps"], t_begin=c["t_begin"]), oc.ref_check(dict(c, obst=obst_ref.make(2, [], [], []))), "n = 0")


def test_check_errors_leave_the_timing():
    import gpismap_amd
    L = gpismap_amd.lib()
    c = oc.special_check_cases()["resting"]
    got, tj, ob = _run_check(c, "resting")
    ob3 = device_set(oc.balls(3, 2, 0.2))
    before = tj.timing()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = dict(min_sep=np.full(1, 7.0), min_time=np.full(1, 7.0), min_obstacle=np.full(1, 7, np.int32), first_hit=np.full(1, 7, np.int32),
               collides=np.full(1, 7, np.int32))

    def check(t=tj, o=ob, dt=0.5, steps=8, t0=0.0, tb=0.0, clr=0.1):
        return L.gpis_obst_check_timing(t.h if t is not None else None, o.h if o is not None else None, dt, steps, t0, tb, clr,
                                        dp(out["min_sep"]), dp(out["min_time"]), ip(out["min_obstacle"]), ip(out["first_hit"]), ip(out["collides"]))

    arg = dict(no_traj=dict(t=None), no_set=dict(o=None), steps0=dict(steps=0), steps_many=dict(steps=4097), dt0=dict(dt=0.0), dt_neg=dict(dt=-1.0),
               dt_nan=dict(dt=np.nan), t0_neg=dict(t0=-0.1), t0_inf=dict(t0=np.inf), tb_nan=dict(tb=np.nan), clr_neg=dict(clr=-0.1),
               clr_inf=dict(clr=np.inf), other_dim=dict(o=ob3))
    for name, kw in arg.items():
        assert check(**kw) == -1, name
        assert all(np.all(v == 7) for v in out.values()), name
    untimed = gpismap_amd.Trajectories()
    assert check(t=untimed) == -3
    env(2)[1].smooth(c["x"], trajectories=untimed, iters=0)
    assert check(t=untimed) == -3                            # a result without a timing
    after = tj.timing()
    for k in before:
        assert np.array_equal(np.ascontiguousarray(before[k]).view(np.uint8), np.ascontiguousarray(after[k]).view(np.uint8)), k
    assert check(steps=4096) == 0 and out["collides"][0] == 1
    _check_equal(tj.check(ob, c["dt"], c["steps"], clearance=c["clearance"]), got, "again")


# ---- closed loop ----------------------------------------------------------------------------------------------------------------
def test_closed_loop_2d_with_a_crossing_disc_on_the_device():
    """The CPU scenario of tests/test_obst_ref.py through Controller, with its acceptance: behaviour, not bits (a q may differ by
    one from the reference's own run).  The disc goes through the device's own unaware run's position of step 30."""
    import gpismap_amd
    sc, df, dist, pl, cost = env(2)

    def loop(obstacles, track=None):
        ctl = gpismap_amd.Controller(**LOOP2["opts"])
        ctl.init(2, LOOP2["K"], LOOP2["T"], seed=LOOP2["seed"])

        def step_fn(pose, t):
            u0, _ = df.control(ctl, pose, planner=pl, obstacles=obstacles, t=t)
            ctl.shift()
            return u0

        return oc.closed_loop(LOOP2, step_fn=step_fn, track=track)

    unaware = loop(None)
    ball = oc.crossing_ball(LOOP2, unaware["states"], 0.3, 0.4)
    unaware["sep"] = oc.least_separation(LOOP2, unaware["states"], ball)
    aware = loop(device_set(ball), track=ball)
    for name, r in (("without the set", unaware), ("with the set", aware)):
        print("%s: %s steps, least field distance %.3f, least separation %.3f, %.3f from the goal" % (name, r["steps"], r["least"], r["sep"], r["e"]))
    assert unaware["sep"] < 0
    assert aware["sep"] >= ball["opts"]["clearance"]
    assert aware["steps"] is not None and aware["steps"] <= LOOP2["budget"] and aware["e"] <= 2 * sc["step"]
    assert aware["least"] >= mc.opts(2)["clearance"]
