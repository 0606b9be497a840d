"""The sampling controller on the GPU (csrc/mppi.hip, gpis_mppi_*) against the numpy reference (tests/mppi_ref.py), stage by
stage: after every call the reference is fed the device's state from before that call.  Everything is compared as bits except
the weights q, where the one inexact step (exp, within 1 ulp on either side; 2^32 * 2^-51 < 1) allows a difference of 1; every
later stage is computed from the device's own q and compared exactly.  The shapes cover the last workgroup of the rollouts, one
and several segments of the update's tree, its zero-padded top and the longest horizon; then every branch of the cost (asserted
in the reference, not assumed), two steps with a shift, set_nominal, streams, the closed loop, the error paths and a run on a
field that never saw a map."""
import ctypes as C

import numpy as np
import pytest

import mppi_cases as mc
import mppi_ref
from test_mppi_ref import LOOP2, closed_loop

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U64 = np.uint64
_ENV = {}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a.view(U64).ravel() != b.view(U64).ravel())
    assert bad.size == 0, (what, "%d differ, first at %s: %r against %r" % (bad.size, bad[:8], a.ravel()[bad[:3]], b.ravel()[bad[:3]]))


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def env(dim):
    """(scene, field, its distances, planner, its cost-to-go) of mppi_cases.scene(dim) on the device, built once; the field
    comes from from_grid alone (no map), and its distances and the planner's costs are the references' bits."""
    if dim not in _ENV:
        import gpismap_amd
        import traj_cases
        sc = mc.scene(dim)
        df = gpismap_amd.DistanceField()
        df.from_grid(_dev(np.ascontiguousarray(sc["f"], F32).ravel()).data_ptr(), sc["shape"], sc["origin"], sc["step"], 0.0)
        dist = df.get()[0].ravel()
        pl = df.plan([traj_cases.world(sc, sc["goal"])], planner=gpismap_amd.Planner(), clearance=0.0, margin=4 * sc["step"], gain=4.0)
        cost = pl.get()[0].ravel()
        assert np.array_equal(dist.view(np.uint32), sc["dist"].view(np.uint32)) and np.array_equal(cost.view(np.uint32), sc["cost"].view(np.uint32))
        _ENV[dim] = (sc, df, dist, pl, cost)
    return _ENV[dim]


class Checked:
    """A Controller (a new one, or `ctl`: one that has served other calls and is initialised again here) whose every call is
    checked against the reference fed with the device's state from before the call."""

    def __init__(self, c, stream=None, ctl=None, env_=None):
        import gpismap_amd
        self.c, self.dim, self.K, self.T, self.seed, self.tick = c, c["dim"], c["K"], c["T"], c["seed"], 0
        # env_: (lattice dict, field, its dist flat, planner, its cost flat) of another scene in env(dim)'s place
        self.sc, self.df, self.dist, self.pl, self.cost = env(self.dim) if env_ is None else env_
        self.stream = stream
        self.ctl = ctl if ctl is not None else gpismap_amd.Controller()
        self.ctl.init(self.dim, self.K, self.T, seed=self.seed)
        g = self.ctl.get()
        assert not g["U"].any() and not g["J"].any() and not g["q"].any() and not g["hits"].any() and not g["stats"]["have_step"]
        i = self.ctl.info()
        assert (i["inited"], i["dim"], i["rollouts"], i["horizon"], i["tick"], i["steps"]) == (1, self.dim, self.K, self.T, 0, 0)
        self.q_off = 0
        self.branches = {}

    def set_nominal(self, U):
        self.ctl.set_nominal(U)
        _same_bits(self.ctl.get()["U"], U, "set_nominal round trip")
        assert self.ctl.info()["tick"] == self.tick

    def step(self, pose=None, **kw):
        c = self.c
        pose = c["pose"] if pose is None else pose
        o = dict(c["opts"], **kw)
        plan = c["terminal"] == "plan"
        cost, goal = (self.cost, None) if plan else (None, self.sc["goal_point"])
        before = self.ctl.get()
        u0, info = self.df.control(self.ctl, pose, goal=goal, planner=self.pl if plan else None, stream=self.stream, **o)
        self.tick += 1
        g = self.ctl.get()
        what = "dim %d K %d T %d tick %d" % (self.dim, self.K, self.T, self.tick)
        args = (self.dist, self.sc["shape"], self.sc["origin"], self.sc["step"], pose, before["U"], self.seed, self.tick)
        r = mppi_ref.roll(*args, self.K, o, cost, goal)
        _same_bits(g["J"], r["J"], "J, " + what)
        assert np.array_equal(g["hits"], r["hits"]), what
        assert _b(info["Jmin"]) == _b(r["Jmin"]) and info["best"] == r["best"], (what, info, r["Jmin"], r["best"])
        # the weights: the one inexact step
        q = g["q"]
        dq = np.abs(q.astype(np.int64) - r["q"].astype(np.int64))
        self.q_off += int(np.count_nonzero(dq))
        assert dq.max() <= 1, "%s: q differs from the reference's at %d of %d rollouts, by up to %d" % (what, np.count_nonzero(dq), self.K, dq.max())
        assert q.max() == U64(1 << 32) and q[r["best"]] == U64(1 << 32)
        # everything after q: from the device's q, exactly
        f = mppi_ref.finish(r, q, *args, o, cost, goal)
        assert (info["T"], info["Th"], info["S2"], info["hits"]) == (f["T"], f["Th"], f["S2"], f["nhit"]), (what, info, f["T"], f["Th"], f["S2"])
        assert _b(info["neff"]) == _b(f["neff"]), (what, info["neff"], f["neff"])
        _same_bits(g["U"], f["U"], "the new sequence, " + what)
        _same_bits(u0, f["u0"], "u0, " + what)
        _same_bits(g["nominal_states"], f["nominal_states"], "nominal states, " + what)
        assert _b(info["nominal_cost"]) == _b(f["nominal_cost"]) and info["nominal_hits"] == f["nominal_hits"], (what, info, f["nominal_cost"])
        i = self.ctl.info()
        assert i["tick"] == self.tick and i["steps"] == self.tick and g["stats"] == info
        for k, v in r["branches"].items():
            self.branches[k] = self.branches.get(k, 0) + v
        return u0, info, r

    def shift(self):
        before = self.ctl.get()["U"]
        self.ctl.shift()
        _same_bits(self.ctl.get()["U"], mppi_ref.shift(before), "shift")
        assert self.ctl.info()["tick"] == self.tick


def _b(v):
    return int(np.float64(v).view(U64))


def _two_steps(c):
    ck = Checked(c)
    ck.set_nominal(mc.nominal_of(c))
    ck.step()
    ck.shift()
    ck.step()
    return ck


# ---- shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T", mc.SHAPES)
def test_stages_2d_every_shape(K, T):
    """Two steps with a shift between them, towards the first ball with the planner's cost-to-go at the end."""
    ck = _two_steps(mc.shape_case(K, T))
    if K >= 63 and T >= 33:
        assert ck.branches["col"] and ck.branches["band"] and ck.branches["free"]
    print("K %d T %d: q off by one at %d rollout-steps of %d" % (K, T, ck.q_off, 2 * K))


@pytest.mark.parametrize("K,T", mc.SHAPES3)
def test_stages_3d(K, T):
    _two_steps(mc.shape_case(K, T, 3))


def test_zero_nominal_from_init():
    """The first step after init: Ubar = 0, every rollout is pure noise."""
    for dim in (2, 3):
        ck = Checked(mc.shape_case(300, 12, dim))
        _, info, _ = ck.step()
        assert info["neff"] > 1.0
        ck.shift()
        ck.step()


# ---- branches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.branch_cases()))
def test_branch(name):
    c = mc.branch_cases()[name]
    ck = Checked(c)
    ck.set_nominal(mc.nominal_of(c))
    _, info, r = ck.step()
    for e in c["expect"]:
        assert r["branches"].get(e, 0) > 0, (name, e, r["branches"])      # asserted, not assumed
    if "col" in c["expect"]:
        assert info["hits"] > 0 and ck.ctl.get()["hits"].max() > 0
    if name == "sigma0":
        assert np.all(ck.ctl.get()["U"][:, 1] == mc.nominal_of(c)[:, 1])
    ck.shift()
    ck.step()


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
def _run(c, stream=None):
    import gpismap_amd
    sc, df, dist, pl, cost = env(c["dim"])
    ctl = gpismap_amd.Controller()
    ctl.init(c["dim"], c["K"], c["T"], seed=c["seed"])
    ctl.set_nominal(mc.nominal_of(c))
    out = []
    for _ in range(2):
        u0, info = df.control(ctl, c["pose"], planner=pl, stream=stream, **c["opts"])
        g = ctl.get()
        g.pop("stats")
        out.append(dict(g, u0=u0, cost=np.float64(info["nominal_cost"])))
        ctl.shift()
    return out


def test_same_bits_on_a_callers_stream_and_on_the_own_stream():
    import torch
    c = mc.shape_case(1000, 33)
    a = _run(c)
    eq = lambda x, y: all(np.array_equal(np.ascontiguousarray(p[k]).view(np.uint8), np.ascontiguousarray(q[k]).view(np.uint8)) for p, q in zip(x, y) for k in p)
    assert eq(a, _run(c))
    s = torch.cuda.Stream(device=0)
    assert eq(a, _run(c, stream=C.c_void_p(s.cuda_stream)))
    assert not eq(a, _run(dict(c, seed=6)))


def test_rollouts_depend_on_seed_tick_and_index_alone():
    a, b = Checked(mc.shape_case(257, 33)), Checked(mc.shape_case(1000, 33))
    for ck in (a, b):
        ck.set_nominal(mc.nominal_of(ck.c))
        ck.step()
    _same_bits(a.ctl.get()["J"], b.ctl.get()["J"][:257], "the first 257 of 1000")


def test_closed_loop_2d_on_the_device():
    """The CPU scenario of tests/test_mppi_ref.py through Controller, with its acceptance: behaviour, not bits (a q may differ
    by one from the reference's own run)."""
    import gpismap_amd
    sc, df, dist, pl, cost = env(2)
    ctl = gpismap_amd.Controller(**LOOP2["opts"])
    ctl.init(2, LOOP2["K"], LOOP2["T"], seed=LOOP2["seed"])

    def step_fn(pose):
        u0, _ = df.control(ctl, pose, planner=pl)
        ctl.shift()
        return u0

    steps, least, e = closed_loop(LOOP2, step_fn)
    print("%s steps, least distance %.3f, %.3f from the goal" % (steps, least, e))
    assert steps is not None and steps <= LOOP2["budget"] and least >= mc.opts(2)["clearance"] and e <= 2 * sc["step"]


def test_device_pointers():
    import gpismap_amd
    ctl = gpismap_amd.Controller()
    ctl.init(2, 300, 8)
    p = ctl.device_ptrs()
    assert all(p[k] for k in gpismap_amd.Controller.PTR_KEYS) and len(set(p.values())) == 5
    ctl.shift()
    q = ctl.device_ptrs()
    assert q["U"] != p["U"] and all(q[k] == p[k] for k in ("J", "q", "hits", "nominal_states"))
    ctl.shift()
    assert ctl.device_ptrs() == p


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_state():
    import gpismap_amd
    L = gpismap_amd.lib()
    sc, df, dist, pl, cost = env(2)
    sc3, df3, _, pl3, _ = env(3)
    nores, nopl = gpismap_amd.DistanceField(), gpismap_amd.Planner()
    dp = lambda a: None if a is None else np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))
    c = mc.shape_case(300, 12)
    ctl = gpismap_amd.Controller()
    goal = sc["goal_point"]

    def step(ctl_h=ctl, f=df, p=pl, pose=c["pose"], g=None, **kw):
        o = gpismap_amd.mppi_opts(2, sc["step"], **kw)
        return L.gpis_mppi_step(ctl_h.h if ctl_h is not None else None, f.h if f is not None else None, p.h if p is not None else None,
                                dp(pose), dp(g), C.byref(o), None, None)

    # before init
    assert step() == -3 and L.gpis_mppi_shift(ctl.h) == -3 and L.gpis_mppi_get(ctl.h, None, None, None, None, None, None) == -3
    assert L.gpis_mppi_set_nominal(ctl.h, dp(np.zeros(24))) == -3 and L.gpis_mppi_device(ctl.h, (C.c_void_p * 5)(), 5) == -3
    assert ctl.info()["inited"] == 0
    with pytest.raises(gpismap_amd.GpisError):
        ctl.get()
    with pytest.raises(gpismap_amd.GpisError):
        ctl.step(df, c["pose"], planner=pl)
    assert L.gpis_mppi_init(None, 2, 8, 8, 1) == -1 and L.gpis_mppi_init(ctl.h, 4, 8, 8, 1) == -1 and L.gpis_mppi_init(ctl.h, 2, 0, 8, 1) == -1
    assert L.gpis_mppi_init(ctl.h, 2, 8, 0, 1) == -1
    assert L.gpis_mppi_init(ctl.h, 2, 65537, 8, 1) == -4 and L.gpis_mppi_init(ctl.h, 2, 8, 257, 1) == -4 and ctl.info()["inited"] == 0
    ctl.init(2, c["K"], c["T"], seed=3)
    ctl.set_nominal(mc.nominal_of(c))
    df.control(ctl, c["pose"], planner=pl, **c["opts"])
    a, ia, pa = ctl.get(), ctl.info(), ctl.device_ptrs()

    def still_there(what):
        b = ctl.get()
        assert ctl.info() == ia and ctl.device_ptrs() == pa and b["stats"] == a["stats"], what
        for k in ("U", "J", "nominal_states"):
            _same_bits(b[k], a[k], what + ": " + k)
        assert np.array_equal(b["q"], a["q"]) and np.array_equal(b["hits"], a["hits"]), what

    bad_pose = c["pose"].copy(); bad_pose[1] = np.nan
    zero_heading = c["pose"].copy(); zero_heading[2:4] = 0.0
    arg = dict(no_field=dict(f=None), no_pose=dict(pose=None), nan_pose=dict(pose=bad_pose), zero_heading=dict(pose=zero_heading),
               both=dict(g=goal), neither=dict(p=None), nan_goal=dict(p=None, g=np.array([np.nan, 0.0])), dim_field=dict(f=df3),
               dim_plan=dict(p=pl3), dt0=dict(dt=0.0), dt_nan=dict(dt=np.nan), lam0=dict(lam=0.0), lam_neg=dict(lam=-1.0),
               sigma_neg=dict(sigma=(0.1, -0.1)), sigma_inf=dict(sigma=(np.inf, 0.1)), w_neg=dict(w_obs=-1.0), w_nan=dict(w_goal=np.nan),
               margin_neg=dict(margin=-0.1), limits=dict(umin=(0.5, 0.0), umax=(0.4, 1.0)), gamma_inf=dict(gamma=np.inf),
               clearance_nan=dict(clearance=np.nan))
    for name, kw in arg.items():
        assert step(**kw) == -1, name
        still_there(name)
    assert step(ctl_h=None) == -1
    assert step(f=nores) == -3 and step(p=nopl) == -3
    still_there("a field and a planner without a result")
    # a planner of another lattice
    other = gpismap_amd.DistanceField()
    other.from_grid(_dev(np.ones(20 * 20, F32)).data_ptr(), (20, 20), (0.0, 0.0), 0.1, 0.0)
    assert step(p=other.plan([(0.5, 0.5)], planner=gpismap_amd.Planner(), clearance=0.0)) == -1
    still_there("a planner of another lattice")
    bad_U = mc.nominal_of(c); bad_U[3, 1] = np.inf
    assert L.gpis_mppi_set_nominal(ctl.h, dp(bad_U)) == -1 and L.gpis_mppi_set_nominal(ctl.h, None) == -1
    assert L.gpis_mppi_init(ctl.h, 2, 65537, 8, 1) == -4 and L.gpis_mppi_init(ctl.h, 3, 8, 300, 1) == -4
    still_there("set_nominal and init")
    with pytest.raises(gpismap_amd.GpisError):
        ctl.step(df, c["pose"])
    with pytest.raises(gpismap_amd.GpisError):
        ctl.step(df, c["pose"][:5], planner=pl)
    with pytest.raises(gpismap_amd.GpisError):
        ctl.step(df, c["pose"], planner=pl, speed=1.0)
    with pytest.raises(gpismap_amd.GpisError):
        ctl.set_nominal(np.zeros(5))
    still_there("python checks")
    # after the errors the controller works again; init replaces it, also by one of the other dimension
    df.control(ctl, c["pose"], goal=goal)
    assert ctl.info()["tick"] == 2
    ctl.init(3, 64, 4, seed=2)
    u0, info = df3.control(ctl, mc.FREE3, planner=pl3)
    assert ctl.info()["dim"] == 3 and u0.shape == (4,) and ctl.info()["tick"] == 1
