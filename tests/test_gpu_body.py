"""The robot's footprint on the GPU (csrc/body.hip, the BODY kernels of csrc/mppi.hip, traj_body_check_kernel of csrc/traj.hip,
gpis_body_*) against the numpy reference (tests/body_ref.py), stage by stage as tests/test_gpu_obst.py does: after every call the
reference is fed the device's state from before that call.  J, hits, dyn_hits, min_sep and the nominal states are compared as
bits; the weights q may differ by 1 (the one exp); everything after q is computed from the device's q and compared exactly.
The batch query and the trajectory check are compared as bits (a NaN equals a NaN) and as integers."""
import ctypes as C

import numpy as np
import pytest

import body_cases as bc
import body_ref
import mppi_cases as mc
import mppi_ref
import obst_cases as oc
import traj_cases
from test_gpu_mppi import _b, _dev, _same_bits, env
from test_gpu_obst import device_set

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U64 = np.uint64


def device_body(B):
    """A Footprint holding the reference's footprint B, read back and compared."""
    import gpismap_amd
    fp = gpismap_amd.Footprint(B["dim"]).set(B["b"], B["rho"])
    g, i = fp.get(), fp.info()
    _same_bits(g["offset"], B["b"], "offsets")
    _same_bits(g["radius"], B["rho"], "radii")
    assert (i["inited"], i["dim"], i["m"]) == (1, B["dim"], B["m"])
    return fp


def _nan_same(u, v, what):
    u, v = np.ascontiguousarray(u, F64), np.ascontiguousarray(v, F64)
    assert u.shape == v.shape, (what, u.shape, v.shape)
    ok = (u.view(U64) == v.view(U64)) | (np.isnan(u) & np.isnan(v))
    assert ok.all(), (what, np.argwhere(~ok)[:6].tolist(), u[~ok][:4], v[~ok][:4])


class Checked:
    """A Controller whose every step with a footprint (and a set of balls, if the case has one) is checked against body_ref fed
    with the device's state from before the call."""

    def __init__(self, c, stream=None, ctl=None, env_=None):
        import gpismap_amd
        self.c, self.dim, self.K, self.T, self.seed, self.tick = c, c["dim"], c["K"], c["T"], c["seed"], 0
        # env_: (lattice dict, field, its dist flat, planner, its cost flat) of another scene in env(dim)'s place
        self.sc, self.df, self.dist, self.pl, self.cost = env(self.dim) if env_ is None else env_
        self.stream = stream
        self.ctl = ctl if ctl is not None else gpismap_amd.Controller()
        self.ctl.init(self.dim, self.K, self.T, seed=self.seed)
        self.ob = device_set(c["obst"], self.sc["step"]) if c["obst"] is not None else None
        self.fp = device_body(c["body"])
        self.q_off = 0

    def step(self, t_now=None):
        c = self.c
        S, B = c["obst"], c["body"]
        t_now = c["t_now"] if t_now is None else t_now
        o = c["opts"]
        plan = c["terminal"] == "plan"
        cost, goal = (self.cost, None) if plan else (None, self.sc["goal_point"])
        before = self.ctl.get()
        u0, info = self.df.control(self.ctl, c["pose"], goal=goal, planner=self.pl if plan else None, stream=self.stream, obstacles=self.ob,
                                   t=t_now, footprint=self.fp, **o)
        self.tick += 1
        g, go, so = self.ctl.get(), self.ctl.get_obstacle(), self.ctl.obstacle_stats()
        what = "dim %d K %d T %d m %d n %d tick %d" % (self.dim, self.K, self.T, B["m"], S["n"] if S else 0, self.tick)
        args = (self.dist, self.sc["shape"], self.sc["origin"], self.sc["step"], c["pose"], before["U"], self.seed, self.tick)
        r = body_ref.roll(*args, self.K, o, cost, goal, obst=S, t_now=t_now, body=B)
        _same_bits(g["J"], r["J"], "J, " + what)
        assert np.array_equal(g["hits"], r["hits"]), what
        assert np.array_equal(go["dyn_hits"], r["dyn_hits"]), what
        _same_bits(go["min_sep"], r["min_sep"], "min_sep, " + what)
        assert _b(info["Jmin"]) == _b(r["Jmin"]) and info["best"] == r["best"], (what, info, r["Jmin"], r["best"])
        q = g["q"]
        dq = np.abs(q.astype(np.int64) - r["q"].astype(np.int64))
        self.q_off += int(np.count_nonzero(dq))
        assert dq.max() <= 1, "%s: q differs from the reference's at %d of %d rollouts, by up to %d" % (what, np.count_nonzero(dq), self.K, dq.max())
        f = body_ref.finish(r, q, *args, o, cost, goal, obst=S, t_now=t_now, body=B)
        assert (info["T"], info["Th"], info["S2"], info["hits"]) == (f["T"], f["Th"], f["S2"], f["nhit"]), (what, info)
        assert _b(info["neff"]) == _b(f["neff"]), (what, info["neff"], f["neff"])
        _same_bits(g["U"], f["U"], "the new sequence, " + what)
        _same_bits(u0, f["u0"], "u0, " + what)
        _same_bits(g["nominal_states"], f["nominal_states"], "nominal states, " + what)
        assert _b(info["nominal_cost"]) == _b(f["nominal_cost"]) and info["nominal_hits"] == f["nominal_hits"], (what, info, f["nominal_cost"])
        assert (so["dyn_hit_rollouts"], so["nominal_dyn_hits"], so["n"]) == (f["ndyn"], f["nominal_dyn_hits"], S["n"] if S else 0), (what, so, f["ndyn"])
        assert _b(so["nominal_min_sep"]) == _b(f["nominal_min_sep"]), (what, so, f["nominal_min_sep"])
        # the nominal rollout's hits are the batch query's count over its states
        chk = self.fp.clearance(self.df, g["nominal_states"][1:], clearance=o["clearance"])
        assert chk["below"] == info["nominal_hits"], (what, chk["below"], info["nominal_hits"])
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


# ---- the footprint itself -------------------------------------------------------------------------------------------------------
def test_set_get_and_its_errors():
    import gpismap_amd
    L = gpismap_amd.lib()
    B = bc.footprint(3, 16)
    fp = device_body(B)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))

    def still_there(what):
        g = fp.get()
        _same_bits(g["offset"], B["b"], what)
        _same_bits(g["radius"], B["rho"], what)
        assert fp.info()["m"] == 16, what

    b, r = B["b"][:4].copy(), B["rho"][:4].copy()
    bad = lambda a, idx, val: (lambda x: (x.__setitem__(idx, val), x)[1])(a.copy())
    calls = dict(null=(None, 3, 4, b, r), dim=(fp.h, 4, 4, b, r), neg_m=(fp.h, 3, -1, b, r), nan_b=(fp.h, 3, 4, bad(b, (2, 1), np.nan), r),
                 inf_b=(fp.h, 3, 4, bad(b, (0, 2), np.inf), r), neg_r=(fp.h, 3, 4, b, bad(r, 3, -1e-9)), nan_r=(fp.h, 3, 4, b, bad(r, 0, np.nan)),
                 no_b=(fp.h, 3, 4, None, r))
    for name, (h, dim, m, bb, rr) in calls.items():
        assert L.gpis_body_set(h, dim, m, dp(bb), dp(rr)) == -1, name
        still_there(name)
    z = np.zeros((17, 3))
    assert L.gpis_body_set(fp.h, 3, 17, dp(z), dp(z[:, 0])) == -4
    still_there("m = 17")
    assert L.gpis_body_info(None, dp(np.zeros(4)), 4) == -1 and L.gpis_body_get(None, None, None) == -1
    fp.set(np.zeros((0, 3)), np.zeros(0))
    assert fp.info()["m"] == 0 and fp.get()["offset"].shape == (0, 3)
    box = gpismap_amd.Footprint.box(1.0, 0.4, 4)
    _same_bits(box.get()["offset"], body_ref.box(1.0, 0.4, 4)["b"], "box")
    _same_bits(box.get()["radius"], body_ref.box(1.0, 0.4, 4)["rho"], "box radii")


# ---- rollout stages -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,m,n", bc.SHAPES)
def test_stages_2d_every_shape(K, T, m, n):
    """Two steps with a shift between them, the clock moved on by dt."""
    ck, r = _two_steps(bc.shape_case(K, T, m, n))
    if K >= 63 and T >= 33:
        br = r["branches"]
        assert br["col"] and br["band"] and (m < 2 or br["second_ball_nearer"]), br
    print("K %d T %d m %d n %d: q off by one at %d rollout-steps of %d" % (K, T, m, n, ck.q_off, 2 * K))


@pytest.mark.parametrize("K,T,m,n", bc.SHAPES3)
def test_stages_3d(K, T, m, n):
    c = bc.shape_case(K, T, m, n, 3)
    assert c["body"]["b"][:, 2].all()
    _two_steps(c)


# ---- identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("balls", (False, True), ids=("no_balls", "balls"))
def test_no_footprint_an_empty_one_and_the_point_are_the_plain_step(balls):
    """footprint=None, m = 0 and the one-ball zero footprint: every output has the bits of a second controller of the same seed
    stepped without a footprint, over two steps, with and without a set of balls; then a plain step after a footprint step is the
    plain step."""
    import gpismap_amd
    c = oc.shape_case(1000, 33, 2)
    sc, df, dist, pl, cost = env(2)
    ob = device_set(c["obst"]) if balls else None
    empty = gpismap_amd.Footprint(2).set(np.zeros((0, 2)), np.zeros(0))
    never = gpismap_amd.Footprint(2)
    point = device_body(body_ref.point(2))
    wide = device_body(bc.footprint(2, 3))

    def run(fps):
        ctl = gpismap_amd.Controller()
        ctl.init(2, c["K"], c["T"], seed=c["seed"])
        ctl.set_nominal(mc.nominal_of(c))
        out = []
        for n, fp in enumerate(fps):
            u0, info = df.control(ctl, c["pose"], planner=pl, obstacles=ob, t=c["t_now"] + n * 0.1, footprint=fp, **c["opts"])
            g = ctl.get()
            g.update(ctl.get_obstacle())
            out.append(dict(g, u0=u0, tick=ctl.info()["tick"], ostats=ctl.obstacle_stats()))
            ctl.shift()
        return out

    base = run([None, None])
    for fp in (empty, never, point):
        for a, b in zip(base, run([fp, fp])):
            assert a["stats"] == b["stats"] and a["tick"] == b["tick"] and a["ostats"] == b["ostats"]
            for k in ("U", "J", "nominal_states", "u0", "min_sep"):
                _same_bits(a[k], b[k], k)
            assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["hits"], b["hits"]) and np.array_equal(a["dyn_hits"], b["dyn_hits"])
    # a plain step after a footprint step: what the plain step gives from the same sequence
    import gpismap_amd as G
    a, b = G.Controller(), G.Controller()
    for ctl in (a, b):
        ctl.init(2, c["K"], c["T"], seed=c["seed"])
        ctl.set_nominal(mc.nominal_of(c))
    df.control(a, c["pose"], planner=pl, obstacles=ob, t=c["t_now"], footprint=wide, **c["opts"])
    df.control(b, c["pose"], planner=pl, obstacles=ob, t=c["t_now"], **c["opts"])
    assert not np.array_equal(a.get()["J"], b.get()["J"])
    b.set_nominal(a.get()["U"])
    ua, _ = df.control(a, c["pose"], planner=pl, obstacles=ob, t=c["t_now"], **c["opts"])
    ub, _ = df.control(b, c["pose"], planner=pl, obstacles=ob, t=c["t_now"], **c["opts"])
    ga, gb = a.get(), b.get()
    for k in ("U", "J", "nominal_states"):
        _same_bits(ga[k], gb[k], "plain after footprint: " + k)
    assert np.array_equal(ga["q"], gb["q"]) and np.array_equal(ga["hits"], gb["hits"]) and ga["stats"] == gb["stats"]
    _same_bits(ua, ub, "u0")


# ---- branches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.branch_cases()))
def test_branch(name):
    c = bc.branch_cases()[name]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    _, info, r = ck.step()
    for e in c["expect"]:
        assert r["branches"].get(e, 0) > 0, (name, e, r["branches"])      # asserted, not assumed
    ck.shift()
    ck.step(c["t_now"] + c["opts"]["dt"])


# ---- the batch query --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (2, 3))
def test_clearance_every_size(dim):
    sc, df, dist, pl, cost = env(dim)
    Sall = bc.states(dim, 1000)
    for m in bc.CLEAR_MS:
        B = bc.footprint(dim, m)
        fp = device_body(B)
        one = fp.clearance(df, Sall[:1], clearance=0.1)
        for n in bc.CLEAR_NS:
            S = Sall[:n]
            got = df.body_clearance(fp, S, clearance=0.1)
            ref = bc.ref_clearance(dim, B, S, 0.1)
            _nan_same(got["D"], ref["D"], (dim, m, n))
            assert np.array_equal(got["ball"], ref["ball"]) and got["ball"].dtype == np.int32, (dim, m, n)
            assert (got["below"], got["off"], got["least"]) == (ref["below"], ref["off"], ref["least"]), (dim, m, n, got, ref)
            for at in (0, 63, 64, n - 1):
                if at < n:
                    T = S.copy()
                    T[[0, at]] = T[[at, 0]]
                    moved = fp.clearance(df, T, clearance=0.1)
                    _nan_same(moved["D"][at], one["D"][0], (dim, m, n, at))
                    assert moved["ball"][at] == one["ball"][0]
    # ties go to the lowest index; every state off
    r = bc.ref_clearance(dim, B, Sall)
    T = np.concatenate([Sall[r["least"]][None], Sall, Sall[r["least"]][None]])
    assert fp.clearance(df, T)["least"] == 0
    far = Sall[np.isnan(r["D"])]
    e = fp.clearance(df, far)
    assert (e["below"], e["off"], e["least"]) == (0, far.shape[0], -1) and np.isnan(e["D"]).all() and np.all(e["ball"] == -1)


# ---- trajectories ---------------------------------------------------------------------------------------------------------------
TRAJ_KEYS = ("D_min", "waypoint", "ball", "collides")


def _traj_equal(got, ref, what):
    _nan_same(got["D_min"], ref["D_min"], what)
    for k in TRAJ_KEYS[1:]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


@pytest.mark.parametrize("dim", (2, 3))
def test_trajectories_after_optimize(dim):
    """The planner's paths to traj_cases' starts, resampled and smoothed on the device; the reference takes the device's
    waypoints and statuses."""
    import gpismap_amd
    sc, df, dist, pl, cost = env(dim)
    B = bc.traj_body(dim)
    fp = device_body(B)
    tj = gpismap_amd.Trajectories()
    shapes = bc.TRAJ_SHAPES if dim == 2 else ((3, 4), (40, 64))
    saw = set()
    for m, N in shapes + ((44, 16),):
        st = traj_cases.starts(sc)[:m] if m <= 40 else traj_cases.starts(sc)            # (44: with the four that have no path)
        pl.paths(st)
        g = df.smooth(pl, N=N, trajectories=tj, iters=8).get()
        got = tj.body_clearance(fp, df, clearance=0.05)
        _traj_equal(got, bc.ref_traj(dim, B, g["x"], g["status"], 0.05), (dim, m, N))
        after = tj.get()
        assert all(np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(after[k]).view(np.uint8)) for k in g)
        saw |= set(g["status"].tolist())
        assert np.all(got["collides"][g["status"] == 2] == 0) and np.isnan(got["D_min"][g["status"] == 2]).all()
    assert 2 in saw and (0 in saw or 1 in saw)


def test_trajectories_hand_made():
    import gpismap_amd
    sc, df, dist, pl, cost = env(2)
    B = bc.traj_body(2)
    fp = device_body(B)
    tj = gpismap_amd.Trajectories()
    x, names = bc.repeated_waypoints()
    g = df.smooth(x, trajectories=tj, iters=0).get()
    assert np.array_equal(g["x"].view(np.uint32), x.view(np.uint32))
    ref = bc.ref_traj(2, B, g["x"], g["status"], 0.0)
    _traj_equal(tj.body_clearance(fp, df), ref, "repeated waypoints")
    assert not np.array_equal(ref["D_min"], bc.ref_traj(2, B, g["x"], g["status"], 0.0, variant="last_x")["D_min"])
    y = bc.leaving_waypoints()
    g = df.smooth(y, trajectories=tj, iters=0).get()
    got = tj.body_clearance(fp, df)
    _traj_equal(got, bc.ref_traj(2, B, g["x"], g["status"], 0.0), "leaving the lattice")
    assert got["collides"].tolist() == [1, 1] and np.isnan(got["D_min"][1]) and got["waypoint"][1] == -1
    # the hand-made batch of the smoother's own tests, with its NaN trajectory (status 2)
    hx, hopts, hnames = traj_cases.hand_made(sc, dist, 65)
    g = df.smooth(hx, trajectories=tj, iters=4).get()
    got = tj.body_clearance(fp, df, clearance=0.1)
    _traj_equal(got, bc.ref_traj(2, B, g["x"], g["status"], 0.1), "hand made")
    assert g["status"][hnames.index("nan")] == 2 and got["collides"][hnames.index("through")] == 1


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
def test_same_bits_on_a_callers_stream_and_on_the_own_stream():
    import gpismap_amd
    import torch
    c = bc.shape_case(1000, 33, 3, 2)
    sc, df, dist, pl, cost = env(2)
    S = bc.states(2, 1000)

    def run(stream=None):
        ob, fp = device_set(c["obst"]), device_body(c["body"])
        ctl = gpismap_amd.Controller()
        ctl.init(2, c["K"], c["T"], seed=c["seed"])
        ctl.set_nominal(mc.nominal_of(c))
        out = []
        for n in range(2):
            u0, info = df.control(ctl, c["pose"], planner=pl, stream=stream, obstacles=ob, t=c["t_now"] + n * 0.1, footprint=fp, **c["opts"])
            g = ctl.get()
            g.pop("stats")
            g.update(ctl.get_obstacle())
            out.append(dict(g, u0=u0, cost=np.float64(info["nominal_cost"])))
            ctl.shift()
        q = fp.clearance(df, S, clearance=0.1, stream=stream)
        out.append(dict(D=q["D"], ball=q["ball"], counts=np.array([q["below"], q["off"], q["least"]])))
        return out

    eq = lambda x, y: all(np.array_equal(np.ascontiguousarray(p[k]).view(np.uint8), np.ascontiguousarray(q[k]).view(np.uint8)) for p, q in zip(x, y) for k in p)
    a = run()
    assert eq(a, run())
    s = torch.cuda.Stream(device=0)
    assert eq(a, run(C.c_void_p(s.cuda_stream)))


# ---- lifetime and errors ----------------------------------------------------------------------------------------------------------
def test_a_footprint_changed_and_destroyed_between_steps():
    c = bc.branch_cases()["crossing"]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    ck.step()
    ck.shift()
    B2 = bc.footprint(2, 16)
    ck.fp.set(B2["b"], B2["rho"])
    ck.c = dict(c, body=B2)
    ck.step()
    ck.shift()
    ck.fp.close()
    B3 = bc.footprint(2, 2)
    ck.fp = device_body(B3)
    ck.c = dict(c, body=B3)
    ck.step()
    ck.fp.close()
    ck.df.control(ck.ctl, c["pose"], planner=ck.pl, **c["opts"])      # and on without one
    assert ck.ctl.info()["tick"] == 4


def test_errors_leave_the_state():
    import gpismap_amd
    L = gpismap_amd.lib()
    sc, df, dist, pl, cost = env(2)
    sc3, df3, _, pl3, _ = env(3)
    c = bc.branch_cases()["crossing"]
    ck = Checked(c)
    ck.ctl.set_nominal(mc.nominal_of(c))
    ck.step()
    ctl, ob, fp = ck.ctl, ck.ob, ck.fp
    fp3 = device_body(bc.footprint(3, 2))
    a, ia, ga, sa = ctl.get(), ctl.info(), ctl.get_obstacle(), ctl.obstacle_stats()
    dp = lambda a: None if a is None else np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def step(ctl_h=ctl, f=df, p=pl, b=fp, o=ob, t=3.5, pose=c["pose"], g=None, **kw):
        mo = gpismap_amd.mppi_opts(2, sc["step"], **kw)
        h = lambda x: x.h if x is not None else None
        return L.gpis_body_mppi_step(h(ctl_h), h(f), h(p), h(b), h(o), t, dp(pose), dp(g), C.byref(mo), None, None)

    def still_there(what):
        b = ctl.get()
        assert ctl.info() == ia and b["stats"] == a["stats"] and ctl.obstacle_stats() == sa, what
        for k in ("U", "J", "nominal_states"):
            _same_bits(b[k], a[k], what + ": " + k)
        assert np.array_equal(b["q"], a["q"]) and np.array_equal(b["hits"], a["hits"]), what
        go = ctl.get_obstacle()
        assert np.array_equal(go["dyn_hits"], ga["dyn_hits"]), what
        _same_bits(go["min_sep"], ga["min_sep"], what + ": min_sep")
        _same_bits(fp.get()["offset"], c["body"]["b"], what + ": the footprint")

    bad_pose = c["pose"].copy(); bad_pose[1] = np.nan
    arg = dict(other_dim=dict(b=fp3), t_nan=dict(t=np.nan), no_field=dict(f=None), nan_pose=dict(pose=bad_pose), both=dict(g=sc["goal_point"]),
               neither=dict(p=None), dim_field=dict(f=df3), dt0=dict(dt=0.0), w_neg=dict(w_obs=-1.0))
    for name, kw in arg.items():
        assert step(**kw) == -1, name
        still_there(name)
    assert step(ctl_h=None) == -1 and step(f=gpismap_amd.DistanceField()) == -3 and step(ctl_h=gpismap_amd.Controller()) == -3
    still_there("handles without a result")
    # the batch query's errors write nothing
    S = bc.states(2, 8)
    out = dict(D=np.full(8, 7.0), ball=np.full(8, 7, np.int32), counts=np.full(3, 7, np.int32))

    def query(f=df, b=fp, S=S, n=8, clr=0.0):
        h = lambda x: x.h if x is not None else None
        return L.gpis_body_clearance(h(f), h(b), dp(S), n, clr, dp(out["D"]), ip(out["ball"]), ip(out["counts"]), None)

    nan_s, zero_h = S.copy(), S.copy()
    nan_s[3, 0] = np.nan
    zero_h[5, 2:] = 0.0
    empty = gpismap_amd.Footprint(2).set(np.zeros((0, 2)), np.zeros(0))
    for name, kw, rc in (("no_field", dict(f=None), -1), ("no_body", dict(b=None), -1), ("n0", dict(n=0), -1), ("nan_state", dict(S=nan_s), -1),
                         ("zero_heading", dict(S=zero_h), -1), ("nan_clr", dict(clr=np.nan), -1), ("other_dim", dict(b=fp3), -1),
                         ("dim_field", dict(f=df3), -1), ("too_many", dict(n=(1 << 24) + 1), -4), ("empty", dict(b=empty), -3),
                         ("no_result", dict(f=gpismap_amd.DistanceField()), -3)):
        assert query(**kw) == rc, name
        assert all(np.all(v == 7) for v in out.values()), name
    assert query() == 0 and not np.all(out["D"] == 7)
    # the trajectory check's errors leave the result
    tj = gpismap_amd.Trajectories()
    x, _ = bc.repeated_waypoints()
    g = df.smooth(x, trajectories=tj, iters=0).get()
    o4 = dict(D=np.full(5, 7.0), w=np.full(5, 7, np.int32), b=np.full(5, 7, np.int32), c=np.full(5, 7, np.int32))

    def check(t=tj, f=df, b=fp, clr=0.0):
        h = lambda x: x.h if x is not None else None
        return L.gpis_body_traj_clearance(h(t), h(f), h(b), clr, dp(o4["D"]), ip(o4["w"]), ip(o4["b"]), ip(o4["c"]))

    for name, kw, rc in (("no_traj", dict(t=None), -1), ("no_field", dict(f=None), -1), ("no_body", dict(b=None), -1), ("inf_clr", dict(clr=np.inf), -1),
                         ("other_dim", dict(b=fp3), -1), ("dim_field", dict(f=df3), -1), ("empty", dict(b=empty), -3),
                         ("no_result", dict(t=gpismap_amd.Trajectories()), -3)):
        assert check(**kw) == rc, name
        assert all(np.all(v == 7) for v in o4.values()), name
    after = tj.get()
    assert all(np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(after[k]).view(np.uint8)) for k in g)
    assert check() == 0
    # after the errors everything works
    ck.shift()
    ck.step(4.0)


# ---- closed loop ----------------------------------------------------------------------------------------------------------------
def test_closed_loop_through_a_door_on_the_device():
    """The CPU scenario of tests/test_body_ref.py through Controller, with its acceptance: behaviour, not bits (a q may differ by
    one from the reference's own run)."""
    import gpismap_amd
    sc = bc.door_scene()
    df = gpismap_amd.DistanceField()
    df.from_grid(_dev(np.ascontiguousarray(sc["f"], F32)).data_ptr(), sc["shape"], sc["origin"], sc["step"], 0.0)
    assert np.array_equal(df.get()[0].ravel().view(np.uint32), sc["dist"].view(np.uint32))
    pl = df.plan([sc["goal_point"].astype(F32)], planner=gpismap_amd.Planner(), **bc.PLAN)
    robot = gpismap_amd.Footprint.box(bc.ROBOT["length"], bc.ROBOT["width"], bc.ROBOT["discs"])

    def loop(footprint, clearance):
        ctl = gpismap_amd.Controller()
        ctl.init(2, bc.LOOP["K"], bc.LOOP["T"], seed=bc.LOOP["seed"])

        def step_fn(pose, o):
            u0, _ = df.control(ctl, pose, planner=pl, footprint=footprint, **o)
            ctl.shift()
            return u0

        return bc.closed_loop(clearance=clearance, step_fn=step_fn)

    body, outer, inner = loop(robot, 0.0), loop(None, bc.R_OUT), loop(None, bc.R_IN)
    for name, r in (("footprint", body), ("point, circumscribed", outer), ("point, inscribed", inner)):
        print("%s: %s steps, %.3f from the goal, least body clearance %.3f, %d driven states with the body in the wall"
              % (name, r["steps"], r["e"], np.nanmin(r["D"]), r["hits"]))
    assert body["steps"] is not None and body["hits"] == 0 and np.nanmin(body["D"]) >= 0.0
    assert outer["steps"] is None and outer["states"][-1, 0] < 3.8
    assert inner["hits"] > 0 and np.nanmin(inner["D"]) < 0.0
