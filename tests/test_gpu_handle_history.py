"""What a call leaves behind for the next one: every object that consumes a distance field keeps grow-only device buffers whose
layout is recomputed from the sizes of the current call, and a robot loop keeps these handles for its lifetime.  One handle per
object goes through its sequence of tests/history_cases.py (larger, smaller across the degenerate branch, the other dimension,
the first call again; tests/test_history_cases.py asserts on the CPU that each sequence reaches those branches).  After every
call: a. the result equals the numpy reference through the object's existing checker, tolerances unchanged (bits everywhere
except the weights of the filter and the controller, within 1 in 2^32); b. every output and every counter equals bit for bit that
of a fresh handle given only this call, the fields of info() no reference states included; c. the last call equals the first bit
for bit.  Times and the round counts of the two iterative solvers (the coverage's labelling, the planner) are not compared: they
depend on the schedule, not on the state.  Then one session: a single set of handles through rounds on different lattices, on a
caller's stream, against a set made anew each round on the default stream (handles against handles; the chain is tied to the
references in tests/test_gpu_nav_chain.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import dfield_ref
import history_cases as hc
import mppi_cases as mc
import test_gpu_body as tbd
import test_gpu_cover as tcv
import test_gpu_locate as tlo
import test_gpu_mppi as tmp
import test_gpu_obst as tob
import test_gpu_pf as tpf
import test_gpu_plan as tpl
import test_gpu_render_field as trf
import test_gpu_track_field as ttf
import test_gpu_view as tvw
from test_gpu_track import _check_bits as _check_track
from test_locate_ref import TH2, depth3
from test_track_ref import CAM, OFF2

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
NOT_STATE = ("rounds", "tile_launches")                   # counters of a schedule, not of the buffers
_FIELDS = {}


# ---- comparing ----------------------------------------------------------------------------------------------------------------
def _strip(info):
    return {k: v for k, v in info.items() if not k.endswith("ms") and k not in NOT_STATE}


def _same(a, b, what):
    """Two results of any nesting (dicts, sequences, arrays, numbers, None) with the same types, shapes and bits."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), (what, sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), (what, len(a), len(b))
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, k))
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
        bad = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)) // max(1, x.dtype.itemsize)
        assert bad.size == 0, (what, "%d bytes differ, first elements %s: %r against %r"
                               % (bad.size, np.unique(bad)[:6], x.reshape(-1)[np.unique(bad)[:3]], y.reshape(-1)[np.unique(bad)[:3]]))


def _run(n, entry, fresh):
    """Entries 0 .. n - 1: `entry(i)` on the long-lived handle (checked against the reference inside), `fresh(i)` on a new one;
    comparison b after every call, c at the end."""
    first = None
    for i in range(n):
        got = entry(i)
        _same(got, fresh(i), "entry %d against a fresh handle" % i)
        if i == 0:
            first = got
    _same(got, first, "the last entry against the first")


def _field(name):
    """(DistanceField, its dist flat) of a named analytic field of history_cases, built once."""
    if name not in _FIELDS:
        fd = hc.field(name)
        _FIELDS[name] = tpl._field(fd["f"].copy(), fd["shape"], fd["origin"], fd["step"])
    return _FIELDS[name]


def _void(stream):
    return C.c_void_p(stream) if stream else None


# ---- Controller ---------------------------------------------------------------------------------------------------------------
def _ctl_snap(ctl, **more):
    return dict(more, get=ctl.get(), info=_strip(ctl.info()))


def _controller_calls(c, init, set_nominal, step, shift, ctl_of):
    tr = []
    init()
    ctl = ctl_of()
    ptr = ctl.device_ptrs()["U"]
    tr.append(_ctl_snap(ctl))
    set_nominal(mc.nominal_of(c))
    tr.append(_ctl_snap(ctl))
    for k in range(2):
        if k:
            shift()
            tr.append(_ctl_snap(ctl))
        u0, info = step()
        tr.append(_ctl_snap(ctl, u0=u0, returned=_strip(info)))
    return tr, ptr


def _controller_checked(c, ctl):
    box = {}

    def init():
        box["ck"] = tmp.Checked(c, ctl=ctl)
    return _controller_calls(c, init, lambda U: box["ck"].set_nominal(U), lambda: box["ck"].step()[:2], lambda: box["ck"].shift(),
                             lambda: box["ck"].ctl)


def _controller_fresh(c):
    import gpismap_amd
    sc, df, dist, pl, cost = tmp.env(c["dim"])
    ctl = gpismap_amd.Controller()
    plan = c["terminal"] == "plan"
    step = lambda: df.control(ctl, c["pose"], goal=None if plan else sc["goal_point"], planner=pl if plan else None, **c["opts"])
    return _controller_calls(c, lambda: ctl.init(c["dim"], c["K"], c["T"], seed=c["seed"]), ctl.set_nominal, step, ctl.shift, lambda: ctl)


def test_controller_one_handle_through_changing_shapes():
    """(dim, K, T) of history_cases.CONTROLLER: the tree of the update 2, 4, 1 (no level, no barrier), 32, 2 segments wide, the
    columns 66, 132, 2, 4, 66; per entry init with a new seed, set_nominal, step, shift, step.  Where no buffer grew, the nominal
    sequence stands after init in the half it stood in after the init before: init returns to the first half."""
    import gpismap_amd
    ctl = gpismap_amd.Controller()
    state = dict(cap=0, ptr=None)

    def entry(i):
        tr, ptr = _controller_checked(hc.controller_case(i), ctl)
        if hc.CONTROLLER_COLUMNS[i] <= state["cap"]:
            assert ptr == state["ptr"], "entry %d: init left the nominal sequence in the other half" % i
        state.update(cap=max(state["cap"], hc.CONTROLLER_COLUMNS[i]), ptr=ptr)
        return tr

    _run(len(hc.CONTROLLER), entry, lambda i: _controller_fresh(hc.controller_case(i))[0])


# ---- Controller with balls and a footprint --------------------------------------------------------------------------------------
def _ctl_body_snap(ctl, **more):
    return dict(more, get=ctl.get(), info=_strip(ctl.info()), obstacle=ctl.get_obstacle(), obstacle_stats=ctl.obstacle_stats())


def _set_handles(c, ob, fp):
    """The case's set and footprint in the long-lived handles (None where the case has none): their own history."""
    S, B = c["obst"], c["body"]
    if S is not None:
        ob[c["dim"]].set(S["c"], S["v"], S["r"], epoch=S["epoch"])
        ob[c["dim"]].set_opts(**S["opts"])
        g = ob[c["dim"]].get()
        tmp._same_bits(g["centre"], S["c"], "centres")
        tmp._same_bits(g["radius"], S["r"], "radii")
    if B is not None:
        fp[c["dim"]].set(B["b"], B["rho"])
        tmp._same_bits(fp[c["dim"]].get()["offset"], B["b"], "offsets")
    return (ob[c["dim"]] if S is not None else None), (fp[c["dim"]] if B is not None else None)


def _controller_body_calls(c, init, step, shift, ctl_of):
    tr = []
    init()
    ctl = ctl_of()
    tr.append(_ctl_body_snap(ctl))
    ctl.set_nominal(mc.nominal_of(c))
    tr.append(_ctl_body_snap(ctl))
    for k in range(2):
        if k:
            shift()
            tr.append(_ctl_body_snap(ctl))
        u0, info = step(c["t_now"] + k * c["opts"]["dt"])
        tr.append(_ctl_body_snap(ctl, u0=u0, returned=_strip(info)))
    return tr


def _controller_body_checked(c, ctl, ob, fp):
    box = {}

    def init():
        if c["body"] is None:                                        # the plain step, by the plain controller's checker
            assert c["obst"] is None
            box["ck"] = tmp.Checked(c, ctl=ctl)
            box["step"] = lambda t: box["ck"].step()[:2]
        else:
            ck = box["ck"] = tbd.Checked(c, ctl=ctl)
            if ck.ob is not None:
                ck.ob.close()
            ck.fp.close()
            ck.ob, ck.fp = _set_handles(c, ob, fp)
            box["step"] = lambda t: ck.step(t)[:2]
    return _controller_body_calls(c, init, lambda t: box["step"](t), lambda: box["ck"].shift(), lambda: box["ck"].ctl)


def _controller_body_fresh(c):
    import gpismap_amd
    sc, df, dist, pl, cost = tmp.env(c["dim"])
    ctl = gpismap_amd.Controller()
    ob = tob.device_set(c["obst"]) if c["obst"] is not None else None
    fp = tbd.device_body(c["body"]) if c["body"] is not None else None
    plan = c["terminal"] == "plan"
    step = lambda t: df.control(ctl, c["pose"], goal=None if plan else sc["goal_point"], planner=pl if plan else None, obstacles=ob, t=t,
                                footprint=fp, **c["opts"])
    return _controller_body_calls(c, lambda: ctl.init(c["dim"], c["K"], c["T"], seed=c["seed"]), step, ctl.shift, lambda: ctl)


def test_controller_with_balls_and_a_footprint_one_handle_through_changing_shapes():
    """(dim, K, T, balls, body balls) of history_cases.CONTROLLER_BODY on one Controller, one Obstacles and one Footprint per
    dimension, set again per entry: init, set_nominal, step, shift, step with the clock moved on.  The per-rollout buffers of the
    balls grow inside step() under their own capacity: entry 3 steps without balls at the largest K, entry 4 with balls at that K.
    get_obstacle() and obstacle_stats() are part of every comparison with the fresh controller."""
    import gpismap_amd
    ctl = gpismap_amd.Controller()
    ob = {d: gpismap_amd.Obstacles(d, mc.scene(d)["step"]) for d in (2, 3)}
    fp = {d: gpismap_amd.Footprint(d) for d in (2, 3)}
    snaps = []

    def entry(i):
        snaps.append(_controller_body_checked(hc.controller_body_case(i), ctl, ob, fp))
        return snaps[-1]

    _run(len(hc.CONTROLLER_BODY), entry, lambda i: _controller_body_fresh(hc.controller_body_case(i)))
    hit = [[t["obstacle_stats"]["dyn_hit_rollouts"] for t in tr if "u0" in t] for tr in snaps]
    assert all(min(h) > 0 for h, e in zip(hit, hc.CONTROLLER_BODY) if e[3]) and hit[3] == [0, 0], hit
    assert [tr[-1]["obstacle_stats"]["n"] for tr in snaps] == [e[3] for e in hc.CONTROLLER_BODY]


# ---- ParticleFilter -----------------------------------------------------------------------------------------------------------
def _frame(dim):
    return tpf.frame2() if dim == 2 else tpf.frame3(hc.STRIDE3)


def _pf_snap(pf, **more):
    return dict(more, get=pf.get(), info=_strip(pf.info()))


def _filter_checked(i, pf):
    dim, m = hc.FILTER[i]
    fr = _frame(dim)
    ck = tpf.Checked(hc.filter_poses(i), hc.FILTER_SEEDS[i], dim, pf=pf)
    tr = [_pf_snap(pf)]
    resampled = []
    for mo, kw in zip(hc.filter_motions(i), hc.FILTER_UPDATES):
        ck.predict(mo)
        tr.append(_pf_snap(pf))
        est, _ = ck.update(fr, **kw)
        resampled.append(est["resampled"])
        tr.append(_pf_snap(pf, estimate=est))
    assert any(resampled) == (m > 2) and not resampled[1], (i, resampled)
    return tr


def _filter_fresh(i):
    import gpismap_amd
    dim, m = hc.FILTER[i]
    fr = _frame(dim)
    pf = gpismap_amd.ParticleFilter()
    pf.init(hc.filter_poses(i), seed=hc.FILTER_SEEDS[i])
    tr = [_pf_snap(pf)]
    for mo, kw in zip(hc.filter_motions(i), hc.FILTER_UPDATES):
        pf.predict(mo)
        tr.append(_pf_snap(pf))
        tr.append(_pf_snap(pf, estimate=fr.update(pf, **kw)))
    return tr


def test_filter_one_handle_through_changing_particle_counts():
    """2-D 257 -> 4097 -> 1 -> 65 particles, 3-D 300, 2-D 257 again: per entry init, predict, update (resamples where m > 2: the
    three-launch scan, the ping-pong gather), predict, update (keeps L); L and the ancestors after an init with fewer particles."""
    import gpismap_amd
    pf = gpismap_amd.ParticleFilter()
    _run(len(hc.FILTER), lambda i: _filter_checked(i, pf), _filter_fresh)


# ---- Coverage -----------------------------------------------------------------------------------------------------------------
def _cover_calls(e, cv, rf, ref=None):
    df, dist = _field(e["field"])
    l = hc.FIELDS[e["field"]][0]
    assert cv.reset(df) is cv and cv.get().sum() == 0 and cv.info()["frames"] == 0 and cv.info()["frontiers"] == 0
    if "depth" in e:
        cv.integrate_depth(e["depth"], e["pose"], e["cam"], **e["opts"])
    else:
        cv.integrate_scan(e["thetas"], e["ranges"], e["pose"], e["off2"], **e["opts"])
    seen = cv.get()
    if ref is not None:
        assert np.array_equal(seen.ravel(), ref["seen"].astype(np.uint8)), np.flatnonzero(seen.ravel() != ref["seen"])[:8]
        fr, _ = tcv._check_frontiers(cv, df, dist, ref["seen"], **e["opts"])
    else:
        fr = cv.frontiers(df, points=True, **e["opts"])
    assert cv.restrict(df, out=rf) is rf
    rd = rf.get()
    samples = rf.sample(hc.sample_points(l))
    if ref is not None:
        assert rf.info() == df.info() and rd[2] is None
        assert tpl._bits_equal(rd[0].ravel(), ref["restricted"]) and np.array_equal(rd[1], df.get()[1])
        assert tpl._bits_equal(samples, ref["samples"])
    return dict(seen=seen, frontiers=fr, restricted=rd, samples=samples, info=_strip(cv.info()), out_info=rf.info())


def test_coverage_one_handle_through_reset_on_four_lattices():
    """60 x 40 with a scan, 24 x 20 x 16 with a depth frame (more than one chunk of lattice points, more than one block of frontier
    points, more components than before), 9 x 7 whose scan has fewer than two valid beams (no frontier point, no table), 60 x 40
    again; per entry reset, integrate, get, frontiers with their points, and restrict into one long-lived field that is sampled."""
    import gpismap_amd
    cv, rf = gpismap_amd.Coverage(), gpismap_amd.DistanceField()

    def entry(i):
        e = hc.COVERAGE[i]
        return _cover_calls(e, cv, rf, hc.coverage_ref(e, _field(e["field"])[1]))

    _run(len(hc.COVERAGE), entry, lambda i: _cover_calls(hc.COVERAGE[i], gpismap_amd.Coverage(), gpismap_amd.DistanceField()))
    assert cv.info()["points"] > 0


# ---- ViewScorer ---------------------------------------------------------------------------------------------------------------
def _view_snap(v):
    inf = v.info()
    return dict(get=v.get(), predicted=[v.predicted(k) for k in range(inf["poses"])], info=_strip(inf))


def _view_calls(e, v, check):
    df, dist = _field(e["field"])
    cv = tcv._cover(df).set(e["seen"])
    if check:
        tvw._check(df, dist, e["seen"], e["sensor"], e["poses"], cv=cv, v=v, **e["opts"])
    elif len(hc.FIELDS[e["field"]][0]["shape"]) == 3:
        df.view_gain_depth(cv, e["sensor"], e["poses"], scorer=v, **e["opts"])
    else:
        df.view_gain_scan(cv, e["sensor"][0], e["poses"], e["sensor"][1], scorer=v, **e["opts"])
    return _view_snap(v)


def test_view_scorer_one_handle_through_changing_batches():
    """2-D 65 poses of 90 beams on a half-seen mask, 3-D 3 poses of 13 x 7 pixels, 2-D 1 pose of 23 beams on a mask without an
    unseen point (no target: no gather), the first again.  info()["samples"] is read from the word after the last gain, which
    after a call with more poses lies inside the old gains; only the fresh handle states what it must be."""
    import gpismap_amd
    assert (hc.SMALL2, hc.SMALL3, hc.CAM13) == (tvw.SMALL2, tvw.SMALL3, tvw.CAM13)          # (the shapes test_gpu_view.py runs)
    v = gpismap_amd.ViewScorer()
    snaps = []

    def entry(i):
        snaps.append(_view_calls(hc.VIEW[i], v, True))
        return snaps[-1]

    _run(len(hc.VIEW), entry, lambda i: _view_calls(hc.VIEW[i], gpismap_amd.ViewScorer(), False))
    assert [s["info"]["targets"] > 0 for s in snaps] == [True, True, False, True]
    assert all(s["info"]["samples"] > 0 and s["get"][0].max() > 0 for s in snaps[:2])


# ---- Locator, Tracker, Renderer: the field paths ------------------------------------------------------------------------------
def _scene_field(dim):
    return tlo.df2() if dim == 2 else tlo.df3()


def _locator_calls(e, loc, check):
    df, dist = _scene_field(e["dim"])
    if e["dim"] == 3:
        out = df.score_depth(depth3(), e["poses"], CAM, locator=loc, stride=e["stride"])
    else:
        out = df.score_scan(TH2, e["ranges"], e["poses"], OFF2, locator=loc)
    if check:
        tlo._check(out, hc.locator_ref(e, dist), "locator, m %d" % len(e["poses"]))
    return dict(out=out, held=loc.get(), info=_strip(loc.info()))


def test_locator_one_handle_through_changing_batches():
    """score_* with locator=: 2-D 300 and 5000 poses of 270 beams, 3-D 3 poses at stride 8, 2-D 1 pose of 37 beams, the first
    again."""
    import gpismap_amd
    loc = gpismap_amd.Locator()
    _run(len(hc.LOCATOR), lambda i: _locator_calls(hc.LOCATOR[i], loc, True), lambda i: _locator_calls(hc.LOCATOR[i], gpismap_amd.Locator(), False))


def _tracker_calls(e, t, check):
    df, dist = _scene_field(e["dim"])
    if e["dim"] == 3:
        out = df.track_depth(depth3(), e["pose0"], CAM, tracker=t, **e["opts"])
    else:
        out = df.track_scan(TH2, e["ranges"], e["pose0"], OFF2, tracker=t, **e["opts"])
    if check:
        _check_track(out, hc.tracker_ref(e, dist), "tracker, dim %d" % e["dim"])
    return dict(pose=out[0], result=_strip(out[1]), held=_strip(t.result()))


def test_tracker_field_path_one_handle_from_many_segments_to_one():
    """3-D at stride 2 (1200 points: five segments of partial sums), 2-D 270 beams (two), 2-D 37 beams (one), the first again."""
    import gpismap_amd
    t = gpismap_amd.Tracker()
    snaps = []

    def entry(i):
        snaps.append(_tracker_calls(hc.TRACKER[i], t, True))
        return snaps[-1]

    _run(len(hc.TRACKER), entry, lambda i: _tracker_calls(hc.TRACKER[i], gpismap_amd.Tracker(), False))
    pts = [s["result"]["points"] for s in snaps]
    assert pts[0] > 2 * hc.SEGMENT and pts[1] > hc.SEGMENT > pts[2] > 0, pts


def _renderer_calls(e, r, check):
    df, _ = _scene_field(e["dim"])
    r.set_field_tiles(e["tiles"])
    if e["dim"] == 3:
        out, _, ref = trf._both3(df, e["pose"], e["cam"], r=r) if check else (df.render_depth(e["pose"], e["cam"], renderer=r), r, None)
    else:
        out, _, ref = trf._both2(df, e["thetas"], e["pose"], OFF2, r=r) if check else (df.render_scan(e["thetas"], e["pose"], OFF2, renderer=r), r, None)
    if check:
        trf._check_bits(out, r, ref, "renderer, dim %d, %d rays" % (e["dim"], out[0].size))
    return dict(out=out, held=r.get(), info=_strip(r.info()))


def test_renderer_field_path_one_handle_through_changing_frames():
    """3-D 80 x 60, 13 x 7 with the other thread-to-pixel mapping, 2-D 360 and 23 beams, the first again."""
    import gpismap_amd
    r = gpismap_amd.Renderer()
    _run(len(hc.RENDERER), lambda i: _renderer_calls(hc.RENDERER[i], r, True), lambda i: _renderer_calls(hc.RENDERER[i], gpismap_amd.Renderer(), False))


# ---- DistanceField ------------------------------------------------------------------------------------------------------------
def _dfield_calls(name, df, check):
    fd = hc.field(name)
    shape, origin, step = hc.lat(fd)
    tpl._field(fd["f"].copy(), shape, origin, step, df=df)
    got = df.get()
    x = hc.sample_points(fd)
    samples = df.sample(x)
    if check:
        rd, rs = hc.ref_field(name)
        assert got[2] is None and tpl._bits_equal(got[0].ravel(), rd) and np.array_equal(got[1].ravel(), rs)
        assert tpl._bits_equal(samples, dfield_ref.sample(rd, shape, origin, step, x))
        inf = df.info()
        assert inf["dim"] == len(shape) and inf["shape"] == tuple(shape) and inf["step"] == F32(step)
        assert np.isnan(samples[-1, 0]) and np.isnan(samples[-2, 0])                                # outside
        assert np.isfinite(samples[-4, 0]) == bool((rs >= 0).any())                                 # the last cell
    return dict(get=got, samples=samples, info=df.info())


def test_distance_field_rebuilt_on_one_handle():
    """from_grid on one handle: 60 x 40, 24 x 20 x 16, 9 x 7 without a site, 60 x 40 again; get() and sample() (the last cell, the
    outside) after each.  A plan and a batch of trajectories taken from the first field stay readable through every rebuild."""
    import gpismap_amd
    df = gpismap_amd.DistanceField()
    first = _dfield_calls(hc.DFIELD[0], df, True)
    _same(first, _dfield_calls(hc.DFIELD[0], gpismap_amd.DistanceField(), False), "entry 0 against a fresh handle")
    fd = hc.field(hc.DFIELD[0])
    shape, origin, step = hc.lat(fd)
    starts = tpl._pts([(55, 35), (10, 30), (3, 3)], origin, step)
    pl, pb, rc, rp = tpl._solve_vs_ref(df, first["get"][0].ravel(), shape, origin, step, tpl._pts([(5, 5)], origin, step), clearance=0.0)
    paths = tpl._paths_vs_ref(pl, pb, rc, rp, starts, None)
    tj = pl.trajectories(33).optimize(df, iters=5)
    held = dict(plan=pl.get(), traj=tj.get())
    assert paths[2][0] == 0 and held["traj"]["status"][0] != 2 and np.isfinite(held["traj"]["x"][0]).all()
    for i in range(1, len(hc.DFIELD)):
        got = _dfield_calls(hc.DFIELD[i], df, True)
        _same(got, _dfield_calls(hc.DFIELD[i], gpismap_amd.DistanceField(), False), "entry %d against a fresh handle" % i)
        _same(dict(plan=pl.get(), traj=tj.get()), held, "the plan and the trajectories after rebuild %d" % i)
        _same(tpl._paths_vs_ref(pl, pb, rc, rp, starts, None), paths, "paths after rebuild %d" % i)
    _same(got, first, "the last entry against the first")


# ---- one session --------------------------------------------------------------------------------------------------------------
SESSION_KEYS = ("df", "rf", "cv", "r", "v", "pl", "tj", "ctl", "pf", "loc", "t", "ob", "fp", "pp", "pj")


def _handles(dim):
    """The session's handles: the eleven field consumers, a set of moving balls, a footprint and, in 2-D, a pose planner with the
    Planner its projection goes into."""
    import gpismap_amd as g
    step = (hc.SMALL2 if dim == 2 else hc.SMALL3)["step"]
    return dict(df=g.DistanceField(), rf=g.DistanceField(), cv=g.Coverage(), r=g.Renderer(), v=g.ViewScorer(), pl=g.Planner(),
                tj=g.Trajectories(), ctl=g.Controller(), pf=g.ParticleFilter(), loc=g.Locator(), t=g.Tracker(),
                ob=g.Obstacles(dim, step), fp=g.Footprint(dim), pp=g.PosePlanner() if dim == 2 else None, pj=g.Planner() if dim == 2 else None)


def _round(h, name, k, stream):
    """One round of the session on the named field with the handles h, every call that takes a stream on `stream` (0: the default
    stream).  Returns every output."""
    import gpismap_amd
    L = gpismap_amd.lib()
    fd = hc.field(name)
    shape, origin, step = hc.lat(fd)
    dim = len(shape)
    sv = _void(stream)
    df, rf, cv, r, v, pl, tj, ctl, pf, loc, t, ob, fp, pp, pj = (h[key] for key in SESSION_KEYS)
    out = {}
    pose = hc.session_pose(name)
    off = np.array((0.03, -0.02), F32)
    # 1, 2: the field, the mask
    val = tpl._dev(fd["f"].copy())
    df.from_grid(val.data_ptr(), shape, origin, step, 0.0, stream=stream)
    out["field"] = df.get()
    cv.reset(df)
    # 3: a frame from the pose; a ray without a return is measured short of the scene's far side
    if dim == 2:
        assert trf._call2(L, None, df, r, TH2, pose, off2=off, stream=sv) == 0
    else:
        assert trf._call3(L, None, df, r, pose, cam6=CAM, stream=sv) == 0
    out["frame"] = r.get()
    out["frame_info"] = _strip(r.info())
    meas = np.where(out["frame"][2] == 0, out["frame"][0], F32(0.3 if dim == 2 else 1.2)).astype(F32)
    # 4 - 6: integrate, frontiers, restrict
    if dim == 2:
        cv.integrate_scan(TH2, meas, pose, off, stream=stream)
    else:
        cv.integrate_depth(meas, pose, CAM, stream=stream)
    out["seen"] = cv.get()
    out["frontiers"] = cv.frontiers(df, points=True, stream=stream)
    assert cv.restrict(df, out=rf, stream=stream) is rf
    out["restricted"] = rf.get()
    out["cover_info"] = _strip(cv.info())
    # 7: the next view over 8 yaws
    start = pose[:dim]
    nv = df.next_view(cv, start, (TH2, off) if dim == 2 else CAM, hc.YAWS8, base_pose=pose if dim == 3 else None, planner=pl, out=rf, scorer=v)
    out["next_view"] = nv
    nc = nv[4]["label"].size
    if nc:
        out["view"] = _view_snap(v)
    # 8 - 10: a plan on the restricted field, paths, trajectories
    goals = nv[4]["rep"] if nc else np.asarray(start, F32)[None]
    pl.solve(rf, goals, stream=stream)
    out["plan"] = pl.get()
    out["plan_info"] = _strip(pl.info())
    seen_pts = np.flatnonzero(out["seen"].ravel())
    pick = seen_pts[np.linspace(0, seen_pts.size - 1, 6).astype(np.int64)] if seen_pts.size else np.zeros(1, np.int64)
    starts = np.concatenate([np.asarray(start, F32)[None], hc.cover_ref.lattice_points(pick, shape, origin, step)])
    out["paths"] = pl.paths(starts, stream=stream)
    pl.trajectories(33, trajectories=tj)
    tj.optimize(rf, stream=stream, iters=5)
    out["traj"] = tj.get()
    # the footprint along the trajectories; in 2-D the pose plan towards the same goals, its paths and its projection
    B = hc.session_body(name)
    fp.set(B["b"], B["rho"])
    out["traj_body"] = tj.body_clearance(fp, rf, clearance=0.0)
    if dim == 2:
        any_heading = lambda x: np.concatenate([np.asarray(x, F32), np.full((len(x), 1), -1, F32)], axis=1)
        pp.solve(rf, fp, any_heading(goals), H=16, stream=stream, clearance=0.0, margin=0.0, turn=2.5 * step)
        out["pose_plan"] = pp.get()
        out["pose_plan_info"] = _strip(pp.info())
        out["pose_paths"] = pp.paths(any_heading(starts), stream=stream)
        assert pp.project(pj) is pj
        out["projection"] = dict(plan=pj.get(), heading2=pp.heading2.copy(), info=_strip(pj.info()))
    # the timing, its controls, and the timed batch against three balls
    tm = tj.time(rf, stream=stream, **hc.session_timing(name))
    out["timing"] = tm
    out["controls"] = tj.controls(hc.SESSION_DT, 33)
    S = hc.session_balls(name)
    ob.set(S["c"], S["v"], S["r"], epoch=S["epoch"])
    out["check"] = tj.check(ob, hc.SESSION_DT, 66, t_begin=hc.SESSION_T0)
    # 11: the controller, seeded by follow from the first timed trajectory, two steps with a shift, the balls and the footprint in
    # every rollout, the clock moved on between the steps; the terminal cost is the projection's (2-D) / the plan's (3-D)
    p64 = pose.astype(F64)
    ctl.init(dim, 257, 33, seed=20 + k)
    timed = np.flatnonzero(tm["status"] == 0)
    out["follow"] = ctl.follow(tj, int(timed[0]), hc.SESSION_DT) if timed.size else None
    steps = []
    for j in range(2):
        if j:
            ctl.shift()
        u0, info = df.control(ctl, p64, planner=pj if dim == 2 else pl, stream=sv, obstacles=ob, t=hc.SESSION_T0 + j * hc.SESSION_DT, footprint=fp)
        steps.append(dict(u0=u0, info=_strip(info), obstacle=ctl.get_obstacle(), obstacle_stats=ctl.obstacle_stats()))
    out["control"] = dict(steps=steps, get=ctl.get(), info=_strip(ctl.info()))
    # 12: the filter, 13: 300 scored poses, 14: one tracking call
    d = np.linspace(-0.06, 0.06, 7)
    if dim == 2:
        th = math.atan2(float(pose[3]), float(pose[2]))
        grid = gpismap_amd.pose_grid2(float(pose[0]) + d, float(pose[1]) + d, th + np.linspace(-0.2, 0.2, 7))
    else:
        offs = np.stack(np.meshgrid(d, d, d[:5], indexing="ij"), axis=-1).reshape(-1, 3)
        grid = gpismap_amd.pose_grid3(pose, offs, [(0.0, 0.0, 0.0), (0.0, 0.02, 0.0)])
    assert grid.shape[0] >= 300
    pf.init(grid[:257], seed=30 + k)
    if dim == 2:
        pf.predict((0.004, 0.0, 0.01), stream=sv)
        est = pf.update_scan(df, TH2, meas, off, stream=sv)
        assert tlo._call2(L, None, df, loc, TH2, meas, grid[:300], off2=off, stream=sv) == 0
        rc, tp = ttf._call2(L, None, df, t, dict(thetas=TH2, ranges=meas), grid[5], off2=off, stream=sv)
    else:
        pf.predict(hc.MOTION3, stream=sv)
        est = pf.update_depth(df, meas, CAM, stream=sv)
        assert tlo._call3(L, None, df, loc, meas, grid[:300], cam6=CAM, stream=sv) == 0
        rc, tp = ttf._call3(L, None, df, t, meas, grid[5], cam6=CAM, stream=sv)
    assert rc == 0
    out["filter"] = _pf_snap(pf, estimate=est)
    out["score"] = dict(held=loc.get(), info=_strip(loc.info()))
    out["track"] = dict(pose=tp, result=_strip(t.result()))
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_one_session_of_long_lived_handles(dim):
    """A single set of handles (field, restricted field, Coverage, Renderer, ViewScorer, Planner, Trajectories, Controller,
    ParticleFilter, Locator, Tracker, Obstacles, Footprint and, in 2-D, a PosePlanner with the Planner of its projection) through
    rounds on different lattices -- 2-D 60 x 40, 150 x 130, 33 x 20; 3-D 24 x 20 x 16, 13 x 11 x 9 -- on one caller's stream; per
    round from_grid, reset, render a frame, integrate it, frontiers, restrict, next_view over 8 yaws, plan, paths, trajectories,
    the footprint along them, the pose plan with its paths and its projection (2-D), the timing, its controls, the timed batch
    against three balls, follow, two controller steps with the balls and the footprint, a filter step, 300 scored poses and one
    tracking call.  Every output equals that of a set made anew for the round on the default stream.  This test compares handles
    with handles: the tests above tie fresh handles to the references on the inputs of history_cases, and
    tests/test_gpu_nav_chain.py ties a chain like this one to the references on the chain's own data."""
    import torch
    s = torch.cuda.Stream(device=0)
    h = _handles(dim)
    seen_something, later = 0, [0, 0]                         # rounds that followed a timed trajectory / whose balls hit rollouts
    for k, name in enumerate(hc.SESSION2 if dim == 2 else hc.SESSION3):
        got = _round(h, name, k, s.cuda_stream)
        _same(got, _round(_handles(dim), name, k, 0), "round %d on %s" % (k, name))
        print("round %d on %s: %d rays hit, %d seen, %d frontier points in %d clusters, plan reaches %d, filter N_eff %.1f, %d inliers tracked"
              % (k, name, int((got["frame"][2] == 0).sum()), int(got["seen"].sum()), got["frontiers"]["npoints"], got["frontiers"]["label"].size,
                 got["plan_info"]["reachable"], got["filter"]["estimate"]["neff"], got["track"]["result"]["inliers"]))
        st = [x["obstacle_stats"] for x in got["control"]["steps"]]
        print("   %d trajectories timed, %d collide with the body, %d with a ball; followed: %s; balls hit %s rollouts of 257%s"
              % (int((got["timing"]["status"] == 0).sum()), int(got["traj_body"]["collides"].sum()), int(got["check"]["collides"].sum()),
                 got["follow"] is not None, [x["dyn_hit_rollouts"] for x in st],
                 "; pose plan reaches %d states" % got["pose_plan_info"]["reachable"] if dim == 2 else ""))
        assert all(x["n"] == 3 for x in st)
        seen_something += int(got["seen"].sum() > 0 and (got["frame"][2] == 0).any() and got["plan_info"]["reachable"] > 0)
        later[0] += int(got["follow"] is not None and (got["timing"]["status"] == 0).any())
        later[1] += int(any(x["dyn_hit_rollouts"] > 0 for x in st))
    assert seen_something >= 2
    assert later[0] >= 1 and later[1] >= 1, later
