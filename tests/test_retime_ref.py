"""The re-timing's host side and its reference (tests/retime_ref.py) on the CPU: the exported C entries, the options the reference
and the library refuse, every branch of the contract on the shared cases (tests/retime_cases.py) counted by a trace, the
certificate (a schedule's own check is clear), the restated stages against their originals on the identity schedule, the
defective variants, and the closed loop of the references: planner -> smoother -> time -> retime -> controls -> the controller's
model, past a disc that crosses the timed position."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import mppi_ref
import obst_cases as oc
import obst_ref
import retime_cases as rc
import retime_ref as rr
import timing_cases as tc
import timing_ref
import traj_cases
import traj_ref

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_retime_default_opts", "gpis_retime_solve", "gpis_retime_get", "gpis_retime_controls", "gpis_retime_follow",
         "gpis_retime_check"}
SKEYS = rr.RES_KEYS + ("own",)


def _same_sched(a, b):
    return all(np.array_equal(a[k], b[k]) for k in SKEYS)


@functools.lru_cache(maxsize=None)
def _solved(name):
    """The contract's own result of a special case with its trace and tables: computed once, left unchanged."""
    c = rc.special_cases()[name]
    trace, keep = {}, {}
    return c, rc.ref_solve(c, trace=trace, keep=keep), trace, keep


# ---- exports --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_retime[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_retime_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_retime_opts)]
    for dim, step in ((2, 0.25), (3, 0.2), (2, 0.1)):
        o = gpismap_amd.gpis_retime_opts()
        assert L.gpis_retime_default_opts(dim, step, C.byref(o)) == 0
        assert {k: getattr(o, k) for k in rr.OPT_KEYS} == rr.default_opts(dim, step), (dim, step)
        p = gpismap_amd.retime_opts(dim, step, slot=0.25, press_on=1)
        assert p.slot == 0.25 and p.press_on == 1 and p.clearance == o.clearance and p.max_pause == 63
    assert rr.default_opts(2, 0.25) == dict(slot=0.1, max_pause=63, clearance=0.25, press_on=0)
    assert L.gpis_retime_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_retime_default_opts(2, 0.1, None) == -1
    assert L.gpis_retime_default_opts(2, 0.0, C.byref(o)) == -1
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.retime_opts(2, 0.25, pause=1.0)
    # a schedule lives on a handle, which lives on a device: without one the entries answer GPIS_ERR_ARG
    d, vp = C.c_double, C.c_void_p
    L.gpis_retime_solve.argtypes = [vp, vp, d, vp, vp]
    L.gpis_retime_get.argtypes = [vp] * 9
    L.gpis_retime_controls.argtypes = [vp, C.c_int, C.c_int, d, d] + [vp] * 4
    L.gpis_retime_follow.argtypes = [vp, vp, C.c_int, C.c_int, d, d, vp, vp]
    L.gpis_retime_check.argtypes = [vp, vp, C.c_int, d] + [vp] * 5
    assert L.gpis_retime_solve(None, None, 0.0, C.byref(o), None) == -1 and L.gpis_retime_get(*[None] * 9) == -1
    assert L.gpis_retime_controls(None, 4, 0, 0.0, 0.0, None, None, None, None) == -1
    assert L.gpis_retime_follow(None, None, 0, 0, 0.0, 0.0, None, None) == -1
    assert L.gpis_retime_check(None, None, 4, 0.1, None, None, None, None, None) == -1
    for meth in ("retime", "retimed", "retimed_controls", "retimed_check"):
        assert callable(getattr(gpismap_amd.Trajectories, meth)), meth
    assert gpismap_amd.Trajectories.OWN_LEN == rr.OWN_LEN == 1280 and (rr.MAX_OWN, rr.MAX_PAUSE) == (1024, 255)
    import inspect
    assert {"retimed", "k0"} <= set(inspect.signature(gpismap_amd.Controller.follow).parameters)


def test_the_reference_rejects_bad_options():
    c = rc.special_cases()["crossing"]
    for kw in (dict(slot=0.0), dict(slot=-0.25), dict(slot=np.nan), dict(slot=np.inf), dict(max_pause=-1), dict(max_pause=256),
               dict(max_pause=1.5), dict(clearance=-0.1), dict(clearance=np.nan), dict(press_on=2), dict(press_on=-1)):
        with pytest.raises(ValueError):
            rc.ref_solve(dict(c, opts=dict(c["opts"], **kw)))
    with pytest.raises(ValueError):
        rc.ref_solve(dict(c, t_begin=np.inf))
    with pytest.raises(ValueError):
        rc.ref_solve(dict(c, obst=oc.balls(3, 2, 0.2)))
    sched = _solved("crossing")[1]
    for kw in (dict(T=0), dict(T=257), dict(k0=-1), dict(w_limit=-1.0), dict(min_move=np.nan)):
        with pytest.raises(ValueError):
            rr.controls(c["x"], c["v"], c["t"], c["status"], sched, **dict(dict(T=4, k0=0, w_limit=0.0, min_move=0.0), **kw))
    for kw in (dict(steps=0), dict(steps=4097), dict(clearance=-1.0), dict(clearance=np.inf)):
        with pytest.raises(ValueError):
            rr.check(c["x"], c["v"], c["t"], c["status"], sched, c["obst"], **dict(dict(steps=8, clearance=0.1), **kw))
    # the least a with a * slot >= duration, at the edges
    assert rr.own_slots(0.0, 0.25) == 0 and rr.own_slots(0.25, 0.25) == 1 and rr.own_slots(0.2500001, 0.25) == 2
    assert rr.own_slots(256.0, 0.25) == 1024 and rr.own_slots(256.1, 0.25) == 1025 and rr.own_slots(1e30, 0.25) == 1025
    assert rr.own_slots(0.3, 0.1) == 3 and F64(3) * F64(0.1) >= F64(0.3) > F64(2) * F64(0.1)


# ---- every branch -----------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_its_branches():
    names = sorted(rc.special_cases())
    seen = set()
    for name in names:
        c, r, trace, _ = _solved(name)
        want = c["expect"]
        if want["status"] is not None:
            assert int(r["status"][0]) == want["status"], (name, r["status"])
        for k in want["counters"]:
            assert trace.get(k, 0) > 0, (name, k, trace)
        seen |= set(int(s) for s in r["status"])
        print("%-16s status %s arrive %s pauses %s own slots %s first pause %s %s" % (
            name, r["status"].tolist(), r["arrive"].tolist(), r["pauses"].tolist(), r["own_slots"].tolist(), r["first_pause"].tolist(), trace))
    assert seen == {0, 1, 2, 3, 4}
    # the issue's batch: eight rows clear as timed, one re-timed, one without a schedule within 63 pauses, one untimed
    b = _solved("batch")[1]
    assert sorted(b["status"].tolist()) == [0] * 8 + [1, 2, 3] and b["pauses"][b["status"] == 1].tolist() == [9]
    # clear as timed: the identity, as with no balls at all
    cl, em = _solved("clear")[1], _solved("empty")[1]
    assert _same_sched(cl, em) and cl["arrive"][0] == cl["own_slots"][0] and cl["first_pause"][0] == -1
    assert np.array_equal(em["own"][0], np.minimum(np.arange(rr.OWN_LEN), em["own_slots"][0]))
    # a parked ball leaves no schedule, and neither do too few pauses; the own slots are still reported
    for name in ("parked", "short_of_pauses"):
        r = _solved(name)[1]
        assert (r["status"][0], r["arrive"][0], r["pauses"][0], r["first_pause"][0]) == (3, -1, -1, -1) and r["own_slots"][0] == cl["own_slots"][0]
        assert np.all(r["own"][0] == -1)
    # the crossing disc: the plain check collides, the schedule waits and then plays every own slot once
    c, r, trace, keep = _solved("crossing")
    A, arrive, p = int(r["own_slots"][0]), int(r["arrive"][0]), int(r["pauses"][0])
    plain = obst_ref.check(c["x"], c["v"], c["t"], c["status"], c["obst"], c["opts"]["slot"], A, 0.0, 0.0, c["opts"]["clearance"])
    assert plain["collides"][0] == 1 and plain["min_sep"][0] < 0
    own = r["own"][0]
    assert arrive == A + p and p > 0 and own[0] == 0 and own[arrive] == A and np.all(own[arrive:] == A)
    assert set(np.diff(own[:arrive + 1]).tolist()) == {0, 1} and int((np.diff(own[:arrive + 1]) == 0).sum()) == p
    # press_on moves the pauses and not the arrival
    late = _solved("crossing_late")[1]
    assert late["arrive"][0] == arrive and late["pauses"][0] == p and not np.array_equal(late["own"][0], own)
    assert r["first_pause"][0] < late["first_pause"][0] and np.all(late["own"][0][:arrive + 1] >= own[:arrive + 1])
    # two separate groups of pauses
    assert _solved("tunnel")[2]["groups"] >= 2
    # the tunnelling ball: the cell it goes through is clear at both of its samples and not in between
    c, r, trace, keep = _solved("tunnel")
    clr, slot = c["opts"]["clearance"], c["opts"]["slot"]
    tun = dict(c["obst"], n=1, c=c["obst"]["c"][1:], v=c["obst"]["v"][1:], r=c["obst"]["r"][1:])
    pos = keep[0]["pos"]
    cells = [(a, p) for a in range(pos.shape[0]) for p in range(c["opts"]["max_pause"] + 1)
             if (rr.sep(pos[a], np.zeros(2), np.array([a + p]), tun, F64(0.0), slot) < clr).any()
             and not (rr.sep(pos[a], np.zeros(2), np.array([a + p]), tun, F64(0.0), slot, True) < clr).any()
             and not (rr.sep(pos[a], np.zeros(2), np.array([a + p + 1]), tun, F64(0.0), slot, True) < clr).any()]
    assert cells and all(not keep[0]["pause"][a, p] for a, p in cells)
    # A = 0: nothing to play and nothing to wait for; A = 1024 is the last length that is solved
    pt = _solved("point")[1]
    assert (pt["status"][0], pt["arrive"][0], pt["own_slots"][0]) == (0, 0, 0) and np.all(pt["own"][0] == 0)
    assert _solved("a1024")[1]["own_slots"][0] == 1024 and _solved("a1024")[1]["arrive"][0] > 1024
    long = _solved("a1025")[1]
    assert long["status"][0] == 4 and long["own_slots"][0] == -1 and np.all(long["own"][0] == -1)
    # rows without a timing
    st = _solved("statuses")
    assert set(st[0]["status"].tolist()) == {0, 2, 3} and np.array_equal(st[1]["status"] == 2, st[0]["status"] != 0)


def test_a_schedules_own_check_is_clear():
    """The certificate: with the solve's set and clearance and steps <= arrive, a schedule of status 0 or 1 does not collide
    and keeps min_sep >= clearance -- on every such row of every case."""
    rows = 0
    for name in sorted(rc.special_cases()):
        c, r, _, _ = _solved(name)
        for i in np.flatnonzero((r["status"] <= 1) & (r["arrive"] >= 1)):
            one = {k: (v[i:i + 1] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
            steps = min(int(r["arrive"][i]), 4096)
            k = rr.check(c["x"][i:i + 1], c["v"][i:i + 1], c["t"][i:i + 1], c["status"][i:i + 1], one, c["obst"], steps, c["opts"]["clearance"])
            assert k["collides"][0] == 0 and k["first_hit"][0] == -1, (name, i, k)
            assert c["obst"]["n"] == 0 or k["min_sep"][0] >= c["opts"]["clearance"], (name, i, k["min_sep"])
            rows += 1
    assert rows >= 20                                    # (seven single rows and the live rows of the two batches)
    c, r, _, _ = _solved("crossing")
    k = rr.check(c["x"], c["v"], c["t"], c["status"], r, c["obst"], int(r["arrive"][0]), c["opts"]["clearance"])
    print("crossing: waits %d slots from slot %d, closest approach %.4f at %.2f s" % (r["pauses"][0], r["first_pause"][0], k["min_sep"][0], k["min_time"][0]))


def test_the_restated_stages_are_the_originals_on_the_identity_schedule():
    c, ident, _, _ = _solved("empty")
    b = rc.special_cases()["batch"]
    ident11 = rr.solve(b["x"], b["v"], b["t"], b["status"], obst_ref.make(2, [], [], []), oc.T_NOW, b["opts"])
    slot = b["opts"]["slot"]
    for T, wl in ((1, 0.0), (65, 0.7), (256, 0.0)):
        mine = rr.controls(b["x"], b["v"], b["t"], b["status"], ident11, T, 0, wl, 1e-9)
        orig = timing_ref.controls(b["x"], b["v"], b["t"], b["status"], slot, T, 0.0, wl, 1e-9)
        for k in ("U", "heading0", "p0", "clamped"):
            assert np.array_equal(np.ascontiguousarray(mine[k]).view(np.uint8), np.ascontiguousarray(orig[k]).view(np.uint8)), (T, k)
    for steps in (1, 64, 300):
        mine = rr.check(b["x"], b["v"], b["t"], b["status"], ident11, b["obst"], steps, None)
        orig = obst_ref.check(b["x"], b["v"], b["t"], b["status"], b["obst"], slot, steps, 0.0, oc.T_NOW, None)
        for k in mine:
            assert np.array_equal(mine[k], orig[k], equal_nan=True), (steps, k)
    # a paused step has no displacement and keeps the heading of the latest moving step; past the arrival the robot rests
    c, r, _, _ = _solved("crossing_late")
    arrive = int(r["arrive"][0])
    u = rr.controls(c["x"], c["v"], c["t"], c["status"], r, 128, 0, 0.0, 1e-9)
    own = r["own"][0]
    paused = np.flatnonzero(own[1:129] == own[:128])
    assert paused.size > 128 - arrive and np.all(u["U"][0, paused] == 0.0)
    far = rr.controls(c["x"], c["v"], c["t"], c["status"], r, 8, arrive + 5, 0.0, 1e-9)
    assert not far["U"].any() and np.array_equal(far["p0"][0], c["x"][0, -1].astype(F64))
    mid = rr.controls(c["x"], c["v"], c["t"], c["status"], r, 16, 20, 0.0, 1e-9)
    assert np.array_equal(mid["p"][0], u["p"][0, 20:37])
    # a row without a schedule stands still, as one without a timing does
    p = _solved("parked")
    still = rr.controls(p[0]["x"], p[0]["v"], p[0]["t"], p[0]["status"], p[1], 8)
    assert not still["U"].any() and still["heading0"].tolist() == [[1.0, 0.0]] and np.array_equal(still["p0"][0], p[0]["x"][0, 0].astype(F64))
    k = rr.check(p[0]["x"], p[0]["v"], p[0]["t"], p[0]["status"], p[1], p[0]["obst"], 8, 0.1)
    assert np.isnan(k["min_sep"][0]) and np.isnan(k["min_time"][0]) and (k["min_obstacle"][0], k["first_hit"][0], k["collides"][0]) == (-1, -1, 0)


# ---- defective variants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,name", (("pause_sample", "tunnel"), ("pause_free", "crossing_late"), ("time_a", "crossing"),
                                          ("walk_swapped", "crossing")))
def test_defective_variant_changes_its_case(variant, name):
    c, r, _, _ = _solved(name)
    b = rc.ref_solve(c, variant)
    changed = [k for k in SKEYS if not np.array_equal(r[k], b[k])]
    print(variant, "changes", changed, "of", name)
    assert changed, (variant, name)
    if variant == "walk_swapped":                        # the same arrival by other pauses
        assert b["arrive"][0] == r["arrive"][0] and "own" in changed
    assert set(rr.VARIANTS) == {"pause_sample", "pause_free", "time_a", "walk_swapped"}


# ---- closed loop, the references alone ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def closed_loop_input():
    """Planner paths -> traj_ref.optimize -> time on the 2-D ball scene (four of the planner's trajectories), the longest of them,
    and the disc that crosses its timed position at mid-duration, perpendicular to the way it goes there."""
    sc = traj_cases.scene(2)
    dist = traj_cases.ref_dist(sc)
    _, _, _, off, pts, _, st = traj_cases.plan(sc, dist)
    x, ist = traj_ref.resample(off, pts, st, 64)
    live = np.flatnonzero(ist == 0)[:4]
    opt = traj_ref.optimize(dist, sc["shape"], sc["origin"], sc["step"], x[live], ist[live])
    tm = timing_ref.time(opt["x"], opt["status"], tc.opts(sc), (dist, sc["shape"], sc["origin"], sc["step"]))
    return sc, dist, opt["x"], tm


def crossing_disc(x, tm, r):
    xs, vs, ts = x[r].astype(F64), tm["v"][r].astype(F64), tm["t"][r].astype(F64)
    dur = float(ts[-1])
    pos = lambda tau: timing_ref.position(xs, vs, ts, F64(tau))
    d = pos(0.5 * dur + 0.05) - pos(0.5 * dur - 0.05)
    d = d / np.sqrt((d * d).sum())
    return rc.through(pos, [0.5 * dur], [(-0.3 * d[1], 0.3 * d[0])], 0.4)


def test_closed_loop_waits_for_a_crossing_disc():
    sc, dist, x, tm = closed_loop_input()
    r = int(np.argmax(np.where(tm["status"] == 0, tm["duration"], -1)))
    assert tm["status"][r] == 0 and tm["duration"][r] > 4.0
    disc = crossing_disc(x, tm, r)
    o = dict(rc.BASE)
    one = (x[r:r + 1], tm["v"][r:r + 1], tm["t"][r:r + 1], tm["status"][r:r + 1])
    A = rr.own_slots(tm["duration"][r], o["slot"])
    plain = obst_ref.check(*one, disc, o["slot"], A, 0.0, 0.0, o["clearance"])
    assert plain["collides"][0] == 1 and plain["min_sep"][0] < 0
    s = rr.solve(*one, disc, 0.0, o)
    assert s["status"][0] == 1 and s["pauses"][0] > 0
    T = int(s["arrive"][0])
    assert T <= timing_ref.MAX_T
    c = rr.controls(*one, s, T, 0, 0.0, 0.0)
    assert not c["clamped"].any()
    mo = dict(dt=o["slot"], gamma=0.0, sigma=(0.0,) * 4, umin=(-np.inf,) * 4, umax=(np.inf,) * 4, clearance=0.0, margin=0.0, w_obs=0.0,
              w_col=0.0, w_off=0.0, w_goal=0.0)
    start = np.concatenate([c["p0"][0], c["heading0"][0]])
    ro = mppi_ref.rollouts(dist, sc["shape"], sc["origin"], sc["step"], start, c["U"][0], np.zeros((1, T, 2)), mo, goal=np.zeros(2), states=True)
    visited = ro["states"][0, :, :2]
    bound = 64 * T * 2.0 ** -53 * max(1.0, float(np.abs(x[r]).max()))
    err = float(np.sqrt(((visited - c["p"][0]) ** 2).sum(axis=1)).max())
    sep = min(float((np.sqrt(((visited[k][None] - obst_ref.at(disc, k * o["slot"])) ** 2).sum(axis=1)) - disc["r"]).min()) for k in range(T + 1))
    k = rr.check(*one, s, disc, T, o["clearance"])
    print("plain check: %.3f at step %d; re-timed: waits %d slots from slot %d, arrives at slot %d of %d own; the model's rollout is within "
          "%.3g of the schedule (allowed %.3g), least separation at the steps %.4f, in continuous time %.4f"
          % (plain["min_sep"][0], plain["first_hit"][0], s["pauses"][0], s["first_pause"][0], T, A, err, bound, sep, k["min_sep"][0]))
    assert err <= bound, (err, bound)
    assert sep >= o["clearance"] - bound and k["collides"][0] == 0 and k["min_sep"][0] >= o["clearance"]
    assert np.sqrt(((visited[-1] - x[r, -1].astype(F64)) ** 2).sum()) <= bound           # it arrives
