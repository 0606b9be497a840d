"""Inputs shared by tests/test_body_time_ref.py (CPU: the reference, its branches and its defective variants) and
tests/test_gpu_body_time.py (the device against the reference): the timed trajectories and sets of tests/retime_cases.py and
tests/obst_cases.py with footprints of tests/body_ref.py.  A case is retime_cases' dict plus body."""
import functools
import math

import numpy as np

import body_ref
import body_time_ref as btr
import obst_cases as oc
import obst_ref
import retime_cases as rc
import retime_ref
import timing_cases as tc

F64 = np.float64
BASE = dict(rc.BASE)                                     # slot 0.25, max_pause 63, clearance 0.25, press_on 0


def body(dim, nb):
    """A footprint of nb balls: one ball off the reference point, else body_ref.box(1.0, 0.4, nb)'s row of discs (3-D: the same
    offsets with heights alternating about the reference point)."""
    if nb == 1:
        off = np.zeros((1, dim))
        off[0, 0], off[0, 1] = -0.3, 0.1
        return body_ref.make(dim, off, [0.2])
    b = body_ref.box(1.0, 0.4, nb)
    if dim == 2:
        return b
    off = np.zeros((nb, 3))
    off[:, :2] = b["b"]
    off[:, 2] = 0.1 * (np.arange(nb) % 3 - 1)
    return body_ref.make(3, off, b["rho"])


# ---- the scene of DESIGN.md §7x's table ------------------------------------------------------------------------------------------
BOX = (1.0, 0.4, 5)
R_IN, R_DISC, R_OUT = 0.2, math.hypot(0.2, 0.1), math.hypot(0.5, 0.2)     # inscribed, one disc's, circumscribed


@functools.lru_cache(maxsize=None)
def table_scene(velocity=(0.0, 0.3)):
    """The free line (A = 70 own slots at slot 0.25) with body_ref.box(1.0, 0.4, 5) against a disc of radius 0.4 through the
    robot's place at half its duration; clearance 0.25.  dict(case, rows): rows name -> (schedule, the body's check along it)
    for the body solve and the point solves with the clearance raised by the inscribed radius, one disc's radius and the
    circumscribed radius."""
    x, v, t, st, pos, dur = rc.line()
    S = rc.through(pos, [0.5 * dur], [velocity], 0.4)
    b = body_ref.box(*BOX)
    case = dict(x=x, v=v, t=t, status=st, obst=S, t_begin=0.0, opts=dict(BASE), body=b)
    rows = {}
    for name, extra in (("body", None), ("inscribed", R_IN), ("disc", R_DISC), ("circumscribed", R_OUT)):
        if extra is None:
            sch = btr.solve(x, v, t, st, S, b, 0.0, BASE)
        else:
            sch = retime_ref.solve(x, v, t, st, S, 0.0, dict(BASE, clearance=BASE["clearance"] + extra))
        steps = int(sch["arrive"][0]) if sch["status"][0] <= 1 else 1
        rows[name] = (sch, btr.sched_check(x, v, t, st, sch, S, b, steps, BASE["clearance"]))
    return dict(case=case, rows=rows)


def parked_beside():
    """A parked disc of radius 0.3 at 0.9 beside the line: 0.9 - 0.3 - R_DISC = 0.376 >= 0.25 from the body (status 0), 0.0615 from
    the circumscribed point for ever (status 3)."""
    x, v, t, st, pos, dur = rc.line()
    S = obst_ref.make(2, [pos(0.5 * dur) + np.array([0.0, 0.9])], [(0.0, 0.0)], [0.3], epoch=0.0, step=0.25)
    return dict(x=x, v=v, t=t, status=st, obst=S, t_begin=0.0, opts=dict(BASE), body=body_ref.box(*BOX))


TWO = dict(off=[(0.3, 0.0), (-0.6, 0.0)], rho=[0.1, 0.1])   # a front ball and a rear ball 0.6 behind the reference point


def rear_only():
    """A small fast disc along y through the place of the rear ball of TWO at tau = 10.5 slots (the middle of an interval): it
    clears the reference point and the front ball by more than the clearance and hits the rear ball alone.  A check case."""
    x, v, t, st, pos, dur = rc.line()
    b = body_ref.make(2, TWO["off"], TWO["rho"])
    tau = 10.5 * rc.SLOT
    at = pos(tau) + np.array([-0.6, 0.0])
    S = obst_ref.make(2, [at - np.array([0.0, 8.0]) * tau], [(0.0, 8.0)], [0.05], epoch=0.0, step=0.25)
    return dict(x=x, v=v, t=t, status=st, obst=S, body=b, dt=rc.SLOT, steps=40, t0=0.0, t_begin=0.0, clearance=0.25)


FRONT = dict(off=[(0.8, 0.0)], rho=[0.1])                   # one ball far ahead of the reference point


@functools.lru_cache(maxsize=None)
def turn_knot():
    """The corner curve (2-D: along y, then along x) with FRONT and a parked disc of radius 0.05 on the middle of the chord the
    front ball's centre takes across the first own slot whose pose and its successor's have different headings: that play cell
    is blocked, the pause cells at its two ends are free.  dict(case, a): a is that own slot."""
    xx, tm = oc.timed_curves(2, 64)
    k = tc.NAMES.index("corner")
    x, v, t, st = xx[k:k + 1], tm["v"][k:k + 1], tm["t"][k:k + 1], tm["status"][k:k + 1]
    b = body_ref.make(2, FRONT["off"], FRONT["rho"])
    xs, vs, ts = x[0].astype(F64), v[0].astype(F64), t[0].astype(F64)
    A = retime_ref.own_slots(ts[-1], rc.SLOT)
    Q = btr.poses(xs, vs, ts, [F64(a) * F64(rc.SLOT) for a in range(A + 1)])
    a = int(np.flatnonzero((Q[1:, 2:] != Q[:-1, 2:]).any(axis=1))[0])
    W = btr.ball_tracks(b, Q)[:, 0]
    S = obst_ref.make(2, [0.5 * (W[a] + W[a + 1])], [(0.0, 0.0)], [0.05], epoch=0.0, step=0.25)
    return dict(case=dict(x=x, v=v, t=t, status=st, obst=S, t_begin=0.0, opts=dict(BASE, clearance=0.1), body=b), a=a)


def special_cases():
    """name -> solve case: retime_cases' special cases with a footprint, and this module's own."""
    sp = rc.special_cases()
    box = body_ref.box(*BOX)
    out = {k: dict(sp[k], body=box) for k in ("clear", "crossing", "crossing_late", "two_discs", "parked", "short_of_pauses", "tunnel",
                                                "empty", "point", "a1025", "statuses", "batch")}
    out["table"] = table_scene()["case"]
    out["parked_beside"] = parked_beside()
    out["turn_knot"] = turn_knot()["case"]
    out["batch_late"] = dict(sp["batch"], opts=dict(BASE, press_on=1), body=body(2, 2))
    return out


def ref_solve(c, variant=None, trace=None, keep=None):
    return btr.solve(c["x"], c["v"], c["t"], c["status"], c["obst"], c["body"], c["t_begin"], c["opts"], variant, trace, keep)


def ref_check(c, variant=None, trace=None):
    return btr.check(c["x"], c["v"], c["t"], c["status"], c["obst"], c["body"], c["dt"], c["steps"], c["t0"], c["t_begin"], c["clearance"],
                     variant, trace)


# ---- shapes for the device ------------------------------------------------------------------------------------------------------
# (m, N, P, n, A, body balls): retime_cases' shapes with 1, 2, 5, 15 and 16 body balls; the largest A, P, n and body never meet.
SHAPES = ((1, 64, 0, 1, 0, 1), (1, 3, 1, 2, 1, 2), (11, 64, 62, 65, 63, 5), (11, 256, 63, 2, 64, 16), (11, 64, 64, 256, 65, 1),
          (11, 3, 255, 1, 63, 15), (600, 64, 1, 2, 64, 5), (11, 64, 63, 0, 65, 5), (1, 64, 255, 65, 65, 2))
SHAPES3 = ((11, 64, 64, 65, 64, 5), (1, 256, 63, 2, 65, 16))
LONG = (1, 64, 255, 2, 1024, 2)                          # one row of A = 1024


def shape_case(m, N, P, n, A, nb, dim=2):
    return dict(rc.shape_case(m, N, P, n, A, dim), body=body(dim, nb))


# (m, N, steps, n, body balls): steps in {1, 64, 1024, 1025} (the kernel takes its intervals 1024 at a time), n in {0, 1, 65, 256},
# body balls in {1, 2, 16}
CHECK_SHAPES = ((1, 3, 1, 1, 1), (11, 64, 64, 65, 2), (3, 64, 1024, 1, 16), (3, 256, 1025, 65, 2), (11, 64, 64, 256, 16), (3, 64, 1025, 0, 2),
                (11, 3, 64, 65, 1))
CHECK_SHAPES3 = ((11, 64, 64, 65, 16), (3, 64, 1025, 1, 2))


def check_shape_case(m, N, steps, n, nb, dim=2):
    c = oc.check_shape_case(m, N, steps, max(n, 1), dim)
    if n == 0:
        c["obst"] = obst_ref.make(dim, [], [], [], epoch=1.25, step=0.2 if dim == 3 else 0.25)
        c["clearance"] = 0.25
    return dict(c, body=body(dim, nb))


@functools.lru_cache(maxsize=None)
def _dup_end():
    import mppi_cases as mc
    import timing_ref
    sc = mc.scene(2)
    x = tc.curves(sc, 64)[tc.NAMES.index("free")][None].copy()
    x[0, 62:] = x[0, 61]                                 # the last two chords have no length
    tm = timing_ref.time(x, np.zeros(1, np.uint8), tc.opts(sc), (sc["dist"], sc["shape"], sc["origin"], sc["step"]))
    return x, tm


def dup_end():
    """The free line with its last three waypoints equal (timing status 0: a segment of no length takes no time), sampled past
    its end, where the chord rule searches backward: a check case."""
    x, tm = _dup_end()
    dur = float(tm["t"][0, -1])
    end = x[0, -1].astype(F64)
    S = obst_ref.make(2, [end + np.array([0.0, 1.0])], [(0.0, 0.0)], [0.2], epoch=0.0, step=0.25)
    return dict(x=x, v=tm["v"], t=tm["t"], status=tm["status"], obst=S, body=body(2, 5), dt=0.5, steps=int(dur / 0.5) + 4, t0=0.0, t_begin=0.0,
                clearance=0.25)


def knot_case():
    """The curves (N = 64) at a step that puts tau_4 on a knot, sampled past every duration's end: dict as check_shape_case's."""
    x, v, t, st = oc.batch(2, 11, 64)
    dt = tc.knot_dts(t, st)[0]
    steps = int(math.ceil(float(np.nanmax(t[st == 0][:, -1])) / dt)) + 3
    return dict(x=x, v=v, t=t, status=st, obst=oc.balls(2, 2, 0.25), body=body(2, 2), dt=dt, steps=min(steps, 4096), t0=0.0, t_begin=oc.T_NOW,
                clearance=None)
