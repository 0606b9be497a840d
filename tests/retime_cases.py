"""Inputs shared by tests/test_retime_ref.py (CPU: the reference, its branches and its defective variants) and
tests/test_gpu_retime.py (the device against the reference): timed trajectories of tests/obst_cases.py (the curves of
tests/timing_cases.py with the reference's timing) against sets of moving balls aimed at them.  A case is dict(x, v, t, status,
obst, t_begin, opts, expect): `expect` names what the case is for -- the status of row 0 and trace counters of
retime_ref.solve that must be reached."""
import numpy as np

import obst_cases as oc
import obst_ref
import retime_ref

F64 = np.float64
SLOT = 0.25
BASE = dict(slot=SLOT, max_pause=63, clearance=0.25, press_on=0)


def line():
    """(x, v, t, status, pos, duration) of the free straight line along x (one row, N = 64, timing status 0)."""
    return oc._free_line()


def slot_for(duration, A):
    """A slot with retime_ref.own_slots(duration, slot) == A >= 1."""
    slot = float(duration) / A * (1.0 + 2.0 ** -40)
    assert retime_ref.own_slots(duration, slot) == A, (duration, A)
    return slot


def through(pos, tau, velocity, radius, **opts):
    """A set of balls, each through the robot's timed position at trajectory time tau[i] at that time (t_begin = 0), with the
    given velocities."""
    tau = np.atleast_1d(np.asarray(tau, F64))
    vel = np.asarray(velocity, F64).reshape(tau.size, -1)
    c = np.stack([pos(tk) - vel[i] * tk for i, tk in enumerate(tau)])
    return obst_ref.make(vel.shape[1], c, vel, np.broadcast_to(np.asarray(radius, F64), tau.shape), epoch=0.0, step=0.25, **opts)


def special_cases():
    """name -> case on the free line (row 0) unless said otherwise."""
    x, v, t, st, pos, dur = line()
    base = dict(x=x, v=v, t=t, status=st, t_begin=0.0)
    far = obst_ref.make(2, [(0.0, 40.0)], [(0.0, 0.0)], [0.3], epoch=0.0, step=0.25)
    cross1 = through(pos, [0.5 * dur], [(0.0, 0.3)], 0.4)
    cross2 = through(pos, [0.5 * dur, 0.33 * dur], [(0.0, 0.3), (0.0, -0.25)], 0.4)
    parked = through(pos, [0.5 * dur], [(0.0, 0.0)], 0.3)
    # the slow disc makes the robot wait short of the middle (press_on: as late as allowed); a small fast one then goes through
    # the place of the third of those waits in the middle of its slot: 1 m away at both of the slot's samples
    late = retime_ref.solve(x, v, t, st, cross1, 0.0, dict(BASE, press_on=1, clearance=0.1))
    own = late["own"][0]
    waits = [k for k in range(int(late["arrive"][0])) if own[k + 1] == own[k]]
    k_w = waits[2]
    at = pos(F64(int(own[k_w])) * F64(SLOT))
    fast = through(pos, [0.5 * dur, (k_w + 0.5) * SLOT], [(0.0, 0.3), (0.0, 8.0)], [0.4, 0.05])
    fast["c"][1] = at - np.array([0.0, 8.0]) * ((k_w + 0.5) * SLOT)
    x11, v11, t11, st11 = oc.batch(2, 11, 64)
    x3, v3, t3, st3 = oc.batch(2, 11, 3)
    import timing_cases as tc
    k = tc.NAMES.index("point")
    point = dict(x=x11[k:k + 1], v=v11[k:k + 1], t=t11[k:k + 1], status=st11[k:k + 1], t_begin=0.0)
    return {
        "clear": dict(base, obst=far, opts=dict(BASE), expect=dict(status=0, counters=("status0", "play"))),
        "crossing": dict(base, obst=cross1, opts=dict(BASE), expect=dict(status=1, counters=("status1", "pause", "play"))),
        "crossing_late": dict(base, obst=cross1, opts=dict(BASE, press_on=1), expect=dict(status=1, counters=("status1", "both"))),
        "two_discs": dict(base, obst=cross2, opts=dict(BASE), expect=dict(status=1, counters=("status1",))),
        "parked": dict(base, obst=parked, opts=dict(BASE), expect=dict(status=3, counters=("status3",))),
        "short_of_pauses": dict(base, obst=cross1, opts=dict(BASE, max_pause=2), expect=dict(status=3, counters=("status3",))),
        "tunnel": dict(base, obst=fast, opts=dict(BASE, press_on=1, clearance=0.1), expect=dict(status=1, counters=("status1",))),
        "empty": dict(base, obst=obst_ref.make(2, [], [], []), opts=dict(BASE), expect=dict(status=0, counters=("n0",))),
        "point": dict(point, obst=far, opts=dict(BASE), expect=dict(status=0, counters=("status0",))),
        "a1024": dict(base, obst=cross1, opts=dict(BASE, slot=slot_for(dur, 1024), max_pause=255), expect=dict(status=1, counters=("status1",))),
        "a1025": dict(base, obst=cross1, opts=dict(BASE, slot=slot_for(dur, 1025)), expect=dict(status=4, counters=("status4",))),
        "statuses": dict(x=x3, v=v3, t=t3, status=st3, t_begin=oc.T_NOW, obst=oc.balls(2, 2, 0.25), opts=dict(BASE),
                         expect=dict(status=None, counters=("status2",))),
        "batch": dict(x=x11, v=v11, t=t11, status=st11, t_begin=oc.T_NOW, obst=oc.balls(2, 8, 0.25), opts=dict(BASE),
                      expect=dict(status=None, counters=("status0", "status1", "status2", "status3"))),
    }


def ref_solve(c, variant=None, trace=None, keep=None):
    return retime_ref.solve(c["x"], c["v"], c["t"], c["status"], c["obst"], c["t_begin"], c["opts"], variant, trace, keep)


# ---- shapes for the device ------------------------------------------------------------------------------------------------------
# (m, N, P, n, A), paired: P + 1 in {1, 2, 63, 64, 65, 256} (one lane, a wavefront's last lanes, its first lane of the next, every
# lane), A in {0 (m = 1 takes the point curve), 1, 63, 64, 65} through the slot (the own slots of the longest row; the other rows
# last shorter), n in {0, 1, 2, 65, 256}, m in {1, 11, 600}, N in {3, 64, 256}.  The largest A, P and n never meet.
SHAPES = ((1, 64, 0, 1, 0), (1, 3, 1, 2, 1), (11, 64, 62, 65, 63), (11, 256, 63, 2, 64), (11, 64, 64, 256, 65), (11, 3, 255, 1, 63),
          (600, 64, 1, 2, 64), (11, 64, 63, 0, 65), (1, 64, 255, 65, 65))
SHAPES3 = ((11, 64, 64, 65, 64), (1, 256, 63, 2, 65))
LONG = (1, 64, 255, 2, 1024)                            # one row of A = 1024


def shape_case(m, N, P, n, A, dim=2):
    """The curves tiled or cut to m rows (m = 1: the half circle; with A = 0 the point) against the scattered balls of
    obst_cases.balls, whose ball 0 crosses the scene; the slot gives the longest row A own slots."""
    import timing_cases as tc
    x, v, t, st = oc.batch(dim, m, N)
    if A == 0:
        k = tc.NAMES.index("point")
        xx, tm = oc.timed_curves(dim, N)
        x, v, t, st = xx[k:k + 1], tm["v"][k:k + 1], tm["t"][k:k + 1], tm["status"][k:k + 1]
        slot = SLOT
    else:
        dur = float(np.max(t[st == 0][:, -1]))
        slot = slot_for(dur, A)
    step = 0.2 if dim == 3 else 0.25
    obst = oc.balls(dim, n, step) if n else obst_ref.make(dim, [], [], [], epoch=1.25, step=step)
    return dict(x=x, v=v, t=t, status=st, obst=obst, t_begin=oc.T_NOW,
                opts=dict(slot=slot, max_pause=P, clearance=step, press_on=(m + N + P) & 1), expect=dict(status=None, counters=()))
