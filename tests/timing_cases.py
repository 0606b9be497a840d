"""Inputs shared by tests/test_timing_ref.py (CPU: the reference against its defective variants, the closure with the
controller's model) and tests/test_gpu_timing.py (the device against the reference): waypoint batches on traj_cases' two ball
scenes that reach every limiter code, every timing status and every branch of the control stage, and the option sets."""
import numpy as np

import timing_ref
import traj_cases

F32 = np.float32
NS = (3, 4, 63, 64, 65, 128, 129, 255, 256)
TS = (1, 2, 63, 64, 65, 255, 256)

# every option off and on, and values that move each limiter into reach
OPT_SETS = (dict(), dict(v_min=0.5, v_max=0.8), dict(a_lat=0.0, w_max=0.0), dict(slow_dist=0.0), dict(a_lat=0.0), dict(w_max=0.0),
            dict(v_start=0.3, v_end=0.6, a_max=0.2, d_max=1.5), dict(a_lat=0.1, w_max=3.0), dict(w_max=0.2),
            dict(clearance=0.6, slow_dist=1.5), dict(v_start=2.0, v_end=2.0, v_max=0.7, v_min=0.7))


def opts(sc, **kw):
    """The reference's option dict: the defaults for the scene with kw replaced, as float32."""
    o = timing_ref.default_opts(len(sc["shape"]), sc["step"])
    o.update({k: F32(v) for k, v in kw.items()})
    return o


def _poly(cells, N):
    """N points on the polyline through `cells` [K, dim], uniform in the polyline's parameter (not in arc length)."""
    c = np.asarray(cells, np.float64)
    u = np.linspace(0.0, c.shape[0] - 1.0, N)
    k = np.minimum(u.astype(int), c.shape[0] - 2)
    w = (u - k)[:, None]
    return c[k] * (1 - w) + c[k + 1] * w


def _arc(centre, r, N, dim, rise):
    a = np.linspace(0.0, np.pi, N)
    p = np.zeros((N, dim))
    p[:, 0], p[:, 1] = centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)
    if dim == 3:
        p[:, 2] = centre[2] + rise * np.linspace(0.0, 1.0, N)
    return p


NAMES = ("free", "arc", "tight", "zigzag", "through", "leaves", "dups", "point", "reversal", "corner", "nan")


def curves(sc, N):
    """x [11, N, dim] f32 in NAMES' order: a free straight line (v_max, the end speeds and both cones), a half circle of radius
    1.2 (lateral acceleration), one of radius 0.3 (yaw rate), a zig-zag (the v_min floor with a raised v_min), a line through the
    first ball (clearance: inside the obstacle and in the band), a line that leaves the lattice (NaN samples: no limit), a line
    with a duplicated waypoint in the middle (N = 3: the last segment has length 0 and the first lies between two zero speeds:
    timing status 3), N copies of a point, an exact reversal along x (den = 0 in the yaw rate), a corner whose first leg is
    vertical in 3-D (steps that do not move horizontally before the first that does; 2-D: along y), a NaN trajectory (status 2)."""
    shape, dim, step = sc["shape"], len(sc["shape"]), sc["step"]
    hi = np.array(shape, np.float64) - 1
    ctr, rad = np.array(sc["bl"][0][0], np.float64), sc["bl"][0][1]
    e0, e1 = np.eye(dim)[0], np.eye(dim)[1]
    lo_c = np.ones(dim)
    free = _poly([lo_c, np.where(np.arange(dim) == 0, hi[0] - 1, 1.0)], N)
    c_arc = np.where(np.arange(dim) == 0, 8.0, np.where(np.arange(dim) == 1, 3.0, 2.0))
    arc = _arc(c_arc, 1.2 / step, N, dim, 3.0)
    tight = _arc(c_arc, 0.3 / step, N, dim, 1.0)
    zz = _poly([ctr - e0 * (rad + 3) + e1 * rad, ctr + e0 * (rad + 3) + e1 * rad], N)
    zz[1:-1:2, 1] += 3
    through = _poly([ctr - e0 * (rad + 4), ctr + e0 * (rad + 4)], N)
    leaves = _poly([hi - 3, hi + 4], N)
    dups = free.copy()
    dups[N // 2 + (N > 3)] = dups[N // 2 + (N > 3) - 1]
    point = np.repeat((lo_c * 2)[None], N, axis=0)
    rev = _poly([lo_c * 2, lo_c * 2 + e0 * 8, lo_c * 2], N)
    up = np.eye(dim)[dim - 1]
    corner = _poly([lo_c * 2, lo_c * 2 + up * 6, lo_c * 2 + up * 6 + e0 * 9], N)
    bad = free.copy()
    bad[N // 2, dim - 1] = np.nan
    cells = np.stack([free, arc, tight, zz, through, leaves, dups, point, rev, corner, bad])
    x = (np.array(sc["origin"], np.float64) + cells * step).astype(F32)
    return x


def knot_dts(t, status):
    """Step lengths that put tau_4 = 4 dt exactly on a knot t_i (a division by 4 is exact): t_i / 4 for waypoints a third and a
    half along the first four timed trajectories of positive duration.  t: the timing's own times, so that the knot is hit in
    the bits under test."""
    N = t.shape[1]
    rows = [r for r in range(t.shape[0]) if status[r] == 0 and t[r, N - 1] > 0][:4]
    return [float(t[r, i]) / 4.0 for r in rows for i in sorted({max(N // 3, 1), N // 2}) if t[r, i] > 0]


def status3():
    """(x [1, 3, 2], opts): x_1 = x_0 and both end speeds 0: the one positive segment has zero speed at both ends."""
    return np.array([[[0.5, 2.0], [0.5, 2.0], [1.5, 2.5]]], F32), dict(v_start=0.0, v_end=0.0)


def planner_input(sc, dist, N):
    """(x [m, N, dim], in_status [m]) of traj_cases' planner paths resampled by the reference: status-2 trajectories and a path of
    one point (N copies) among them."""
    import traj_ref
    _, _, _, off, pts, _, st = traj_cases.plan(sc, dist)
    return traj_ref.resample(off, pts, st, N)
