"""Inputs shared by tests/test_history_cases.py (CPU: every sequence reaches the branch it is there for, asserted on the
references alone) and tests/test_gpu_handle_history.py (the device: one long-lived handle per object through its sequence).
Per object a list of calls A, B, C, ..., A: B larger than A in every capacity the object keeps, C smaller than A and across the
object's degenerate branch, one call in the other dimension where the object serves both, and A again at the end.  Every field
is an analytic f grid (balls, free space) for from_grid, or one of the two analytic scenes of tests/test_track_ref.py on the
lattices of tests/test_track_field_ref.py; no map is needed.  The references take the dist grid as an argument: the CPU test
passes dfield_ref's, the device test the device's own."""
import math

import numpy as np

import cover_ref
import dfield_ref
import locate_ref
import mppi_cases as mc
import mppi_ref
import pf_ref
import render_field_ref
import track_field_ref
import track_ref
import traj_cases
import view_ref
from test_locate_ref import TH2, TRUE2, TRUE3, depth3, grid2, grid3, ranges2
from test_pf_ref import IDENT3, MOTION2, motion2, motion3
from test_track_field_ref import LAT2, LAT3
from test_track_ref import CAM, OFF2, pose6, pose12, rot

F32 = np.float32
F64 = np.float64

# ---- lattices and analytic fields ---------------------------------------------------------------------------------------------
SMALL2 = dict(shape=(60, 40), origin=(-0.6, -0.4), step=0.02)
SMALL3 = dict(shape=(24, 20, 16), origin=(-0.6, -0.5, 0.3), step=0.05)
TINY2 = dict(shape=(9, 7), origin=(-0.4, -0.3), step=0.1)
BIG2 = dict(shape=(150, 130), origin=(-1.5, -1.3), step=0.02)
MID2 = dict(shape=(33, 20), origin=(-0.34, -0.2), step=0.02)
TINY3 = dict(shape=(13, 11, 9), origin=(-0.3, -0.25, 0.3), step=0.05)
CAM13 = (10.0, 10.0, 6.0, 3.0, 13, 7)                    # 2 x 1 tiles of 8 x 8 pixels, both hanging over the image
TH90 = TH2[::4]
TH23 = TH2[::16]
GAP5 = math.radians(5.0)                                 # (TH90's beams are 4 degrees apart)
GAP17 = math.radians(17.0)                               # (TH23's are 16 apart)
FIELDS = {                                               # name -> (lattice, balls in lattice units; None: free space, no site)
    "small2": (SMALL2, [((40.0, 20.0), 6.0)]),
    "small3": (SMALL3, [((12.0, 10.0, 10.0), 3.0)]),
    "tiny2": (TINY2, None),
    "big2": (BIG2, [((100.0, 65.0), 14.0), ((40.0, 100.0), 9.0)]),
    "mid2": (MID2, [((24.0, 10.0), 3.5)]),
    "tiny3": (TINY3, [((7.0, 5.0, 6.0), 1.6)]),
}
_CACHE = {}


def lat(l):
    return l["shape"], l["origin"], l["step"]


def field(name):
    """dict(shape, origin, step, f): the analytic f grid (flat, x fastest) of a named field."""
    if ("f", name) not in _CACHE:
        l, bl = FIELDS[name]
        f = np.ones(int(np.prod(l["shape"])), F32) if bl is None else traj_cases.balls(l["shape"], l["step"], bl)
        f.setflags(write=False)
        _CACHE["f", name] = dict(l, f=f)
    return _CACHE["f", name]


def ref_field(name):
    """(dist, site) of dfield_ref on a named field, computed once."""
    if ("d", name) not in _CACHE:
        fd = field(name)
        _CACHE["d", name] = dfield_ref.distance_field(fd["f"], fd["shape"], fd["origin"], fd["step"], 0.0)
    return _CACHE["d", name]


def sample_points(l, m=300, seed=9):
    """Points for the sampler: random ones in and a little around the lattice, the lattice's last point (its last cell), its first,
    and points outside on every side."""
    dim = len(l["shape"])
    lo = np.array(l["origin"], F64)
    hi = lo + (np.array(l["shape"]) - 1) * l["step"]
    x = (lo + np.random.default_rng(seed).uniform(-0.05, 1.05, (m, dim)) * (hi - lo)).astype(F32)
    last = cover_ref.lattice_points([int(np.prod(l["shape"])) - 1], *lat(l))[0]
    inside_last = (last - F32(0.25 * l["step"])).astype(F32)
    return np.concatenate([x, last[None], inside_last[None], lo[None].astype(F32), (hi + 3 * l["step"])[None].astype(F32),
                           (lo - 3 * l["step"])[None].astype(F32)])


def masked(ranges, p, seed=11):
    """The scan with all but p beams (a fixed scattered subset, in order) made invalid."""
    keep = np.sort(np.random.default_rng(seed).permutation(ranges.size)[:p])
    out = np.zeros_like(ranges)
    out[keep] = ranges[keep]
    return out


# ---- Controller ---------------------------------------------------------------------------------------------------------------
CONTROLLER = ((2, 257, 33), (3, 1000, 33), (2, 64, 1), (2, 4097, 2), (2, 257, 33))      # (dim, K, T)
CONTROLLER_SEEDS = (5, 6, 7, 8, 5)                       # a new seed per init; the last entry is the first again
CONTROLLER_P = (2, 4, 1, 32, 2)
CONTROLLER_COLUMNS = (66, 132, 2, 4, 66)


def mppi_segments(K):
    """P of csrc/mppi.hip: the power of two at or above ceil(K / 256), the width of the update's tree."""
    P = 1
    while P < (K + 255) // 256:
        P *= 2
    return P


def controller_case(i):
    dim, K, T = CONTROLLER[i]
    return dict(mc.shape_case(K, T, dim), seed=CONTROLLER_SEEDS[i])


def controller_ref(i):
    """The two steps of entry i by the reference (its own weights): [step 1, step 2] as mppi_ref.step returns them."""
    c = controller_case(i)
    sc = mc.scene(c["dim"])
    cost, goal = mc.terminal_args(c)
    ctl = mppi_ref.Controller(c["dim"], c["K"], c["T"], c["seed"])
    ctl.set_nominal(mc.nominal_of(c))
    out = []
    for k in range(2):
        if k:
            ctl.shift()
        ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], c["opts"], cost, goal)
        out.append(ctl.last)
    return out


# ---- Controller with a set of moving balls and a footprint ----------------------------------------------------------------------
# (dim, K, T, balls, body balls): A; B larger in every capacity; C across P = 1 with one ball and one body ball; a plain step at
# the largest K, after which the rollout buffers (grown by init under cap_k) are longer than the per-rollout buffers of the balls
# (d_dyn, d_msep, d_bdyn: grown by step under cap_dyn); then balls under that K, which init has served and step has not; A again
CONTROLLER_BODY = ((2, 257, 33, 65, 5), (3, 1000, 33, 256, 16), (2, 64, 1, 1, 1), (2, 4097, 2, 0, 0), (2, 4097, 2, 2, 16), (2, 257, 33, 65, 5))
CONTROLLER_BODY_SEEDS = (5, 6, 7, 8, 9, 5)


def controller_body_case(i):
    """Entry i as a case of tests/body_cases.py (obst None without balls, body None without body balls).  Where the horizon is too
    short for the shape cases' crossing ball to arrive, ball 0 rests just ahead of the robot instead."""
    import body_cases as bc
    import obst_cases as oc
    import obst_ref
    dim, K, T, n, m = CONTROLLER_BODY[i]
    c = dict(mc.shape_case(K, T, dim), seed=CONTROLLER_BODY_SEEDS[i], t_now=oc.T_NOW, expect=())
    S = oc.balls(dim, n, mc.scene(dim)["step"]) if n else None
    if S is not None and T <= 2:
        ahead = mppi_ref.start_state(c["pose"], dim)[:dim] + np.array([0.1, 0.0, 0.0])[:dim]
        S = obst_ref.make(dim, np.concatenate([ahead[None], S["c"][1:]]), np.concatenate([np.zeros((1, dim)), S["v"][1:]]), S["r"], epoch=S["epoch"],
                          step=mc.scene(dim)["step"])
    return dict(c, obst=S, body=bc.footprint(dim, m) if m else None)


def controller_body_ref(i):
    """The two steps of entry i by the reference (its own weights), the clock moved on by dt between them: [step 1, step 2] as
    body_ref.step returns them."""
    import body_ref
    c = controller_body_case(i)
    sc = mc.scene(c["dim"])
    cost, goal = mc.terminal_args(c)
    ctl = body_ref.Controller(c["dim"], c["K"], c["T"], c["seed"])
    ctl.set_nominal(mc.nominal_of(c))
    out = []
    for k in range(2):
        if k:
            ctl.shift()
        ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], c["opts"], cost, goal, obst=c["obst"],
                 t_now=c["t_now"] + k * c["opts"]["dt"], body=c["body"])
        out.append(ctl.last)
    return out


# ---- ParticleFilter -----------------------------------------------------------------------------------------------------------
FILTER = ((2, 257), (2, 4097), (2, 1), (2, 65), (3, 300), (2, 257))      # (dim, particles)
FILTER_SEEDS = (1, 2, 3, 4, 5, 1)
FILTER_UPDATES = (dict(), dict(resample_below=0.0))      # the first collapses the set and resamples (m > 2), the second keeps L
MOTION3 = motion3((0.002, -0.001, 0.003), (1, 2, 3), 0.004)
STRIDE3 = 8


def filter_poses(i):
    dim, m = FILTER[i]
    return grid2()[:m] if dim == 2 else grid3()[(171 + 37 * np.arange(m)) % 1029]


def filter_motions(i):
    return (motion2(*MOTION2), motion2(*MOTION2)) if FILTER[i][0] == 2 else (IDENT3, MOTION3)


def filter_points(dim):
    """The frame every update of that dimension weighs against, as the tracker's local points."""
    if dim == 2:
        return track_ref.points2(TH2, ranges2(), OFF2)[0]
    return track_ref.points3(depth3(), CAM, STRIDE3)[0]


def filter_ref(i, dist):
    """Entry i by the reference (its own weights) on the dist grid of LAT2 / LAT3: [(resampled, Filter after the update)] of
    the two updates."""
    dim, m = FILTER[i]
    l = LAT2 if dim == 2 else LAT3
    loc = filter_points(dim)
    f = pf_ref.Filter(filter_poses(i), dim, FILTER_SEEDS[i])
    out = []
    for mo, kw in zip(filter_motions(i), FILTER_UPDATES):
        o = dict(pf_ref.default_opts(dim), **kw)
        f.predict(mo, o["sigma_t"], o["sigma_r"])
        f.update(dist, *lat(l), loc, o["max_residual"], o["beta"], o["resample_below"])
        out.append((bool(f.resampled), dict(state=f.state.copy(), L=f.L.copy(), q=f.q.copy(), cost=f.cost.copy(),
                                            inliers=f.inliers.copy(), ancestors=f.anc.copy())))
    return out


# ---- Coverage -----------------------------------------------------------------------------------------------------------------
def _cover_ranges2():
    th = TH2.astype(F64)
    r = (0.40 + 0.15 * np.cos(3.0 * th)).astype(F32)     # 0.25 .. 0.55: every beam valid
    r[20:60] = 0.0                                       # 40 invalid beams: a wedge stays unseen
    return r


def _cover_depth3():
    """A 13 x 7 frame (column-major, pixel (u, v) at u * 7 + v) of a wavy wall about 1.9 m away, three columns and the middle row invalid: the view
    falls into parts a few lattice cells apart, each with a frontier component of its own."""
    u, v = np.arange(13, dtype=F64)[:, None], np.arange(7, dtype=F64)[None, :]
    d = 1.9 + 0.05 * np.cos(1.3 * u) + 0.04 * np.sin(0.9 * v)
    d[[3, 6, 9], :] = 0.0
    d[:, 3] = 0.0
    return d.astype(F32).ravel()


COVERAGE = (
    dict(field="small2", thetas=TH2, ranges=_cover_ranges2(), pose=pose6(0.4, (-0.25, 0.05)), off2=(0.03, -0.02), opts={}),
    dict(field="small3", depth=_cover_depth3(), cam=CAM13, pose=pose12(np.eye(3), np.array([-0.3, -0.3, -1.2])), opts={}),
    # one valid beam of three, the sensor on a lattice point: fewer than two valid beams see nothing
    dict(field="tiny2", thetas=np.array([0.0, 0.02, 0.04], F32), ranges=np.array([0.5, 0.0, 0.0], F32), pose=pose6(0.3, (0.0, 0.0)),
         off2=(0.0, 0.0), opts=dict(back_off=0.01)),
)
COVERAGE = COVERAGE + (COVERAGE[0],)


def coverage_ref(e, dist):
    """One entry by the references on the entry's lattice: dict(seen, frontiers, restricted, samples)."""
    l = FIELDS[e["field"]][0]
    shape, origin, step = lat(l)
    o = dict(cover_ref.default_opts(len(shape), float(F32(step))), **e["opts"])
    none = np.zeros(int(np.prod(shape)), bool)
    if "depth" in e:
        seen = cover_ref.integrate_depth(none, shape, origin, step, e["depth"], e["cam"], e["pose"], o["back_off"])
    else:
        seen = cover_ref.integrate_scan(none, shape, origin, step, e["thetas"], e["ranges"], e["pose"], e["off2"], o["back_off"], o["max_gap"])
    fr = cover_ref.frontiers(seen, dist, shape, origin, step, o["clearance"], o["min_size"])
    rd = cover_ref.restrict(seen, dist, -float(F32(step)))
    return dict(seen=seen, frontiers=fr, restricted=rd, samples=dfield_ref.sample(rd, shape, origin, step, sample_points(l)))


# ---- ViewScorer ---------------------------------------------------------------------------------------------------------------
def poses2(m, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([pose6(rng.uniform(-3, 3), (rng.uniform(-0.5, 0.1), rng.uniform(-0.35, 0.35))) for _ in range(m)])


def poses3(m, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([pose12(rot(rng.normal(size=3), rng.uniform(0, 0.3)), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2),
                                                                                     rng.uniform(-0.35, -0.15)])) for _ in range(m)])


def half_seen(n, seed=3):
    return np.random.default_rng(seed).random(n) < 0.5


VIEW = (
    dict(field="small2", sensor=(TH90, (0.03, -0.02)), poses=poses2(65), seen=half_seen(60 * 40), opts=dict(max_gap=GAP5)),
    dict(field="small3", sensor=CAM13, poses=poses3(3), seen=half_seen(24 * 20 * 16), opts={}),
    dict(field="tiny2", sensor=(TH23, (0.0, 0.0)), poses=pose6(0.3, (0.0, 0.0))[None], seen=np.ones(9 * 7, bool), opts=dict(max_gap=GAP17)),
)
VIEW = VIEW + (VIEW[0],)


def view_ref_call(e, dist):
    """(gain, hits, predicted, targets, the march's samples of the first pose) of one entry by the references."""
    l = FIELDS[e["field"]][0]
    shape, origin, step = lat(l)
    if len(shape) == 3:
        g, h, p = view_ref.gain_depth(dist, e["seen"], shape, origin, step, e["sensor"], e["poses"], **e["opts"])
        stats = render_field_ref.render_depth(dist, shape, origin, step, e["sensor"], e["poses"][0])[3]
    else:
        g, h, p = view_ref.gain_scan(dist, e["seen"], shape, origin, step, e["sensor"][0], e["sensor"][1], e["poses"], **e["opts"])
        stats = render_field_ref.render_scan(dist, shape, origin, step, e["sensor"][0], e["poses"][0], e["sensor"][1])[3]
    return g, h, p, int(view_ref.targets(e["seen"], dist, -math.inf).sum()), int(stats["samples"])


# ---- Locator, Tracker, Renderer: the field paths on the analytic scenes (LAT2 / LAT3) -----------------------------------------
LOCATOR = (
    dict(dim=2, poses=grid2()[:300], ranges=masked(ranges2(), 270)),
    dict(dim=2, poses=grid2()[:5000], ranges=masked(ranges2(), 270)),
    dict(dim=3, poses=grid3()[[171, 0, 1028]], stride=8),
    dict(dim=2, poses=grid2()[187:188], ranges=masked(ranges2(), 37)),
)
LOCATOR = LOCATOR + (LOCATOR[0],)


def locator_ref(e, dist):
    if e["dim"] == 3:
        return locate_ref.score_depth(dist, *lat(LAT3), depth3(), CAM, e["poses"], stride=e["stride"])
    return locate_ref.score_scan(dist, *lat(LAT2), TH2, e["ranges"], e["poses"], OFF2)


START2 = pose6(0.15 + math.radians(2.0), (0.3 + 0.015, -0.2 - 0.013))
START3 = pose12(rot([0.4, -1, 0.7], math.radians(2.0)) @ np.asarray(TRUE3[3:], F64).reshape(3, 3).T,
                np.asarray(TRUE3[:3], F64) + np.array([0.0128, -0.0102, 0.0115]))
SEGMENT = 256                                            # csrc/track.h: points per partial sum
TRACKER = (
    dict(dim=3, pose0=START3, opts=dict(stride=2)),
    dict(dim=2, pose0=START2, ranges=masked(ranges2(), 270), opts={}),
    dict(dim=2, pose0=START2, ranges=masked(ranges2(), 37), opts={}),
)
TRACKER = TRACKER + (TRACKER[0],)


def tracker_ref(e, dist):
    if e["dim"] == 3:
        return track_field_ref.track_depth(dist, *lat(LAT3), depth3(), CAM, e["pose0"], **e["opts"])
    return track_field_ref.track_scan(dist, *lat(LAT2), TH2, e["ranges"], e["pose0"], OFF2, **e["opts"])


RENDERER = (
    dict(dim=3, cam=CAM, pose=TRUE3, tiles=True),
    dict(dim=3, cam=CAM13, pose=TRUE3, tiles=False),       # the other thread-to-pixel mapping, on an image no tile divides
    dict(dim=2, thetas=TH2, pose=TRUE2, tiles=True),
    dict(dim=2, thetas=TH23, pose=TRUE2, tiles=True),
)
RENDERER = RENDERER + (RENDERER[0],)


def renderer_ref(e, dist):
    """(depth, rec, status, stats) of render_field_ref."""
    if e["dim"] == 3:
        return render_field_ref.render_depth(dist, *lat(LAT3), e["cam"], e["pose"])
    return render_field_ref.render_scan(dist, *lat(LAT2), e["thetas"], e["pose"], OFF2)


# ---- DistanceField ------------------------------------------------------------------------------------------------------------
DFIELD = ("small2", "small3", "tiny2", "small2")         # 60 x 40 -> 24 x 20 x 16 -> 9 x 7 without a site -> 60 x 40


# ---- the session: every object's call once per round on one set of handles ----------------------------------------------------
SESSION2 = ("small2", "big2", "mid2")
SESSION3 = ("small3", "tiny3")
YAWS8 = np.arange(8) * (2.0 * math.pi / 8.0)


def session_pose(name):
    """The sensor pose of a round, in free space of the named field, looking along +x (2-D) / +z from below the lattice (3-D)."""
    l = FIELDS[name][0]
    o, s, n = np.array(l["origin"], F64), l["step"], np.array(l["shape"])
    if len(n) == 2:
        return pose6(0.3, tuple(o + 0.25 * (n - 1) * s))
    c = o + 0.5 * (n - 1) * s
    return pose12(np.eye(3), np.array([c[0] - 2 * s, c[1] + s, o[2] - 0.9]))


# what the session's later stages add: a footprint, limits and three balls in the scale of the round's lattice
SESSION_DT = 0.1
SESSION_T0 = 1.0


def _extent(name):
    l = FIELDS[name][0]
    return np.array(l["origin"], F64), (np.array(l["shape"]) - 1) * l["step"], l["step"]


def session_body(name):
    """The robot of a round: a box of five discs (2-D) / three balls turning about z (3-D), a few lattice steps long."""
    import body_ref
    o, ext, s = _extent(name)
    if len(o) == 2:
        return body_ref.box(6 * s, 2.5 * s, 5)
    return body_ref.make(3, [(1.2 * s, 0.0, 0.4 * s), (-s, 0.6 * s, -0.4 * s), (0.0, -s, 0.8 * s)], [0.8 * s, s, 0.6 * s])


def session_timing(name):
    """Speed and acceleration limits for a lattice about a metre across."""
    return dict(v_max=0.3, v_min=0.02, a_max=0.2, d_max=0.2, a_lat=0.2)


def session_balls(name):
    """Three balls: one that crosses just ahead of the round's pose within the controller's horizon, one that rests in a corner,
    one that drifts along the lattice's far side."""
    import obst_ref
    o, ext, s = _extent(name)
    dim = len(o)
    p = session_pose(name)[:dim].astype(F64)
    ahead = p + np.array([4 * s, 0.0, 0.0])[:dim] if dim == 2 else p + np.array([0.0, 0.0, 6 * s])
    v0 = np.zeros(dim)
    v0[1] = 2 * s
    drift = np.zeros(dim)
    drift[0] = -s
    c = np.stack([ahead - v0 * (SESSION_T0 + 1.0), o + 0.03 * ext, o + 0.9 * ext])
    return obst_ref.make(dim, c, np.stack([v0, np.zeros(dim), drift]), [2 * s, s, 1.5 * s], epoch=0.0, step=s)
