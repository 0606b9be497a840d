"""Inputs shared by tests/test_tplan_ref.py (CPU: the time planner's reference against a Dijkstra on the explicit graph, against
the static planner, and against its defective variants) and tests/test_gpu_tplan.py (the device against the reference): the
shape cases on pplan_cases.shape_scene, small special scenes that force one branch each, and the two scenes on
pplan_cases.z_scene (a parked disc on the corridor, a disc that crosses it)."""
import functools

import numpy as np

import obst_ref
import pplan_cases
import tplan_ref as tr

F32 = np.float32
F64 = np.float64

# name: (nx, ny, S, n, connectivity, m, (T, k0)).  The lattices: the smallest, one point short of / exactly / one point past a
# tile in each axis, several tiles of odd sizes; S: 1, 2, 7, 8, 9, 17, 64 against the layers per launch 1, 2, 8, 16; the ball
# counts 0, 1, 2, 65, 256 (one word of the kept mask, one more, all four); the numpy reference stays within seconds
SHAPES = {
    "a": (2, 2, 1, 0, 1, 1, (1, 0)),
    "b": (31, 33, 7, 1, 0, 11, (64, 3)),
    "c": (32, 32, 8, 2, 1, 11, (256, 0)),
    "d": (33, 65, 2, 256, 1, 600, (1, 5)),
    "e": (70, 45, 17, 65, 1, 11, (64, 40)),
    "f": (70, 45, 64, 2, 1, 600, (64, 0)),
    "g": (31, 33, 9, 0, 1, 11, (256, 7)),
}
SCHEDULES = tuple((L, cull) for L in (1, 2, 8, 16) for cull in (0, 1))
LONG = (8, 8, 1024)


def world(sc, cells):
    cells = np.asarray(cells, F64).reshape(-1, 2)
    return (np.array(sc["origin"], F64) + cells * sc["step"]).astype(F32)


def shape_goals(sc, S):
    """Goals on a grid of spacing g = min(max(2, S // 2), 12) lattice points (so that a short horizon still serves a share of
    the free points), one of them twice, one outside the lattice, and the lattice's first point (not free in the smallest)."""
    nx, ny = sc["shape"]
    g = min(max(2, S // 2), 12)
    cells = [(i, j) for j in range(g // 2, ny, g) for i in range(g // 2, nx, g)]
    cells += [cells[0], (-4, 1), (0, 0)]
    return world(sc, cells)


def shape_balls(sc, n, seed):
    """n balls around and over the lattice: centres in a box 1.5 times the lattice's about its middle, speeds up to 0.6 m/s,
    radii 0.05 .. 0.3, an epoch off zero."""
    rng = np.random.default_rng(seed)
    nx, ny = sc["shape"]
    lo = np.array(sc["origin"], F64)
    ext = np.array([nx - 1, ny - 1], F64) * sc["step"]
    c = lo + ext * rng.uniform(-0.25, 1.25, (n, 2))
    v = rng.uniform(-0.6, 0.6, (n, 2))
    if n:
        v[0] = 0.0                                       # one ball stands still
    r = rng.uniform(0.05, 0.3, n)
    return obst_ref.make(2, c, v, r, epoch=0.75, step=sc["step"])


def shape_starts(sc, m, goals, seed):
    """m starts: a goal (arrive 0), a point outside, a NaN, then points spread over a box slightly larger than the lattice."""
    rng = np.random.default_rng(seed)
    nx, ny = sc["shape"]
    lo = np.array(sc["origin"], F64)
    ext = np.array([nx - 1, ny - 1], F64) * sc["step"]
    x = (lo + ext * rng.uniform(-0.05, 1.05, (m, 2))).astype(F32)
    x[0] = goals[0]
    if m > 2:
        x[1] = (lo[0] - 1.0, lo[1])
        x[2] = (np.nan, lo[1])
    return x


@functools.lru_cache(maxsize=None)
def shape_case(name):
    nx, ny, S, n, conn, m, (T, k0) = SHAPES[name]
    sc = pplan_cases.shape_scene(nx, ny)
    goals = shape_goals(sc, S)
    opts = dict(tr.default_opts(sc["step"]), horizon=S, connectivity=conn, slot=0.2, dyn_clearance=0.15, keep_cost=1,
                margin=0.2, gain=1.0)
    return dict(name=name, sc=sc, goals=goals, obst=shape_balls(sc, n, 100 + nx + S), t_begin=1.25, opts=opts,
                starts=shape_starts(sc, m, goals, 7 + nx), T=T, k0=k0)


@functools.lru_cache(maxsize=None)
def long_case():
    nx, ny, S = LONG
    sc = pplan_cases.shape_scene(nx, ny)
    opts = dict(tr.default_opts(sc["step"]), horizon=S, slot=0.05, dyn_clearance=0.1, keep_cost=1)
    ob = obst_ref.make(2, [[sc["origin"][0] - 20.0, sc["origin"][1] + 0.35]], [[0.5, 0.0]], [0.2], epoch=0.0, step=sc["step"])
    return dict(name="long", sc=sc, goals=world(sc, [(1, 1)]), obst=ob, t_begin=0.0, opts=opts, starts=world(sc, [(2, 6), (1, 1), (7, 0)]),
                T=256, k0=1000)


def ref_solve(c, dist=None, variant=None, trace=None):
    sc = c["sc"]
    return tr.solve(sc["dist"] if dist is None else dist, sc["shape"], sc["origin"], sc["step"], c["goals"], c["obst"], c["t_begin"],
                    c["opts"], variant, trace)


# ---- the Z corridor --------------------------------------------------------------------------------------------------------------
Z_OPTS = dict(clearance=0.1, margin=0.2, gain=1.0, connectivity=1, slot=0.2, horizon=128, dyn_clearance=0.2, wait=0.5, keep_cost=0)


def z_case(kind, speed=0.3, at=None):
    """The Z corridor with no ball ("static"), a disc of radius 0.25 parked at `at` (default: the scene's middle) ("parked"), or
    a disc of radius 0.3 that crosses the route at `at` at `speed` along +y, over it at slot 30 ("crossing")."""
    sc = pplan_cases.z_scene()
    at = np.asarray(sc["middle"] if at is None else at, F64)
    if kind == "static":
        ob = obst_ref.make(2, np.zeros((0, 2)), np.zeros((0, 2)), [], step=sc["step"])
    elif kind == "parked":
        ob = obst_ref.make(2, [at], [[0.0, 0.0]], [0.25], step=sc["step"])
    else:
        t_over = 30 * Z_OPTS["slot"]
        ob = obst_ref.make(2, [at - np.array([0.0, speed * t_over])], [[0.0, speed]], [0.3], step=sc["step"])
    return dict(name="z_" + kind, sc=sc, goals=sc["goal"].reshape(1, 2), obst=ob, t_begin=0.0, opts=dict(Z_OPTS),
                starts=sc["start"].reshape(1, 2), T=64, k0=0)


# ---- small scenes that force one branch each ----------------------------------------------------------------------------------------
def open_scene(nx, ny, step=0.1, origin=(0.0, 0.0), blocked=()):
    """Free space with the given lattice points blocked; dist = +1 on free points and -1 on blocked ones (the planner reads the
    sign against its clearance 0 alone here: margin 0)."""
    d = np.ones((ny, nx), F32)
    for i, j in blocked:
        d[j, i] = -1.0
    return dict(shape=(nx, ny), origin=origin, step=step, dist=d.ravel(), f=d.ravel())


def small_case(name):
    """A corridor one point wide (9 x 1 ... as a 9 x 3 lattice with the outer rows blocked), the goal at its right end."""
    wall = [(i, j) for i in range(9) for j in (0, 2)]
    sc = open_scene(9, 3, blocked=wall)
    opts = dict(tr.default_opts(sc["step"]), margin=0.0, horizon=24, slot=0.2, dyn_clearance=0.1)
    goal, start = world(sc, [(8, 1)]), world(sc, [(0, 1)])
    none = obst_ref.make(2, np.zeros((0, 2)), np.zeros((0, 2)), [], step=sc["step"])
    c = dict(name=name, sc=sc, goals=goal, obst=none, t_begin=0.0, opts=opts, starts=start, T=8, k0=0)
    if name == "cross":          # a ball crosses the corridor ahead of the robot and is gone: wait, then go
        c["obst"] = obst_ref.make(2, [[0.4, 0.1 - 0.5]], [[0.0, 0.5]], [0.15], step=sc["step"])
    elif name == "tunnel":       # a fast small ball passes between two samples of the robot's third move
        c["obst"] = obst_ref.make(2, [[0.25, 0.1 - 8.0 * 0.5]], [[0.0, 8.0]], [0.02], step=sc["step"])
        c["opts"]["dyn_clearance"] = 0.02
    elif name == "on_start":     # a ball rests over the start: no move out of it is clear
        c["obst"] = obst_ref.make(2, [[0.0, 0.1]], [[0.0, 0.0]], [0.05], step=sc["step"])
    elif name == "short":        # the horizon cannot serve the start
        c["opts"]["horizon"] = 5
    elif name == "goal_blocked": # the goal is not free
        c["goals"] = world(sc, [(8, 0)])
    elif name == "nan":          # a ball whose place overflows: inf - inf in its displacement, a NaN separation
        c["obst"] = obst_ref.make(2, [[0.3, 0.1]], [[1e308, 0.0]], [0.05], step=sc["step"], epoch=-1e3)
    elif name == "at_goal":
        c["starts"] = goal
    else:
        assert name == "plain", name
    return c


SMALL = ("plain", "cross", "tunnel", "on_start", "short", "goal_blocked", "nan", "at_goal")
