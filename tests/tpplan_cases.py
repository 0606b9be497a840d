"""Inputs shared by tests/test_tpplan_ref.py (CPU: the time-pose planner's reference against a Dijkstra on the explicit graph,
against the pose planner and the time planner, and against its defective variants) and tests/test_gpu_tpplan.py (the device
against the reference): the shape cases on pplan_cases.shape_scene, small scenes that force one branch each, and the
demonstration: a corridor with a disc parked on the route of the long narrow robot body_ref.box(1.0, 0.4, 5)."""
import functools

import numpy as np

import body_ref
import obst_ref
import pplan_cases
import pplan_ref
import tplan_cases
import tplan_ref
import tpplan_ref as tp

F32 = np.float32
F64 = np.float64

# name: (nx, ny, H, S, n, body balls, moves, m, (T, k0)).  The lattices: the smallest, a ragged edge in both axes, exactly one
# tile, a tile and a point / two tiles and a point, multiple ragged tiles; every H; S 1, 2, 7, 9, 17; the ball counts 0, 1, 2, 65
# (one word of the kept mask and one more), 256; 1, 4 and 16 body balls.  The pairings keep (states x balls x body balls x S)
# below about two million, so that the numpy reference stays within seconds per case.
SHAPES = {
    "a": (2, 2, 8, 1, 0, 1, "any", 1, (1, 0)),
    "b": (7, 9, 16, 7, 65, 4, "forward", 11, (64, 3)),
    "c": (8, 8, 8, 2, 256, 1, "any", 600, (1, 5)),
    "d": (9, 17, 32, 9, 2, 16, "any", 11, (256, 0)),
    "e": (20, 13, 64, 17, 1, 4, "forward", 600, (64, 40)),
    "f": (20, 13, 8, 2, 256, 1, "any", 11, (64, 0)),
}
LONG = (8, 8, 8, 1024)


def world(sc, cells):
    cells = np.asarray(cells, F64).reshape(-1, 2)
    return (np.array(sc["origin"], F64) + cells * sc["step"]).astype(F32)


def poses(xy, h=-1):
    """[g, 3] f32 rows (x, y, h) of the points xy [g, 2]."""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    return np.concatenate([xy, np.full((xy.shape[0], 1), h, F32)], axis=1)


def shape_goals(sc, H, S):
    """pplan_cases.shape_goals (every heading, one heading, a duplicate, one outside) and goals at every heading on a grid of
    spacing min(max(2, S // 2), 12) lattice points, so that a short horizon still serves a share of the free states."""
    nx, ny = sc["shape"]
    g = min(max(2, S // 2), 12)
    cells = [(i, j) for j in range(g // 2, ny, g) for i in range(g // 2, nx, g)]
    return np.concatenate([pplan_cases.shape_goals(nx, ny, H), poses(world(sc, cells))])


def shape_balls(sc, n, seed):
    """n small balls around and over the lattice: centres in a box about its middle that grows with n (about six balls per
    square metre), speeds up to 0.6 m/s, radii 0.01 .. 0.03, an epoch off zero; ball 0 stands still."""
    rng = np.random.default_rng(seed)
    nx, ny = sc["shape"]
    lo = np.array(sc["origin"], F64)
    ext = np.array([nx - 1, ny - 1], F64) * sc["step"]
    half = np.maximum(0.75 * ext, 0.2 * np.sqrt(max(n, 1)))
    c = (lo + 0.5 * ext) + half * rng.uniform(-1.0, 1.0, (n, 2))
    v = rng.uniform(-0.6, 0.6, (n, 2))
    if n:
        v[0] = 0.0
    return obst_ref.make(2, c, v, rng.uniform(0.01, 0.03, n), epoch=0.75, step=sc["step"])


def shape_starts(sc, H, m, goals, seed):
    """m starts [m, 3]: a goal at heading -1 (arrive 0), a point outside, a NaN, then points spread over a box slightly larger
    than the lattice, the heading -1 for one in three and an index otherwise."""
    rng = np.random.default_rng(seed)
    nx, ny = sc["shape"]
    lo = np.array(sc["origin"], F64)
    ext = np.array([nx - 1, ny - 1], F64) * sc["step"]
    x = np.zeros((m, 3), F32)
    x[:, :2] = lo + ext * rng.uniform(-0.05, 1.05, (m, 2))
    x[:, 2] = rng.integers(0, H, m)
    x[::3, 2] = -1
    x[0] = goals[0]
    if m > 2:
        x[1, :2] = (lo[0] - 1.0, lo[1])
        x[2, :2] = (np.nan, lo[1])
    return x


@functools.lru_cache(maxsize=None)
def shape_case(name):
    nx, ny, H, S, n, mb, moves, m, (T, k0) = SHAPES[name]
    sc = pplan_cases.shape_scene(nx, ny)
    goals = shape_goals(sc, H, S)
    opts = dict(tp.default_opts(sc["step"], H), horizon=S, slot=0.2, dyn_clearance=0.02, keep_cost=1, margin=0.1, gain=1.0, turn=0.05)
    return dict(name=name, sc=sc, H=H, moves=moves, body=pplan_cases.footprint(mb), goals=goals, obst=shape_balls(sc, n, 100 + nx + S),
                t_begin=1.25, opts=opts, starts=shape_starts(sc, H, m, goals, 7 + nx), T=T, k0=k0)


@functools.lru_cache(maxsize=None)
def long_case():
    nx, ny, H, S = LONG
    sc = pplan_cases.shape_scene(nx, ny)
    opts = dict(tp.default_opts(sc["step"], H), horizon=S, slot=0.05, dyn_clearance=0.05, keep_cost=1, turn=0.05)
    ob = obst_ref.make(2, [[sc["origin"][0] - 20.0, sc["origin"][1] + 0.35]], [[0.5, 0.0]], [0.1], epoch=0.0, step=sc["step"])
    st = np.concatenate([poses(world(sc, [(2, 6), (1, 1)])), poses(world(sc, [(6, 1)]), 3)])
    return dict(name="long", sc=sc, H=H, moves="any", body=pplan_cases.footprint(1), goals=poses(world(sc, [(1, 1)])), obst=ob, t_begin=0.0,
                opts=opts, starts=st, T=256, k0=1000)


def ref_solve(c, dist=None, variant=None, trace=None, body=None, obst="case"):
    sc = c["sc"]
    return tp.solve(sc["dist"] if dist is None else dist, sc["shape"], sc["origin"], sc["step"], c["body"] if body is None else body,
                    pplan_ref.heading_table(c["H"]), pplan_ref.heading_moves(c["H"], c["moves"]), c["goals"],
                    c["obst"] if isinstance(obst, str) else obst, c["t_begin"], c["opts"], variant, trace)


# ---- small scenes that force one branch each ----------------------------------------------------------------------------------------
NOSE = dict(off=[(0.0, 0.0), (-0.2, 0.0)], rho=[0.02, 0.02])      # the reference point's ball and a rear ball 0.2 behind it
NO_BALLS = obst_ref.make(2, np.zeros((0, 2)), np.zeros((0, 2)), [], step=0.1)


def small_case(name):
    """A room of 13 x 11 points whose lowest and highest rows are wall (dist = -1 there and +1 elsewhere on the CPU; the device
    computes its own distance field from the same grid), H = 8, the body NOSE, the goal at (10, 5) at every heading and the start
    at (3, 5) heading along +x, unless the name says otherwise."""
    sc = tplan_cases.open_scene(13, 11, blocked=[(i, j) for i in range(13) for j in (0, 10)])
    opts = dict(tp.default_opts(sc["step"], 8), margin=0.0, horizon=20, slot=0.2, dyn_clearance=0.03, turn=0.05, keep_cost=1)
    c = dict(name=name, sc=sc, H=8, moves="any", body=body_ref.make(2, NOSE["off"], NOSE["rho"]), goals=poses(world(sc, [(10, 5)])),
             obst=NO_BALLS, t_begin=0.0, opts=opts, starts=poses(world(sc, [(3, 5)]), 0), T=8, k0=0)
    one = lambda ctr, vel, r: obst_ref.make(2, [ctr], [vel], [r], step=sc["step"])
    y = 0.5                      # the row of the start and the goal
    if name == "cross":          # a ball crosses the row ahead of the robot and is gone; forward moves only: wait, then go
        c["moves"] = "forward"
        c["obst"] = one([0.6, y - 0.5], [0.0, 0.5], 0.1)
    elif name == "tunnel":       # a fast small ball passes through the row between two samples of the robot's third move
        c["moves"] = "forward"
        c["obst"] = one([0.55, y - 8.0 * 0.5], [0.0, 8.0], 0.01)
    elif name == "rear":         # a small ball parked just beside the row: it clears the reference point's ball at every heading
        c["moves"] = "forward"   # along the row and the point itself, and is swept by the rear ball of a robot that turned
        c["obst"] = one([0.5, y + 0.06], [0.0, 0.0], 0.005)
        c["starts"] = poses(world(sc, [(3, 5)]), 1)
    elif name == "turn":         # forward moves only, a start that faces -x: it must turn on the spot.  A small ball is parked on
        c["moves"] = "forward"   # the middle of the chord the rear ball's centre takes from heading 7 to heading 0: the poses
        c["starts"] = poses(world(sc, [(5, 5)]), 4)    # held at both ends clear it, the turn between them does not
        rad = 0.2 * np.cos(np.pi / 8.0)
        c["obst"] = one([0.5 + rad * np.cos(np.pi * 0.875), y + rad * np.sin(np.pi * 0.875)], [0.0, 0.0], 0.005)
        c["body"] = body_ref.make(2, [(0.0, 0.0), (-0.2, 0.0)], [0.02, 0.001])
        c["opts"]["dyn_clearance"] = 0.005
    elif name == "side":         # a ball parked ahead on the row closes the translation at heading 0; sideways moves are not
        c["moves"] = "forward"   # allowed, so the robot turns and goes round
        c["obst"] = one([0.6, y], [0.0, 0.0], 0.05)
    elif name == "on_start":     # a ball rests over the start: no move out of it is clear
        c["obst"] = one([0.3, y], [0.0, 0.0], 0.05)
    elif name == "short":        # the horizon cannot serve the start
        c["opts"]["horizon"] = 5
    elif name == "nan":          # a ball whose place overflows: inf - inf in its displacement, a NaN separation
        c["obst"] = obst_ref.make(2, [[0.5, y]], [[1e308, 0.0]], [0.05], step=sc["step"], epoch=-1e3)
    elif name == "any_heading":
        c["starts"] = poses(world(sc, [(3, 5)]))
    else:
        assert name == "plain", name
    return c


SMALL = ("plain", "cross", "tunnel", "rear", "turn", "side", "on_start", "short", "nan", "any_heading")


# ---- the demonstration: a disc parked on the long robot's route ---------------------------------------------------------------------
BOX = (1.0, 0.4, 5)
R_IN, R_OUT = pplan_cases.R_IN, pplan_cases.R_OUT
DEMO = dict(shape=(36, 20), step=0.1, start=(0.8, 1.0), goal=(2.8, 1.0), disc=((1.8, 1.0), 0.15), dyn_clearance=0.05, slot=0.2, horizon=48, H=16)


@functools.lru_cache(maxsize=None)
def demo_scene():
    """A corridor along x, 36 x 20 points of step 0.1, walled along its lower and upper edge (pplan_cases.balls_f's walls, the
    distance field the reference computes from them, as the device does)."""
    shape, step = DEMO["shape"], DEMO["step"]
    nx, ny = shape
    f = pplan_cases.balls_f(shape, step, [], [(0, nx - 1, 0, 1), (0, nx - 1, ny - 2, ny - 1)])
    return pplan_cases._with_dist(dict(f=f, shape=shape, origin=(0.0, 0.0), step=step))


def demo_obst():
    (cx, cy), r = DEMO["disc"]
    return obst_ref.make(2, [[cx, cy]], [[0.0, 0.0]], [r], step=DEMO["step"])


def demo_case():
    """The time-pose problem: box(1.0, 0.4, 5) from the start, facing +x, to the goal at every heading."""
    sc = demo_scene()
    opts = dict(tp.default_opts(sc["step"], DEMO["H"]), margin=0.0, turn=0.05, slot=DEMO["slot"], horizon=DEMO["horizon"],
                dyn_clearance=DEMO["dyn_clearance"])
    return dict(name="demo", sc=sc, H=DEMO["H"], moves="any", body=body_ref.box(*BOX), goals=poses([DEMO["goal"]]), obst=demo_obst(), t_begin=0.0,
                opts=opts, starts=poses([DEMO["start"]], 0), T=48, k0=0)


def demo_point(radius):
    """(solution, paths) of the point time planner (tplan_ref) for a disc robot of the given radius: the static clearance and the
    dyn_clearance both raised by it."""
    sc = demo_scene()
    o = dict(tplan_ref.default_opts(sc["step"]), clearance=radius, margin=0.0, slot=DEMO["slot"], horizon=DEMO["horizon"],
             dyn_clearance=DEMO["dyn_clearance"] + radius)
    sol = tplan_ref.solve(sc["dist"], sc["shape"], sc["origin"], sc["step"], np.array([DEMO["goal"]], F32), demo_obst(), 0.0, o)
    return sol, tplan_ref.paths(sol, np.array([DEMO["start"]], F32))


def point_route_as_poses(pa, H):
    """The point route pa (tplan_ref.paths) as a pose route for tpplan_ref.check: the robot faces where it goes (the heading
    index of each move's direction, kept while it waits; the first move's before it)."""
    cells = pa["cells"][0]
    hd, cur = [], None
    for a, b in zip(cells[:-1], cells[1:]):
        d = (int(b[0] - a[0]), int(b[1] - a[1]))
        if d != (0, 0):
            cur = pplan_ref.ANGLE8[9 + (d[1] + 1) * 3 + (d[0] + 1)] * H // 8
        hd.append(cur)
    first = next((h for h in hd if h is not None), 0)
    hd = [first if h is None else h for h in hd]
    hd = np.array(hd + [hd[-1] if hd else first], np.int32)
    return dict(pa, heading=hd)
