"""Inputs shared by tests/test_pplan_ref.py (CPU: the pose planner's reference against itself and its defective variants) and
tests/test_gpu_pplan.py (the device against the reference): the door scene of tests/body_cases.py, a Z-shaped corridor that is
wide enough for the robot's width and whose bends are too tight for its length, and small ball-and-wall scenes built as the
planner's tests build theirs.  Every scene is an analytic f grid; its dist comes from dfield_ref.distance_field on the host and
from DistanceField.from_grid on the device."""
import math

import numpy as np

import body_cases
import body_ref
import dfield_ref
import pplan_ref

F32 = np.float32
F64 = np.float64
ROBOT = body_cases.ROBOT
R_IN, R_OUT = body_cases.R_IN, body_cases.R_OUT
R_DISC = math.hypot(0.5 * ROBOT["width"], ROBOT["length"] / (2.0 * ROBOT["discs"]))     # the radius of one disc of the box
# (nx, ny, H, m) of the device tests: the smallest lattice, exactly one tile, one point past a tile edge in each axis, odd
# sizes over several tiles, the largest H
SHAPES = ((2, 2, 8, 1), (8, 8, 8, 2), (9, 8, 16, 16), (8, 9, 16, 3), (17, 23, 32, 3), (33, 20, 64, 5))
_cache = {}


def robot():
    return body_ref.box(ROBOT["length"], ROBOT["width"], ROBOT["discs"])


def _with_dist(sc):
    dist = dfield_ref.distance_field(sc["f"], sc["shape"], sc["origin"], sc["step"], 0.0)[0]
    dist.setflags(write=False)
    sc["dist"] = dist
    return sc


def door_scene():
    """body_cases.door_scene() with the pose planner's start and goal: (f, dist, shape, origin, step, start, goal)."""
    sc = body_cases.door_scene()
    return dict(f=sc["f"], dist=sc["dist"], shape=sc["shape"], origin=sc["origin"], step=sc["step"],
                start=np.array(sc["start"][:2], F32), goal=np.array(sc["goal_point"], F32))


def z_f():
    """The f grid of the Z corridor: 81 x 61, step 0.1, -1 on blocked lattice points and +1 elsewhere."""
    f = np.ones((61, 81), F32)
    f[0:46, 30:51] = -1.0
    f[20:26, 30:46] = 1.0
    f[6:26, 40:46] = 1.0
    f[6:12, 40:51] = 1.0
    return f.ravel()


def z_scene():
    """A block across the lower part of the lattice with a corridor 0.6 wide through it that bends twice at right angles; the
    bypass lies above y = 4.5.  middle: a point inside the corridor between the bends."""
    if "z" not in _cache:
        _cache["z"] = _with_dist(dict(f=z_f(), shape=(81, 61), origin=(0.0, 0.0), step=0.1, start=np.array([1.5, 2.3], F32),
                                      goal=np.array([6.5, 0.9], F32), middle=np.array([4.3, 1.6], F32)))
    return _cache["z"]


def lattice_index(sc, xy):
    i, j = (int(round((float(xy[a]) - sc["origin"][a]) / sc["step"])) for a in range(2))
    return j * sc["shape"][0] + i


def footprint(m):
    """m discs of a robot about 0.25 long and 0.1 wide (the small scenes are 0.7 across): ball 0 ahead of the reference point,
    the others scattered over the body, radii between 0.02 and 0.05.  m = 1: one disc just off the reference point."""
    rng = np.random.default_rng(500 + m)
    b = np.zeros((m, 2), F64)
    b[:, 0] = rng.uniform(-0.12, 0.12, m)
    b[:, 1] = rng.uniform(-0.05, 0.05, m)
    b[0] = (0.1, -0.03) if m > 1 else (0.03, -0.01)
    return body_ref.make(2, b, rng.uniform(0.02, 0.05, m))


def balls_f(shape, step, balls, walls=()):
    """f = distance to the union of balls (centre and radius in lattice units) and of walls (x0, x1, y0, y1 in lattice units,
    inclusive: -1 on their points), negative inside.  Flat float32, x fastest."""
    nx, ny = shape
    X, Y = np.meshgrid(np.arange(nx, dtype=F64), np.arange(ny, dtype=F64))
    f = np.full((ny, nx), 1e3)
    for (cx, cy), r in balls:
        f = np.minimum(f, np.sqrt((X - cx) ** 2 + (Y - cy) ** 2) - r)
    f = f * step
    for x0, x1, y0, y1 in walls:
        f[y0:y1 + 1, x0:x1 + 1] = -step
    return f.astype(F32).ravel()


def shape_scene(nx, ny):
    """A ball-and-wall scene on an nx x ny lattice of step 0.1 (origin off zero): one ball in the upper right part and, from 8
    points on, a short wall from the lower edge; on the 2 x 2 lattice the point (0, 0) alone is inside."""
    shape, origin, step = (nx, ny), (-0.3, 0.7), 0.1
    if min(nx, ny) <= 2:
        f = np.full(nx * ny, step, F32)
        f[0] = -step
    else:
        f = balls_f(shape, step, [((0.7 * nx, 0.65 * ny), 0.14 * min(nx, ny))], [(nx // 2, nx // 2, 0, ny // 3)])
    return _with_dist(dict(f=f, shape=shape, origin=origin, step=step))


def shape_goals(nx, ny, H):
    """Goals [g, 3] for shape_scene: a point near the lower left corner at every heading, one near the upper left corner at
    one heading, a duplicate of the first at heading 0, one outside the lattice."""
    o, s = (-0.3, 0.7), 0.1
    c = min(2, nx - 1, ny - 1)
    return np.array([(o[0] + c * s, o[1] + c * s, -1), (o[0] + c * s, o[1] + (ny - 1 - c) * s, H // 4), (o[0] + c * s, o[1] + c * s, 0),
                     (o[0] - 5 * s, o[1], -1)], F32)


def problem(sc, body, H, goals, moves="any", variant=None, dist=None, **opts):
    """pplan_ref.Problem of a scene (dist: the device's own grid in its place)."""
    return pplan_ref.Problem(sc["dist"] if dist is None else dist, sc["shape"], sc["origin"], sc["step"], body, pplan_ref.heading_table(H),
                             pplan_ref.heading_moves(H, moves) if isinstance(moves, str) else moves, goals, variant=variant, **opts)


def scene_problem(name, H=16, moves="any", variant=None, dist=None):
    """The door / Z problem of the issue's prototype: box(1.0, 0.4, 5), margin 0, turn 0.05, the goal at every heading."""
    sc = door_scene() if name == "door" else z_scene()
    g = np.array([[sc["goal"][0], sc["goal"][1], -1]], F32)
    return sc, problem(sc, robot(), H, g, moves, variant, dist, clearance=0.0, margin=0.0, turn=0.05)


def solved(name, H=16, moves="any"):
    """(scene, problem, cost, policy, projection) of a scene problem, computed once."""
    key = (name, H, moves)
    if key not in _cache:
        sc, pb = scene_problem(name, H, moves)
        cost = pplan_ref.solve_dijkstra(pb)
        cost.setflags(write=False)
        _cache[key] = (sc, pb, cost, pplan_ref.policy(pb, cost), pplan_ref.project(pb, cost))
    return _cache[key]


def start_cost(sc, pj):
    return float(pj["cost2"][lattice_index(sc, sc["start"])])


# ---- the closed loop on the Z corridor -----------------------------------------------------------------------------------------
LOOP = body_cases.LOOP


def point_cost(sc, clearance):
    """plan_ref's cost-to-go of a point with `clearance` towards the scene's goal (margin 0)."""
    import plan_ref
    pb = plan_ref.Problem(sc["dist"], sc["shape"], sc["origin"], sc["step"], [sc["goal"]], clearance=clearance, margin=0.0)
    return np.ascontiguousarray(plan_ref.solve_dijkstra(pb), F32).ravel()


def closed_loop(sc, cost, body, budget=None, step_fn=None, reach=0.3):
    """Drive body_cases.LOOP's controller (the reference, or step_fn(pose, o) -> u0, which steps and shifts, in its place)
    through `sc` from its start, heading along +x, with the terminal cost `cost` and the footprint `body`, field clearance 0.
    Returns dict(steps (None: the goal was not reached within the budget), states [n, 4], D (the body's clearance at every
    driven state), hits (the driven states with D < 0 or off the lattice))."""
    import mppi_ref
    o = mppi_ref.default_opts(2, sc["step"])
    o.update(LOOP["opts"], clearance=0.0)
    ctl = body_ref.Controller(2, LOOP["K"], LOOP["T"], LOOP["seed"])
    st = np.array([sc["start"][0], sc["start"][1], 1.0, 0.0], F64)
    goal = np.asarray(sc["goal"], F64)
    visited = [st.copy()]
    out = dict(steps=None)
    for n in range(LOOP["budget"] if budget is None else budget):
        pose = mppi_ref.pose_of_state(st, 2)
        if step_fn is None:
            u0, _ = ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], pose, o, cost=cost, body=body)
            ctl.shift()
        else:
            u0 = step_fn(pose, o)
        st = mppi_ref.advance(st, u0, 2, o["dt"])
        visited.append(st.copy())
        if float(np.linalg.norm(st[:2] - goal)) <= reach:
            out["steps"] = n + 1
            break
    S = np.array(visited)
    chk = body_ref.clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], body, S, 0.0)
    out.update(states=S, D=chk["D"], hits=chk["below"] + chk["off"])
    return out


# ---- a small scene that reaches every branch -----------------------------------------------------------------------------------
def slim():
    """A slim asymmetric body: three discs along x (0.56 long, 0.16 wide) and a small one on its left side."""
    return body_ref.make(2, [(-0.2, 0.0), (0.0, 0.0), (0.2, 0.0), (0.1, 0.12)], [0.08, 0.08, 0.08, 0.05])


def gap_scene():
    """26 x 22 points of step 0.1, origin off zero: a wall along y with a gap three points wide below the middle -- the slim
    body passes it lengthwise only -- and a ball in the upper right part.  goal: behind the wall at heading 0; start: in front
    of it."""
    if "gap" not in _cache:
        shape, origin, step = (26, 22), (0.5, -0.2), 0.1
        f = balls_f(shape, step, [((19.0, 15.0), 2.5)]).reshape(22, 26)
        f[:, 12] = -step
        f[8:11, 12] = step
        sc = dict(f=f.ravel(), shape=shape, origin=origin, step=step, start=np.array([origin[0] + 0.5, origin[1] + 1.5], F32),
                  goal=np.array([origin[0] + 2.0, origin[1] + 0.6], F32))
        _cache["gap"] = _with_dist(sc)
    return _cache["gap"]


GAP_OPTS = dict(clearance=0.0, margin=0.15, gain=4.0, turn=0.05)


def gap_problem(moves="forward", H=8, variant=None, dist=None, goal_h=0, in_gap=False, **opts):
    """The gap case: the goal (in_gap: the middle of the gap instead, where only the lengthwise headings are free) given twice
    with the heading goal_h, a goal outside the lattice and one inside the wall."""
    sc = gap_scene()
    gx, gy = (sc["origin"][0] + 1.2, sc["origin"][1] + 0.9) if in_gap else (sc["goal"][0], sc["goal"][1])
    g = np.array([[gx, gy, goal_h], [gx, gy, goal_h], [-9.0, 0.0, -1],
                  [sc["origin"][0] + 1.2, sc["origin"][1] + 0.3, -1]], F32)           # a duplicate, one outside, one inside the wall
    return sc, problem(sc, slim(), H, g, moves, variant, dist, **dict(GAP_OPTS, **opts))
