"""Inputs shared by tests/test_body_ref.py (CPU: the reference against its defective variants) and tests/test_gpu_body.py (the
device against the reference): footprints on the scenes and cases of tests/mppi_cases.py, tests/obst_cases.py and
tests/traj_cases.py.  A case is an obst case (`obst` may be None) with `body` (a footprint of body_ref.make) and `expect` (branch
counters of body_ref.rollouts that must be > 0 in the first step) added."""
import math

import numpy as np

import body_ref
import mppi_cases as mc
import mppi_ref
import obst_cases as oc

F32 = np.float32
F64 = np.float64
# (K, T, m, n): the last workgroup of the rollouts, both ends of m, moving balls on and off
SHAPES = ((1, 1, 1, 0), (63, 2, 2, 0), (64, 33, 15, 0), (65, 33, 16, 1), (257, 2, 16, 65), (1000, 33, 3, 0), (1000, 33, 3, 2))
SHAPES3 = ((64, 33, 1, 0), (64, 33, 16, 1), (257, 2, 5, 65))
CLEAR_NS = (1, 63, 64, 65, 257, 1000)
CLEAR_MS = (1, 2, 16)
TRAJ_SHAPES = ((1, 3), (3, 4), (40, 63), (40, 64), (40, 65), (5, 256))


def footprint(dim, m):
    """m balls of a robot about 1.2 long: ball 0 ahead of the reference point, the others scattered over the body with offsets
    on both sides of every axis (3-D: a non-zero b2 in every ball) and radii between 0.05 and 0.3."""
    rng = np.random.default_rng(1000 * dim + m)
    b = np.zeros((m, dim), F64)
    b[:, 0] = rng.uniform(-0.6, 0.6, m)
    b[:, 1] = rng.uniform(-0.25, 0.25, m)
    if dim == 3:
        b[:, 2] = rng.uniform(0.1, 0.3, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    rho = rng.uniform(0.05, 0.3, m)
    b[0, 0], b[0, 1] = 0.45, -0.125
    return body_ref.make(dim, b, rho)


def with_body(c, body, expect=(), obst=None, t_now=oc.T_NOW):
    return dict(c, body=body, obst=obst, t_now=t_now, expect=tuple(expect))


def shape_case(K, T, m, n, dim=2):
    step = 0.2 if dim == 3 else 0.25
    return with_body(mc.shape_case(K, T, dim), footprint(dim, m), obst=oc.balls(dim, n, step) if n else None)


def branch_cases():
    """name -> case, each with the branch counters it must reach."""
    b = mc.branch_cases()
    into = b["into_ball"]
    two = body_ref.make(2, [(0.0, 0.0), (-1.0, 0.0)], [0.2, 0.2])                 # a front and a rear disc
    # a ball that crosses the robot's line where its rear disc is 2 s ahead (the reference point is 1 m further by then)
    rear_ball = oc._set2([(0.7, 8.0)], [(0.0, -1.0)], [0.2])
    return {
        "wide": with_body(into, footprint(2, 5), ("col", "band", "free", "second_ball_nearer")),
        "half_off": with_body(b["off_lattice"], body_ref.make(2, [(-0.4, 0.1), (0.8, 0.0)], [0.2, 0.1]), ("off", "free")),
        "tie": with_body(into, body_ref.make(2, [(0.3, 0.1), (0.3, 0.1), (-0.2, 0.0)], [0.15, 0.15, 0.1]), ("tie", "col")),
        "margin0": with_body(b["margin0"], footprint(2, 3), ("col", "free")),
        "crossing": with_body(into, footprint(2, 4), ("dyn_col", "dyn_band", "dyn_free", "dyn_rear"), obst=oc.branch_cases()["crossing"]["obst"]),
        "rear_hit": with_body(into, two, ("dyn_col", "dyn_rear"), obst=rear_ball),
        "off_ball": with_body(b["off_lattice"], body_ref.make(2, [(0.8, 0.0), (-0.4, 0.1)], [0.1, 0.2]), ("off", "dyn_off", "dyn_col"),
                              obst=oc.branch_cases()["off_lattice"]["obst"]),
        "sphere3": with_body(b["into_ball3"], body_ref.make(3, [(0.15, 0.0, 0.1), (-0.15, 0.05, -0.1), (0.0, -0.1, 0.05)], [0.05, 0.08, 0.03]),
                             ("col", "band", "free", "dyn_col", "dyn_band"),
                             obst=oc.branch_cases()["sphere3"]["obst"]),
        "leaves3": with_body(b["leaves3"], footprint(3, 2), ("off",)),
    }


def ref_step(c, Ubar, tick, variant=None, body="case"):
    sc = mc.scene(c["dim"])
    cost, goal = mc.terminal_args(c)
    return body_ref.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], Ubar, c["seed"], tick, c["K"], c["opts"], cost, goal,
                         variant, c["obst"], c["t_now"], c["body"] if isinstance(body, str) else body)


# ---- batches of states ------------------------------------------------------------------------------------------------------
def states(dim, n, seed=7):
    """n states over the scene and a little beyond its lattice, with unit headings; the first is fixed (it is the one the tests
    move through the batch)."""
    sc = mc.scene(dim)
    rng = np.random.default_rng(seed + 10 * dim)
    lo = np.array(sc["origin"], F64) - 0.3
    hi = np.array(sc["origin"], F64) + (np.array(sc["shape"], F64) - 1) * sc["step"] + 0.3
    S = np.zeros((n, dim + 2), F64)
    S[:, :dim] = lo + (hi - lo) * rng.random((n, dim))
    th = rng.uniform(-math.pi, math.pi, n)
    S[:, dim], S[:, dim + 1] = np.cos(th), np.sin(th)
    S[0, :dim] = (np.array(sc["origin"], F64) + 0.4 * (hi - lo))
    nn = np.sqrt(S[:, dim] * S[:, dim] + S[:, dim + 1] * S[:, dim + 1])
    S[:, dim], S[:, dim + 1] = S[:, dim] / nn, S[:, dim + 1] / nn
    return S


def ref_clearance(dim, body, S, clearance=0.0, variant=None, br=None):
    sc = mc.scene(dim)
    return body_ref.clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], body, S, clearance, variant, br)


# ---- trajectories -----------------------------------------------------------------------------------------------------------
def traj_body(dim):
    """An asymmetric body: a long nose, a short tail and a side ball, so that every heading shows."""
    if dim == 2:
        return body_ref.make(2, [(0.5, 0.0), (-0.25, 0.0), (0.0, 0.3)], [0.1, 0.15, 0.05])
    return body_ref.make(3, [(0.5, 0.0, 0.1), (-0.25, 0.0, -0.1), (0.0, 0.3, 0.2)], [0.1, 0.15, 0.05])


def repeated_waypoints():
    """(x [5, 6, 2] f32, names): a diagonal line with a zero chord at the start, in the middle, at the end, all points equal, and
    the plain line (whose last chord is not along x: it tells the "last_x" variant apart)."""
    p = np.array([(1.0 + 0.5 * i, 3.0 + 0.25 * i) for i in range(6)], F32)
    start, mid, end, same = p.copy(), p.copy(), p.copy(), p.copy()
    start[1] = start[0]
    mid[3] = mid[2]
    end[5] = end[4] = end[3]
    same[:] = same[0]
    return np.stack([start, mid, end, same, p]), ("start", "middle", "end", "all_equal", "line")


def leaving_waypoints(N=8):
    """(x [2, N, 2] f32): a line that leaves the lattice half way, and one wholly outside it."""
    import traj_cases
    sc = mc.scene(2)
    hi = np.array(sc["shape"]) - 1
    leaves = traj_cases._line(traj_cases.world(sc, hi - 6), traj_cases.world(sc, hi + 6), N)
    outside = traj_cases._line(traj_cases.world(sc, hi + 8), traj_cases.world(sc, hi + 12), N)
    return np.stack([leaves, outside]).astype(F32)


def ref_traj(dim, body, x, status, clearance=0.0, variant=None, trace=None):
    sc = mc.scene(dim)
    return body_ref.traj_clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], body, x, status, clearance, variant, trace)


# ---- the closed loop: a door wider than the robot and shorter than it is long --------------------------------------------------
ROBOT = dict(length=1.0, width=0.4, discs=5)
R_IN = 0.5 * ROBOT["width"]                                       # the inscribed radius
R_OUT = math.hypot(0.5 * ROBOT["length"], 0.5 * ROBOT["width"])   # the circumscribed radius
_door = {}
HALF_WALL, HALF_DOOR = 0.1, 0.35


def door_scene():
    """A 2-D lattice (step 0.1) with a wall along y (0.2 thick, at x = 4) that has a door 0.7 wide at y = 3: wider than the
    robot's 0.4, narrower than its length 1.0 and than twice its circumscribed radius.  f is the exact distance to the wall
    (negative inside) and dist the distance field the reference computes from it, as the device does; the goal lies behind the door and below it, the start in front of it
    and above, so that the shortest route crosses the door at a slant.  cost is the planner reference's cost-to-go for a point with PLAN's clearance (the inscribed radius): the
    route through the door, which all three robots are offered."""
    if not _door:
        shape, origin, step = (81, 61), (0.0, 0.0), 0.1
        X, Y = np.meshgrid(np.arange(shape[0]) * step, np.arange(shape[1]) * step)

        def box_sdf(cx, cy, hx, hy):
            qx, qy = np.abs(X - cx) - hx, np.abs(Y - cy) - hy
            return np.sqrt(np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2) + np.minimum(np.maximum(qx, qy), 0)

        lower = box_sdf(4.0, (3.0 - HALF_DOOR) - 5.0, HALF_WALL, 5.0)   # y up to 2.65 (and far below the lattice)
        upper = box_sdf(4.0, (3.0 + HALF_DOOR) + 5.0, HALF_WALL, 5.0)   # y from 3.35 on (and far above it)
        f = np.minimum(lower, upper).astype(F32).ravel()
        import dfield_ref
        import plan_ref
        dist = dfield_ref.distance_field(f, shape, origin, step, 0.0)[0]
        dist.setflags(write=False)
        goal = np.array([4.6, 1.6], F32)
        pb = plan_ref.Problem(dist, shape, origin, step, [goal], **PLAN)
        cost = np.ascontiguousarray(plan_ref.solve_dijkstra(pb), F32).ravel()
        cost.setflags(write=False)
        _door.update(shape=shape, origin=origin, step=step, f=f, dist=dist, goal_point=goal.astype(F64), cost=cost,
                     start=np.array([3.4, 4.6, math.cos(-1.2), math.sin(-1.2)], F64))
    return _door


PLAN = dict(clearance=0.2, margin=0.0, gain=4.0)
LOOP = dict(K=512, T=20, seed=3, budget=140,
            opts=dict(dt=0.25, lam=0.5, w_goal=10.0, w_obs=2.0, w_col=200.0, w_off=200.0, margin=0.1, sigma=(0.2, 0.6, 0.0, 0.0), umax=(0.8, 1.5, 0.0, 0.0),
                      umin=(0.0, -1.5, 0.0, 0.0)))


def closed_loop(body=None, clearance=0.0, step_fn=None):
    """Drive LOOP through door_scene with the reference (or step_fn(pose) -> u0, which steps and shifts, in its place): the
    controller sees `body` (None: the point) with the field clearance `clearance`.  Returns dict(steps (None: the goal was not
    reached within the budget), e (the final distance to the goal), states [n, 4], D (the box robot's body clearance at every
    driven state, by body_ref.clearance), hits (the driven states with D < 0))."""
    sc = door_scene()
    o = mppi_ref.default_opts(2, sc["step"])
    o.update(LOOP["opts"], clearance=clearance)
    ctl = body_ref.Controller(2, LOOP["K"], LOOP["T"], LOOP["seed"])
    st = sc["start"].copy()
    visited = [st.copy()]
    out = dict(steps=None)
    for n in range(LOOP["budget"]):
        pose = mppi_ref.pose_of_state(st, 2)
        if step_fn is None:
            u0, _ = ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], pose, o, cost=sc["cost"], body=body)
            ctl.shift()
        else:
            u0 = step_fn(pose, o)
        st = mppi_ref.advance(st, u0, 2, o["dt"])
        visited.append(st.copy())
        if float(np.linalg.norm(st[:2] - sc["goal_point"])) <= 0.3:
            out["steps"] = n + 1
            break
    S = np.array(visited)
    robot = body_ref.box(ROBOT["length"], ROBOT["width"], ROBOT["discs"])
    chk = body_ref.clearance(sc["dist"], sc["shape"], sc["origin"], sc["step"], robot, S, 0.0)
    out.update(e=float(np.linalg.norm(st[:2] - sc["goal_point"])), states=S, D=chk["D"], hits=chk["below"] + chk["off"])
    return out
