"""Inputs shared by tests/test_mppi_ref.py (CPU: the reference against its defective variants) and tests/test_gpu_mppi.py (the
device against the reference): the two ball scenes of tests/traj_cases.py, starts that reach every branch of the contract and
the (K, T) shapes.  A case is a dict(dim, K, T, seed, pose, terminal ("plan" / "goal"), opts, nominal (None or [U] values
every row of the sequence is set to), expect (branch counters of mppi_ref.rollouts that must be > 0 in the first step))."""
import math

import numpy as np

import mppi_ref
import traj_cases

F64 = np.float64
KS = (1, 63, 64, 65, 255, 256, 257, 1000, 4097)
TS = (1, 2, 33, 256)
SHAPES = tuple((K, T) for T in TS for K in KS if T < 256 or K <= 257)
SHAPES3 = ((1, 2), (64, 33), (257, 2), (1000, 33))

_scene = {}


def scene(dim):
    """traj_cases.scene(dim) with the reference's distances, the planner reference's cost-to-go and the goal point added;
    computed once."""
    if dim not in _scene:
        sc = traj_cases.scene(dim)
        sc["dist"] = traj_cases.ref_dist(sc)
        sc["cost"] = np.ascontiguousarray(traj_cases.plan(sc, sc["dist"])[1], np.float32).ravel()
        sc["goal_point"] = traj_cases.world(sc, sc["goal"]).astype(F64)
        for k in ("dist", "cost"):
            sc[k].setflags(write=False)
        _scene[dim] = sc
    return _scene[dim]


def pose(dim, xyz, heading):
    return mppi_ref.pose_of_state(list(xyz) + [math.cos(heading), math.sin(heading)], dim)


def opts(dim, **kw):
    o = mppi_ref.default_opts(dim, 0.2 if dim == 3 else 0.25)            # (the scenes' lattice steps)
    o.update(kw)
    return o


def case(dim, K, T, pose_, terminal, nominal=None, expect=(), seed=5, **kw):
    return dict(dim=dim, K=K, T=T, seed=seed, pose=pose_, terminal=terminal, opts=opts(dim, **kw), nominal=nominal, expect=tuple(expect))


# 2-D: x in [-3, 12.75], y in [1, 12.75]; balls at (4.5, 6.0) r 2.35 and (9.5, 9.75) r 1.525; the goal at (-2.5, 1.5)
FREE2 = pose(2, (0.0, 10.0), -2.0)
INTO_BALL2 = pose(2, (0.5, 6.0), 0.0)
LEAVES2 = pose(2, (-2.0, 1.5), math.pi)
# 3-D: x in [0, 4.6], y in [0, 3.8], z in [0, 3.0]; a ball at (2.2, 1.8, 1.6) r 1.04; the goal at the origin
INTO_BALL3 = pose(3, (0.3, 1.8, 1.6), 0.0)
FREE3 = pose(3, (0.8, 3.0, 2.4), -2.0)


def shape_case(K, T, dim=2):
    """The case the shapes run: towards the first ball with a nominal forward speed, so that within 33 steps of 0.1 s rollouts
    cross the margin band and enter the ball; the planner's cost-to-go ends the 2-D ones, the goal point the 3-D ones."""
    if dim == 2:
        return case(2, K, T, INTO_BALL2, "plan", nominal=(0.6, 0.1), gamma=0.5)
    return case(3, K, T, INTO_BALL3, "goal", nominal=(0.5, 0.05, -0.05, 0.1), gamma=0.5)


def branch_cases():
    """name -> case, each with the branch counters it must reach."""
    return {
        "off_lattice": case(2, 257, 12, LEAVES2, "plan", nominal=(1.0, 0.0), expect=("off", "term_off")),
        "into_ball": case(2, 257, 33, INTO_BALL2, "plan", nominal=(0.6, 0.0), expect=("col", "band", "free", "term_blocked", "term_cost")),
        "margin0": case(2, 257, 33, INTO_BALL2, "plan", nominal=(1.0, 0.0), margin=0.0, expect=("col", "free")),
        "clamp": case(2, 257, 8, FREE2, "plan", nominal=(0.9, 0.9), sigma=(2.0, 3.0, 0.0, 0.0), expect=("clamped", "term_cost")),
        "sigma0": case(2, 257, 8, FREE2, "plan", nominal=(0.5, 0.2), sigma=(0.25, 0.0, 0.0, 0.0), expect=("free",)),
        "gamma0": case(2, 257, 8, FREE2, "plan", nominal=(0.5, 0.2), gamma=0.0, expect=("free",)),
        "goal2": case(2, 257, 8, FREE2, "goal", nominal=(0.5, 0.2), expect=("term_goal",)),
        "into_ball3": case(3, 300, 33, INTO_BALL3, "goal", nominal=(1.0, 0.0, 0.0, 0.1), expect=("col", "band", "free", "term_goal")),
        "plan3": case(3, 300, 12, FREE3, "plan", nominal=(0.5, 0.1, -0.1, 0.1), w_off=7.0, expect=("free", "term_cost")),
        "leaves3": case(3, 65, 12, pose(3, (0.2, 0.2, 2.9), 0.3), "plan", nominal=(0.0, 0.0, 1.0, 0.0), expect=("off", "term_off")),
    }


def terminal_args(c):
    """(cost, goal) for mppi_ref of a case."""
    sc = scene(c["dim"])
    return (sc["cost"], None) if c["terminal"] == "plan" else (None, sc["goal_point"])


def nominal_of(c):
    """The sequence [T, U] a case starts from."""
    U = mppi_ref.ncontrols(c["dim"])
    if c["nominal"] is None:
        return np.zeros((c["T"], U), F64)
    return np.tile(np.asarray(c["nominal"], F64)[None, :U], (c["T"], 1))


def ref_step(c, Ubar, tick, variant=None):
    sc = scene(c["dim"])
    cost, goal = terminal_args(c)
    return mppi_ref.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], Ubar, c["seed"], tick, c["K"], c["opts"], cost, goal,
                         variant)
