"""Inputs shared by tests/test_obst_ref.py (CPU: the reference against its defective variants) and tests/test_gpu_obst.py (the
device against the reference): sets of moving balls on the scenes and cases of tests/mppi_cases.py.  A case is an mppi case with
`obst` (a set of obst_ref.make), `t_now` and `expect` (branch counters of obst_ref.rollouts that must be > 0 in the first
step) added."""
import math

import numpy as np

import mppi_cases as mc
import mppi_ref
import obst_ref

F64 = np.float64
NS = (1, 2, 63, 64, 65, 256)
# (K, T, n), paired: every K and every T of the issue's list with every n once, the boundaries of n (63, 64, 65: one and two
# passes of a 64-wide table, were a kernel to tile it) at the boundaries of K (63, 64, 65: the last workgroup of the rollouts)
SHAPES = ((1, 1, 1), (63, 2, 63), (64, 33, 64), (65, 33, 65), (257, 2, 2), (1000, 33, 256), (65, 33, 1), (1000, 33, 2))
SHAPES3 = ((64, 33, 1), (64, 33, 65), (257, 2, 1), (257, 2, 65))
T_NOW = 3.5                                              # the absolute time of the cases' poses; the sets' epoch is 1.25


def balls(dim, n, step, **opts):
    """n balls for the shape cases' pose (towards the first static ball): ball 0 crosses the route about 2 s (2-D) or 1.4 s (3-D)
    ahead, the others are scattered over the scene with speeds up to 0.5; epoch 1.25, so that E0 is not 0."""
    rng = np.random.default_rng(100 * dim + n)
    epoch = 1.25
    if dim == 2:
        c0, v0, r0 = (1.7, 8.0), (0.0, -1.0), 0.3
        lo, hi = np.array([-3.0, 1.0]), np.array([12.75, 12.75])
    else:
        c0, v0, r0 = (1.5, 2.8, 1.6), (0.0, -0.7, 0.0), 0.25
        lo, hi = np.zeros(3), np.array([4.6, 3.8, 3.0])
    c = lo + (hi - lo) * rng.random((n, dim))
    v = rng.uniform(-0.5, 0.5, (n, dim))
    r = rng.uniform(0.05, 0.3, n)
    c[0], v[0], r[0] = c0, v0, r0
    # centres are given at the epoch: ball 0 is at c0 at T_NOW
    c[0] = c[0] - v[0] * (T_NOW - epoch)
    return obst_ref.make(dim, c, v, r, epoch=epoch, step=step, **opts)


def with_set(c, obst, expect=(), t_now=T_NOW):
    return dict(c, obst=obst, t_now=t_now, expect=tuple(expect))


def shape_case(K, T, n, dim=2):
    return with_set(mc.shape_case(K, T, dim), balls(dim, n, 0.2 if dim == 3 else 0.25))


def _set2(c, v, r, t_now=T_NOW, **opts):
    """A 2-D set given by where its balls are at t_now."""
    c, v = np.asarray(c, F64).reshape(-1, 2), np.asarray(v, F64).reshape(-1, 2)
    return obst_ref.make(2, c - v * (t_now - 1.25), v, r, epoch=1.25, step=0.25, **opts)


def branch_cases():
    """name -> case, each with the branch counters it must reach."""
    into = mc.branch_cases()["into_ball"]
    cross = ((1.7, 8.0), (0.0, -1.0), 0.3)
    return {
        "crossing": with_set(into, _set2(*[[x] for x in cross]), ("dyn_col", "dyn_band", "dyn_free", "band", "col")),
        "off_lattice": with_set(mc.branch_cases()["off_lattice"], _set2([(-3.3, 1.5)], [(0.0, 0.0)], [0.2]), ("off", "dyn_off", "dyn_col")),
        "margin0": with_set(into, _set2(*[[x] for x in cross], margin=0.0), ("dyn_col", "dyn_free")),
        "second_nearer": with_set(into, _set2([(10.0, 10.0), cross[0]], [(0.0, 0.0), cross[1]], [0.5, cross[2]]),
                                  ("second_nearer", "dyn_col")),
        "identical": with_set(into, _set2([cross[0]] * 2, [cross[1]] * 2, [cross[2]] * 2), ("tie", "dyn_col")),
        "sphere3": with_set(mc.branch_cases()["into_ball3"],
                            obst_ref.make(3, np.array([(1.5, 2.8, 1.6)]) - np.array([(0.0, -0.7, 0.0)]) * (T_NOW - 1.25), [(0.0, -0.7, 0.0)],
                                          [0.25], epoch=1.25, step=0.2), ("dyn_col", "dyn_band", "dyn_free")),
    }


def nan_first_case():
    """A set the library refuses (a NaN centre), for the reference alone: with finite arguments a NaN separation needs an
    infinite elapsed time, at which no ball is near, so the only input that tells "D starts from the first ball's sep" from the
    contract is a first ball without a position and a second one in the way."""
    into = mc.branch_cases()["into_ball"]
    s = _set2([(1.7, 8.0), (1.7, 8.0)], [(0.0, -1.0), (0.0, -1.0)], [0.3, 0.3])
    s["c"][0, 0] = np.nan
    return with_set(into, s, ("dyn_col",))


def ref_step(c, Ubar, tick, variant=None):
    sc = mc.scene(c["dim"])
    cost, goal = mc.terminal_args(c)
    return obst_ref.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], Ubar, c["seed"], tick, c["K"], c["opts"], cost, goal,
                         variant, c["obst"], c["t_now"])


# ---- closed loops -----------------------------------------------------------------------------------------------------------
LOOP_OBST = dict(clearance=0.25, margin=1.0, w_obs=4.0, w_col=100.0)
CROSS_STEP = 30


def closed_loop(cfg, obst=None, step_fn=None, track=None):
    """tests/test_mppi_ref.py's closed loop with the clock running: state n is at time n * dt.  step_fn(pose, t) -> u0 steps and
    shifts in the reference's place.  `track`: a set whose separation from the visited states is measured (default obst).
    Returns dict(steps (None: not reached), least (field distance), e, sep (least separation over the visited states, at their
    times), states)."""
    import dfield_ref
    import traj_cases
    dim = cfg["dim"]
    sc = mc.scene(dim)
    o = mc.opts(dim, **cfg["opts"])
    cost, goal = (sc["cost"], None) if cfg["terminal"] == "plan" else (None, sc["goal_point"])
    ctl = obst_ref.Controller(dim, cfg["K"], cfg["T"], cfg["seed"])
    st = np.array(list(traj_cases.starts(sc)[cfg["start"]].astype(F64)) + [math.cos(cfg["heading"]), math.sin(cfg["heading"])])
    dmin = lambda p: float(dfield_ref.sample(sc["dist"], sc["shape"], sc["origin"], sc["step"], p[None, :dim].astype(np.float32))[0, 0])
    track = obst if track is None else track

    def sep_at(p, t):
        if track is None or not track["n"]:
            return math.inf
        q = p[None, :dim] - obst_ref.at(track, t)
        return float((np.sqrt((q * q).sum(axis=1)) - track["r"]).min())

    out = dict(steps=None, least=dmin(st), e=math.nan, sep=sep_at(st, 0.0), states=[st.copy()])
    for n in range(cfg["budget"]):
        pose = mppi_ref.pose_of_state(st, dim)
        t = n * o["dt"]
        if step_fn is None:
            u0, _ = ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], pose, o, cost=cost, goal=goal, obst=obst, t_now=t)
            ctl.shift()
        else:
            u0 = step_fn(pose, t)
        st = mppi_ref.advance(st, u0, dim, o["dt"])
        out["states"].append(st.copy())
        d = dmin(st)
        if d != d:                                       # off the lattice
            out["least"] = d
            return out
        out["least"] = min(out["least"], d)
        out["sep"] = min(out["sep"], sep_at(st, (n + 1) * o["dt"]))
        out["e"] = float(np.linalg.norm(st[:dim] - sc["goal_point"]))
        if out["e"] <= 2 * sc["step"]:
            out["steps"] = n + 1
            return out
    return out


def least_separation(cfg, states, ball):
    """The least separation of the visited states (state n at time n * dt) from a set."""
    dim = cfg["dim"]
    dt = mc.opts(dim, **cfg["opts"])["dt"]
    least = math.inf
    for n, st in enumerate(states):
        q = st[None, :dim] - obst_ref.at(ball, n * dt)
        least = min(least, float((np.sqrt((q * q).sum(axis=1)) - ball["r"]).min()))
    return least


def crossing_ball(cfg, states, speed, radius):
    """The ball through the unaware robot's state CROSS_STEP at that step's time, perpendicular to its heading there (in the
    x-y plane), given at epoch 0."""
    dim = cfg["dim"]
    dt = mc.opts(dim, **cfg["opts"])["dt"]
    st = states[CROSS_STEP]
    v = np.zeros(dim, F64)
    v[0], v[1] = -st[dim + 1] * speed, st[dim] * speed
    c = st[:dim] - v * (CROSS_STEP * dt)
    return obst_ref.make(dim, [c], [v], [radius], epoch=0.0, step=mc.scene(dim)["step"], **LOOP_OBST)


# ---- timed trajectories against a set ---------------------------------------------------------------------------------------
# (m, N, steps, n), paired.  N = 2 is not a trajectory a handle can hold (Trajectories::kMinN = 3), so the smallest N is 3; steps
# 1000 stays inside one chunk of the kernel's 1024 intervals and CHECK_LONG crosses it.
CHECK_SHAPES = ((1, 3, 1, 1), (3, 4, 2, 64), (65, 64, 63, 65), (3, 256, 64, 256), (1, 64, 65, 1), (3, 64, 256, 64), (3, 64, 1000, 65))
CHECK_SHAPES3 = ((3, 64, 65, 65),)
CHECK_LONG = (3, 64, 2049, 2)                           # (the kernel takes its intervals 1024 at a time)
_timed = {}


def timed_curves(dim, N):
    """(x [11, N, dim], timing) of timing_cases.curves on the scene with the reference's timing (the field's slow-down on); the
    GPU tests hold the device's timing to these bits before they use it."""
    import timing_cases as tc
    import timing_ref
    if (dim, N) not in _timed:
        sc = mc.scene(dim)
        x = tc.curves(sc, N)
        st = np.zeros(x.shape[0], np.uint8)
        st[tc.NAMES.index("nan")] = 2                    # (what the evaluation pass makes of a NaN trajectory)
        tm = timing_ref.time(x, st, tc.opts(sc), (sc["dist"], sc["shape"], sc["origin"], sc["step"]))
        _timed[(dim, N)] = (x, tm)
    return _timed[(dim, N)]


def batch(dim, m, N):
    """(x [m, N, dim], v, t, status): the curves tiled or cut to m trajectories (m = 1: the half circle)."""
    import timing_cases as tc
    x, tm = timed_curves(dim, N)
    idx = np.array([tc.NAMES.index("arc")]) if m == 1 else np.arange(m) % x.shape[0]
    return x[idx], tm["v"][idx], tm["t"][idx], tm["status"][idx]


def check_shape_case(m, N, steps, n, dim=2):
    """dict(x, v, t, status, obst, dt, steps, t0, t_begin, clearance): the scattered balls of the shape cases (their ball 0
    crosses the scene), a clock that does not start at 0 and a dt that spreads `steps` over about 20 s of the trajectories."""
    x, v, t, st = batch(dim, m, N)
    dt = 20.0 / steps if steps > 32 else 0.5
    return dict(x=x, v=v, t=t, status=st, obst=balls(dim, n, 0.2 if dim == 3 else 0.25), dt=dt, steps=steps, t0=0.375, t_begin=T_NOW,
                clearance=None)


def _free_line():
    import timing_cases as tc
    import timing_ref
    x, tm = timed_curves(2, 64)
    k = tc.NAMES.index("free")
    xs, vs, ts = x[k].astype(F64), tm["v"][k].astype(F64), tm["t"][k].astype(F64)
    pos = lambda tau: timing_ref.position(xs, vs, ts, F64(tau))
    return x[k:k + 1], tm["v"][k:k + 1], tm["t"][k:k + 1], tm["status"][k:k + 1], pos, float(ts[-1])


def special_check_cases():
    """name -> case on the free straight line along x (timing status 0), each with the trace counters or results it must show:
    tunnelling: a ball of radius 0.05 at 8 m/s along y through the middle of the robot's interval 6 at its mid-time: 2 m from
      the route at both samples; collides, and does not under "sample_only";
    resting: a ball that reaches x_{N-1} two seconds after the duration;
    still: a ball with v = 0 next to x_{N-1}: bb = 0 in every interval after the duration, all of them tie, the first wins;
    status23: the curves with their status-2 and status-3 rows (N = 3) against the scattered balls."""
    x, v, t, st, pos, dur = _free_line()
    dt = 0.5
    mid = 0.5 * (pos(6 * dt) + pos(7 * dt))
    tun = obst_ref.make(2, [mid - np.array([0.0, 8.0]) * (6.5 * dt)], [(0.0, 8.0)], [0.05], epoch=0.0, step=0.25)
    steps_rest = int(math.ceil((dur + 4.0) / dt))
    end = x[0, -1].astype(F64)
    rest = obst_ref.make(2, [end - np.array([0.0, -1.0]) * (dur + 2.0)], [(0.0, -1.0)], [0.2], epoch=0.0, step=0.25)
    still = obst_ref.make(2, [end + np.array([0.5, 0.0])], [(0.0, 0.0)], [0.125], epoch=0.0, step=0.25)
    base = dict(x=x, v=v, t=t, status=st, dt=dt, t0=0.0, t_begin=0.0, clearance=0.1)
    x3, v3, t3, st3 = batch(2, 11, 3)
    return {
        "tunnelling": dict(base, obst=tun, steps=16, expect=dict(collides=1, first_hit=6, inner=1)),
        "resting": dict(base, obst=rest, steps=steps_rest, expect=dict(collides=1, rest=1)),
        "still": dict(base, obst=still, steps=steps_rest, expect=dict(collides=0, rest=1, bb0=1)),
        "status23": dict(x=x3, v=v3, t=t3, status=st3, obst=balls(2, 2, 0.25), dt=dt, steps=8, t0=0.0, t_begin=T_NOW, clearance=None,
                         expect=dict()),
    }


def ref_check(c, variant=None, trace=None):
    return obst_ref.check(c["x"], c["v"], c["t"], c["status"], c["obst"], c["dt"], c["steps"], c["t0"], c["t_begin"], c["clearance"],
                          variant, trace)
