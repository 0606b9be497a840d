"""One navigation round written once, with the references alone: every stage of a robot's loop takes what the
stages before it computed -- a field restricted to seen space with its unseen_dist plateau, a cost-to-go that is inf over
everything unseen, paths that end at frontier representatives, trajectories resampled from them, smoothed and timed, a controller
seeded with a timed trajectory's controls and ended by a pose plan's projection, a filter and a tracker fed a rendered scan --
where the case tables of the per-object tests hand each object inputs made for it.  It imports nothing from gpismap_amd.

A stage is a function (r) -> outputs: r holds "cfg" (the scene, the pose, the sensor and every option: config(dim)) and the
outputs of the stages before it under their names.  run() calls them in order; tests/test_nav_chain.py asserts on the result
that the round reaches what it is there for, and tests/test_gpu_nav_chain.py passes run() a hook per stage that puts the
device's outputs in the reference's place, so the next stage's reference is evaluated on what the device handed on.

2-D: the door scene of tests/pplan_cases.py (81 x 61, step 0.1), body_cases.ROBOT's box of five discs, H = 16.  3-D:
history_cases.SMALL3 (24 x 20 x 16, step 0.05) with its ball and one more, three balls turning about z, no pose planner."""
import math

import numpy as np

import body_ref
import cover_ref
import dfield_ref
import history_cases as hc
import locate_ref
import mppi_ref
import obst_ref
import pf_ref
import plan_ref
import pplan_cases as pc
import pplan_ref
import render_field_ref
import timing_ref
import track_field_ref
import track_ref
import traj_cases
import traj_ref
import view_ref
from test_track_ref import pose6, pose12

F32 = np.float32
F64 = np.float64
STAGES = ("field", "frame", "cover", "view", "plan", "pplan", "traj", "timing", "control", "localise")
K, T, N = 257, 33, 33
PARTICLES, POSES = 257, 300
_CFG = {}
LOOK_X = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])      # a camera that looks along +x with +z up in the image's y


# ---- the two rounds -----------------------------------------------------------------------------------------------------------
def config(dim):
    """Everything a round is given: the scene's f grid and lattice, the start pose, the sensor, the footprint and the options of
    every stage.  Computed once; the arrays are read-only."""
    if dim in _CFG:
        return _CFG[dim]
    if dim == 2:
        sc = pc.door_scene()
        shape, origin, step, f = sc["shape"], sc["origin"], sc["step"], sc["f"]
        c = dict(scene="pplan_cases.door_scene", pose=pose6(0.4, (1.5, 4.3)), thetas=hc.TH90, off2=np.array((0.03, -0.02), F32), short=F32(7.0),
                 cover=dict(max_gap=hc.GAP5), view=dict(max_gap=hc.GAP5), body=pc.robot(), H=16, pplan=dict(clearance=0.0, margin=0.1, turn=0.05),
                 plan=dict(clearance=0.1, margin=0.2), timing=dict(), dt=0.1, ball_step=38, ball_speed=0.5, ball_radius=0.1,
                 mppi=dict(dt=0.1, lam=100.0, w_goal=2.0), grid=dict(d=0.3, th=0.2), motion=pose6(0.01, (0.004, 0.0)).astype(F64),
                 track=dict(min_inliers=12), pf=dict(), locate=dict())
    else:
        l = hc.SMALL3
        shape, origin, step = l["shape"], l["origin"], l["step"]
        f = traj_cases.balls(shape, step, hc.FIELDS["small3"][1] + [((6.0, 13.0, 11.0), 2.5)])
        body = body_ref.make(3, [(0.06, 0.0, 0.02), (-0.05, 0.03, -0.02), (0.0, -0.05, 0.04)], [0.04, 0.05, 0.03])
        ctr = np.array(origin, F64) + 0.5 * (np.array(shape) - 1) * step
        c = dict(scene="history_cases.SMALL3 with a second ball", pose=pose12(LOOK_X, np.array([ctr[0] - 0.525, ctr[1] - 0.05, ctr[2] - 0.075])),
                 cam=(40.0, 40.0, 31.5, 23.5, 64, 48), short=F32(1.0), cover=dict(), view=dict(), body=body,
                 plan=dict(clearance=0.05, margin=0.1), timing=dict(v_max=0.3, v_min=0.02, a_max=0.2, d_max=0.2, a_lat=0.2),
                 dt=0.1, ball_step=38, ball_speed=0.15, ball_radius=0.04,
                 mppi=dict(dt=0.1, lam=20.0, w_goal=10.0, sigma=(0.1, 0.1, 0.1, 0.5), umin=(-0.4,) * 3 + (-1.0,), umax=(0.4,) * 3 + (1.0,)),
                 grid=dict(d=0.03), motion=hc.MOTION3, track=dict(stride=1, min_inliers=40, max_residual=0.08), pf=dict(stride=2), locate=dict(stride=2))
    f = np.ascontiguousarray(f, F32).ravel()
    f.setflags(write=False)
    c.update(dim=dim, shape=tuple(shape), origin=tuple(origin), step=step, f=f, seed=20 + dim, pf_seed=30 + dim, t_begin=1.5)
    _CFG[dim] = c
    return c


def lat(c):
    return c["shape"], c["origin"], c["step"]


def start_point(c):
    """Where the robot stands: at the sensor (2-D); three lattice steps along the camera's view (3-D: the camera's own position
    lies on its image plane, which sees nothing)."""
    p = np.asarray(c["pose"][:c["dim"]], F64)
    if c["dim"] == 3:
        p = p + 3 * c["step"] * np.asarray(c["pose"][9:12], F64)
    return p.astype(F32)


def candidate_poses(c, reps):
    """The frontier representatives seen from, over history_cases.YAWS8: [reps x 8] poses (2-D: pose6 at the point; 3-D: the start
    pose turned about z, moved over the point at the start's height)."""
    out = []
    for p in np.asarray(reps, F64).reshape(-1, c["dim"]):
        for yaw in hc.YAWS8:
            if c["dim"] == 2:
                out.append(pose6(yaw, (p[0], p[1])))
            else:
                R0 = np.asarray(c["pose"][3:], F64).reshape(3, 3).T
                cz, sz = math.cos(yaw), math.sin(yaw)
                out.append(pose12(np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ R0, np.array([p[0], p[1], float(c["pose"][2])])))
    return np.stack(out).astype(F32) if out else np.zeros((0, 6 if c["dim"] == 2 else 12), F32)


def path_starts(c, seen, reps, dist):
    """The six path starts: the start, the first frontier representative (a seen lattice point that is a goal: a path of one
    point, whose resampled waypoints all coincide), three seen lattice points spread over the mask and the seen lattice point
    nearest to a surface (the first of them), from which no path leaves."""
    idx = np.flatnonzero(np.asarray(seen).ravel())
    pick = np.append(idx[np.linspace(0, idx.size - 1, 5).astype(np.int64)[1:4]], idx[np.argmin(np.asarray(dist).ravel()[idx])])
    return np.concatenate([start_point(c)[None], np.asarray(reps, F32)[:1], cover_ref.lattice_points(pick, *lat(c))]).astype(F32)


def pose_grid(c):
    """Poses round the start for the filter and the scorer: at least POSES of them, the start not among the first."""
    g = c["grid"]
    d = np.linspace(-g["d"], g["d"], 7)
    if c["dim"] == 2:
        th = math.atan2(float(c["pose"][3]), float(c["pose"][2]))
        return locate_ref.pose_grid2(float(c["pose"][0]) + d, float(c["pose"][1]) + d, th + np.linspace(-g["th"], g["th"], 7))
    offs = np.stack(np.meshgrid(d, d, d[:5], indexing="ij"), axis=-1).reshape(-1, 3)
    return locate_ref.pose_grid3(c["pose"], offs, [(0.0, 0.0, 0.0), (0.0, 0.02, 0.0)])


def timing_opts(c):
    o = timing_ref.default_opts(c["dim"], c["step"])
    o.update({k: F32(v) for k, v in c["timing"].items()})
    return o


def mppi_opts(c):
    o = mppi_ref.default_opts(c["dim"], c["step"])
    o.update(c["mppi"], clearance=0.0)
    return o


def cover_opts(c):
    return dict(cover_ref.default_opts(c["dim"], float(F32(c["step"]))), **c["cover"])


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def stage_field(r):
    """1. The distance field of the f grid."""
    c = r["cfg"]
    dist, site = dfield_ref.distance_field(c["f"], *lat(c), 0.0)
    return dict(dist=dist, site=site)


def measured(c, depth, status):
    """The frame a sensor would hand on: a ray without a return is measured short."""
    return np.where(np.asarray(status) == 0, np.asarray(depth, F32), c["short"]).astype(F32)


def stage_frame(r):
    """2. A scan / a depth image rendered from the start pose."""
    c, dist = r["cfg"], r["field"]["dist"]
    if c["dim"] == 2:
        depth, rec, status, stats = render_field_ref.render_scan(dist, *lat(c), c["thetas"], c["pose"], c["off2"])
    else:
        depth, rec, status, stats = render_field_ref.render_depth(dist, *lat(c), c["cam"], c["pose"])
    return dict(depth=depth, rec=rec, status=status, stats=stats, meas=measured(c, depth, status))


def stage_cover(r):
    """3. The frame integrated into an empty mask, the frontiers with their points, the field restricted to seen space."""
    c, dist, meas = r["cfg"], r["field"]["dist"], r["frame"]["meas"]
    o = cover_opts(c)
    none = np.zeros(int(np.prod(c["shape"])), bool)
    if c["dim"] == 2:
        seen = cover_ref.integrate_scan(none, *lat(c), c["thetas"], meas, c["pose"], c["off2"], o["back_off"], o["max_gap"])
    else:
        seen = cover_ref.integrate_depth(none, *lat(c), meas, c["cam"], c["pose"], o["back_off"])
    fr = cover_ref.frontiers(seen, dist, *lat(c), o["clearance"], o["min_size"])
    unseen_dist = -float(F32(c["step"]))
    rd = cover_ref.restrict(seen, dist, unseen_dist)
    return dict(seen=seen, frontiers=fr, reps=fr["rep_point"], restricted=rd, unseen_dist=unseen_dist)


def stage_view(r):
    """4. The gain of looking from every frontier representative over eight yaws."""
    c, dist, seen = r["cfg"], r["field"]["dist"], r["cover"]["seen"]
    poses = candidate_poses(c, r["cover"]["reps"])
    if c["dim"] == 2:
        gain, hits, pred = view_ref.gain_scan(dist, seen, *lat(c), c["thetas"], c["off2"], poses, **c["view"])
    else:
        gain, hits, pred = view_ref.gain_depth(dist, seen, *lat(c), c["cam"], poses, **c["view"])
    return dict(poses=poses, gain=gain, hits=hits, predicted=pred)


def stage_plan(r):
    """5. Cost-to-go and policy on the restricted field towards the frontier representatives, and the six paths."""
    c, rd = r["cfg"], r["cover"]["restricted"]
    pb = plan_ref.Problem(rd, *lat(c), r["cover"]["reps"], **c["plan"])
    cost = plan_ref.solve_dijkstra(pb)
    pol = plan_ref.policy(pb, cost)
    starts = path_starts(c, r["cover"]["seen"], r["cover"]["reps"], rd)
    off, pts, scost, status = plan_ref.paths(pb, cost, pol, starts, cost.size)
    return dict(pb=pb, cost=cost, policy=pol, starts=starts, off=off, points=pts, start_cost=scost, status=status)


def stage_pplan(r):
    """6 (2-D). The pose plan of the footprint on the restricted field towards the same goals at any heading, its paths from
    the six starts and its projection."""
    c, rd = r["cfg"], r["cover"]["restricted"]
    goals = np.concatenate([np.asarray(r["cover"]["reps"], F32), np.full((len(r["cover"]["reps"]), 1), -1, F32)], axis=1)
    pb = pplan_ref.Problem(rd, *lat(c), c["body"], pplan_ref.heading_table(c["H"]), pplan_ref.heading_moves(c["H"], "any"), goals, **c["pplan"])
    cost = pplan_ref.solve_dijkstra(pb)
    pol = pplan_ref.policy(pb, cost)
    starts = np.concatenate([r["plan"]["starts"], np.full((len(r["plan"]["starts"]), 1), -1, F32)], axis=1)
    off, pts, hd, scost, status = pplan_ref.paths(pb, cost, pol, starts, cost.size)
    return dict(pb=pb, goals=goals, cost=cost, policy=pol, starts=starts, off=off, points=pts, heading=hd, start_cost=scost, status=status,
                projection=pplan_ref.project(pb, cost))


def traj_opts(c):
    return dict(traj_ref.default_opts(c["dim"], c["step"]), iters=5)


def stage_traj(r):
    """7. The point paths resampled to N waypoints, five iterations of the smoother, the footprint along the result."""
    c, rd, p = r["cfg"], r["cover"]["restricted"], r["plan"]
    x0, ist = traj_ref.resample(p["off"], p["points"], p["status"], N)
    res = traj_ref.optimize(rd, *lat(c), x0, ist, traj_opts(c))
    return dict(x0=x0, in_status=ist, result=res, clearance=body_ref.traj_clearance(rd, *lat(c), c["body"], res["x"], res["status"], 0.0))


def crossing_set(c, x, tm):
    """Three balls: one through trajectory 0's timed position of step ball_step at that step's time, across its direction of
    travel there (as obst_cases.crossing_ball places its ball), one resting far from every route, one drifting along the lattice's edge."""
    dim = c["dim"]
    xs, vs, ts = x[0].astype(F64), tm["v"][0].astype(F64), tm["t"][0].astype(F64)
    tau = c["ball_step"] * c["dt"]
    p, q = timing_ref.position(xs, vs, ts, F64(tau)), timing_ref.position(xs, vs, ts, F64(tau + c["dt"]))
    e = q[:2] - p[:2]
    n = math.sqrt(float(e[0] * e[0] + e[1] * e[1]))
    h = e / n if n > 0 else np.array([1.0, 0.0])
    v = np.zeros(dim, F64)
    v[0], v[1] = -h[1] * c["ball_speed"], h[0] * c["ball_speed"]
    lo = np.array(c["origin"], F64)
    hi = lo + (np.array(c["shape"]) - 1) * c["step"]
    far = lo + 0.02 * (hi - lo)
    drift = np.zeros(dim, F64)
    drift[0] = 0.25 * c["ball_speed"]
    edge = np.where(np.arange(dim) == 1, hi, lo + 0.1 * (hi - lo))
    return obst_ref.make(dim, [p - v * (c["t_begin"] + tau), far, edge], [v, np.zeros(dim), drift], [c["ball_radius"], 0.5 * c["ball_radius"], c["ball_radius"]],
                         epoch=0.0, step=c["step"])


def stage_timing(r):
    """8. Speeds and times with the restricted field's slow-down, the control sequences, and the timed batch against three balls."""
    c, rd, res = r["cfg"], r["cover"]["restricted"], r["traj"]["result"]
    tm = timing_ref.time(res["x"], res["status"], timing_opts(c), (rd, *lat(c)))
    ctl = timing_ref.controls(res["x"], tm["v"], tm["t"], tm["status"], c["dt"], T)
    S = crossing_set(c, res["x"], tm)
    chk = obst_ref.check(res["x"], tm["v"], tm["t"], tm["status"], S, c["dt"], 2 * T, 0.0, c["t_begin"])
    return dict(timing=tm, controls=ctl, obst=S, check=chk)


def control_step(c, rd, cost, pose, Ubar, tick, t_now, S, q=None):
    """One controller step by body_ref: roll's dict, finish's dict (from `q`: the device's weights in the reference's place), and
    the rollouts the body rule charges where the point rule does not."""
    o = mppi_opts(c)
    args = (rd, *lat(c), pose, Ubar, c["seed"], tick)
    roll = body_ref.roll(*args, K, o, cost, None, obst=S, t_now=t_now, body=c["body"])
    fin = body_ref.finish(roll, roll["q"] if q is None else q, *args, o, cost, None, obst=S, t_now=t_now, body=c["body"])
    point = obst_ref.roll(*args, K, o, cost, None, obst=S, t_now=t_now)
    return dict(roll=roll, finish=fin, body_only=int(np.count_nonzero((roll["hits"] > 0) & (point["hits"] == 0))))


def terminal_cost(r):
    """The cost that ends the controller's rollouts: the pose plan's projection (2-D), the point plan's cost-to-go (3-D)."""
    return r["pplan"]["projection"]["cost2"] if r["cfg"]["dim"] == 2 else r["plan"]["cost"]


def control_pose(c, ctl):
    """The pose the controller steps from: where trajectory 0's controls start, facing as they do (what follow() returns)."""
    return mppi_ref.pose_of_state(np.concatenate([ctl["p0"][0], ctl["heading0"][0]]), c["dim"])


def stage_control(r):
    """9. Two controller steps with a shift between them from trajectory 0's control sequence, with the balls, the footprint and
    the terminal cost of the stages before."""
    c, rd, tmg = r["cfg"], r["cover"]["restricted"], r["timing"]
    cost, S = terminal_cost(r), tmg["obst"]
    pose = control_pose(c, tmg["controls"])
    U = tmg["controls"]["U"][0]
    steps = []
    for k in range(2):
        if k:
            U = mppi_ref.shift(U)
        s = control_step(c, rd, cost, pose, U, k + 1, c["t_begin"] + k * c["dt"], S)
        U = s["finish"]["U"]
        steps.append(s)
    return dict(pose=pose, U0=tmg["controls"]["U"][0], steps=steps)


def local_points(c, meas):
    if c["dim"] == 2:
        return track_ref.points2(c["thetas"], meas, c["off2"])[0]
    return track_ref.points3(meas, c["cam"], c["pf"]["stride"])[0]


def stage_localise(r):
    """10. The filter on a pose grid round the start (one predict, one update with the frame), 300 scored poses and one
    tracking call from a grid pose, all against the whole field."""
    c, dist, meas = r["cfg"], r["field"]["dist"], r["frame"]["meas"]
    dim = c["dim"]
    grid = pose_grid(c)
    o = pf_ref.default_opts(dim)
    f = pf_ref.Filter(grid[:PARTICLES], dim, c["pf_seed"])
    f.predict(c["motion"], o["sigma_t"], o["sigma_r"])
    predicted = f.state.copy()
    f.update(dist, *lat(c), local_points(c, meas), o["max_residual"], o["beta"], o["resample_below"])
    flt = dict(predicted=predicted, state=f.state.copy(), L=f.L.copy(), q=f.q.copy(), cost=f.cost.copy(), inliers=f.inliers.copy(),
               ancestors=f.anc.copy(), neff=f.neff, resampled=bool(f.resampled), estimate=pf_ref.pose64(f.est, dim))
    if dim == 2:
        score = locate_ref.score_scan(dist, *lat(c), c["thetas"], meas, grid[:POSES], c["off2"], **c["locate"])
        track = track_field_ref.track_scan(dist, *lat(c), c["thetas"], meas, grid[5], c["off2"], **c["track"])
    else:
        score = locate_ref.score_depth(dist, *lat(c), meas, c["cam"], grid[:POSES], **c["locate"])
        track = track_field_ref.track_depth(dist, *lat(c), meas, c["cam"], grid[5], **c["track"])
    return dict(grid=grid, filter=flt, score=score, track=track)


STAGE_FN = dict(field=stage_field, frame=stage_frame, cover=stage_cover, view=stage_view, plan=stage_plan, pplan=stage_pplan, traj=stage_traj,
                timing=stage_timing, control=stage_control, localise=stage_localise)


def stages_of(dim):
    return tuple(s for s in STAGES if dim == 2 or s != "pplan")


def run(dim, stages=None, hooks=None):
    """The round of `dim`: dict(cfg, <stage name>: its outputs, ...).  stages: the names to run (default all; a stage needs the ones
    before it that it reads).  hooks: {name: fn(r, out) -> out'} called after the stage; what it returns is handed on in the
    stage's place (None: the stage's own outputs)."""
    r = dict(cfg=config(dim))
    for name in stages_of(dim):
        if stages is not None and name not in stages:
            continue
        out = STAGE_FN[name](r)
        if hooks and name in hooks:
            got = hooks[name](r, out)
            out = out if got is None else got
        r[name] = out
    return r
