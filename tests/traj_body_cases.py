"""Inputs shared by tests/test_traj_body_ref.py (CPU: the body smoother's reference against its defective variants, the branch
census, the geometry) and tests/test_gpu_traj_body.py (the device against the reference): footprints of tests/body_cases.py on
the scenes and hand-made waypoints of tests/traj_cases.py, the degenerate waypoints of tests/body_cases.py, the door scene, and
pose paths with turns in place.  A case is dict(name, scene, x, body, opts, w_turn); `scene` names a field of fields()."""
import numpy as np

import body_cases as bc
import body_ref
import pplan_cases
import pplan_ref
import traj_cases
import traj_ref

F32 = np.float32
F64 = np.float64
NS = (3, 4, 63, 64, 65, 129, 256)            # 65 and 129: a wavefront with one lane
ITERS = 6
DOOR_POLYLINE = np.array([(3.4, 4.6), (4.0, 3.0), (4.6, 1.6)], F32)
DOOR_NS = (32, 64, 128)


def fields():
    """name -> dict(f, shape, origin, step): §7i's 2-D and 3-D scenes and the door scene."""
    d = bc.door_scene()
    return {"balls2": traj_cases.scene(2), "balls3": traj_cases.scene(3), "door": dict(f=d["f"], shape=d["shape"], origin=d["origin"], step=d["step"])}


def ref_dists():
    """name -> the reference's dist of every field (the device tests use the device's own)."""
    return {"balls2": traj_cases.ref_dist(traj_cases.scene(2)), "balls3": traj_cases.ref_dist(traj_cases.scene(3)), "door": bc.door_scene()["dist"]}


def bodies(dim):
    """1, 2 and 16 balls, §7r's asymmetric body (b2 != 0 in 3-D), and a pair whose first ball is the zero ball (e == 0 there)."""
    zero2 = body_ref.make(dim, [(0.0,) * dim, (0.3, 0.1) + ((0.1,) if dim == 3 else ())], [0.0, 0.1])
    return {"one": bc.footprint(dim, 1), "two": bc.footprint(dim, 2), "sixteen": bc.footprint(dim, 16), "asym": bc.traj_body(dim), "zero2": zero2}


def _case(name, scene, x, body, opts, w_turn):
    return dict(name=name, scene=scene, x=np.ascontiguousarray(x, F32), body=body, opts=dict(opts), w_turn=F32(w_turn))


def field_cases(dim, dist):
    """The hand-made batch of traj_cases (free, through the ball, leaving the lattice, along its last cells, a zig-zag next to the
    ball, lattice-exact waypoints, a NaN trajectory: status 2) at every N, the footprints in turn (all of them at N = 64), both
    w_turn; ITERS iterations with the clearance and margin that make e == 0 at the zero ball."""
    sc = traj_cases.scene(dim)
    B = bodies(dim)
    names = ("one", "two", "sixteen", "asym")
    out = []
    for i, N in enumerate(NS):
        x, o, _ = traj_cases.hand_made(sc, dist, N)
        for bn in (names + ("zero2",) if N == 64 else (names[i % 4],)):
            for wt in (0, 1):
                out.append(_case("hand%d_N%d_%s_w%d" % (dim, N, bn, wt), "balls%d" % dim, x, B[bn], dict(o, iters=ITERS), wt))
    x, o, _ = traj_cases.hand_made(sc, dist, 16)
    out.append(_case("hand%d_iters0" % dim, "balls%d" % dim, x, B["asym"], dict(o, iters=0), 1))
    return out


def degenerate_cases():
    """body_cases' repeated waypoints (a zero chord at the start, in the middle, at the end, everywhere) and its trajectories
    that leave the lattice and lie wholly outside it, on the 2-D scene."""
    B = bodies(2)
    o = dict(clearance=F32(0.3), iters=ITERS)
    rep, _ = bc.repeated_waypoints()
    return [_case("repeated_w%d" % wt, "balls2", rep, B["asym"], o, wt) for wt in (0, 1)] + \
           [_case("leaving", "balls2", bc.leaving_waypoints(), B["two"], o, 1)]


def door_cases():
    """The door: the issue's polyline at N = 32, 64, 128 for the 1.0 x 0.4 robot with the defaults, and one batch whose members
    stop at different iterations (the polyline, a straight line in free space, a line through the doorpost, a NaN)."""
    robot = pplan_cases.robot()
    out = [_case("door_N%d" % N, "door", traj_ref.resample_one(DOOR_POLYLINE, N)[None], robot, {}, 1) for N in DOOR_NS]
    N = 40
    mix = np.stack([traj_ref.resample_one(DOOR_POLYLINE, N), traj_cases._line((0.6, 0.7), (3.1, 5.2), N), traj_cases._line((2.0, 2.2), (6.0, 2.4), N),
                    traj_cases._line((5.0, 1.0), (7.5, 5.0), N)]).astype(F32)
    mix[3, 7, 0] = np.nan
    out.append(_case("door_mix", "door", mix, robot, {}, 1))
    return out


def batch_case(dist, m=600, N=12, seed=5):
    """m perturbed lines across the 2-D scene, a few iterations; member 17 has no input (status 2)."""
    sc = traj_cases.scene(2)
    rng = np.random.default_rng(seed)
    hi = (np.array(sc["shape"]) - 1) * sc["step"]
    a = np.array(sc["origin"]) + rng.uniform(0.05, 0.95, (m, 2)) * hi
    b = np.array(sc["origin"]) + rng.uniform(0.05, 0.95, (m, 2)) * hi
    t = np.linspace(0.0, 1.0, N)[None, :, None]
    x = (a[:, None] * (1 - t) + b[:, None] * t + rng.normal(0.0, 0.05, (m, N, 2))).astype(F32)
    x[17, 3, 1] = np.nan
    return _case("batch%d" % m, "balls2", x, bodies(2)["asym"], dict(clearance=F32(0.2), iters=3), 1)


def all_cases(dists):
    """Every case of the device tests but the large batch, on the given dists (name -> dist)."""
    return field_cases(2, dists["balls2"]) + field_cases(3, dists["balls3"]) + degenerate_cases() + door_cases()


# ---- pose paths with turns in place ---------------------------------------------------------------------------------------------
TURN_H = 8
TURN_MOVES = "forward"


def turn_scene():
    """(scene, footprint, goals [1, 3], starts [5, 3]) on pplan_cases.shape_scene(17, 23), the robot moving forward only towards
    a goal with a heading: two routes that end in a turn in place, a start on the goal at the opposite heading (a path of five
    points and no length), the goal itself (one point), a start outside the lattice (no path)."""
    sc = pplan_cases.shape_scene(17, 23)
    o = sc["origin"]
    goals = np.array([(o[0] + 0.2, o[1] + 0.2, 2)], F32)
    starts = np.array([(o[0] + 1.2, o[1] + 1.9, -1), (o[0] + 0.2, o[1] + 0.2, 6), (o[0] + 0.2, o[1] + 0.2, 2), (o[0] + 1.4, o[1] + 0.3, 0),
                       (o[0] - 3.0, o[1], 0)], F32)
    return sc, pplan_cases.footprint(3), goals, starts


TURN_OPTS = dict(clearance=0.0, margin=0.0, turn=0.05)
TURN_ENDS, TURN_ONLY, TURN_POINT, TURN_NONE = (0, 3), 1, 2, 4


def turn_paths_ref():
    """(off, points, heading, status) of the pose planner's reference on turn_scene()."""
    sc, body, goals, starts = turn_scene()
    pb = pplan_cases.problem(sc, body, TURN_H, goals, TURN_MOVES, **TURN_OPTS)
    cost = pplan_ref.solve_dijkstra(pb)
    off, pts, hd, _, st = pplan_ref.paths(pb, cost, pplan_ref.policy(pb, cost), starts, cost.size)
    return off, pts, hd, st


def check_turn_paths(off, pts, st):
    """What the turn paths must hold, asserted alike on the reference's paths and on the device's."""
    ln = off[1:] - off[:-1]
    assert st.tolist() == [0, 0, 0, 0, 1] and ln[TURN_POINT] == 1 and ln[TURN_NONE] == 0 and ln[TURN_ONLY] > 1
    q = pts[off[TURN_ONLY]:off[TURN_ONLY + 1]]
    assert np.all(q == q[0])
    for k in TURN_ENDS:
        q = pts[off[k]:off[k + 1]]
        assert np.all(q[-1] == q[-2]) and not np.all(q == q[0])
