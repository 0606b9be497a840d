"""Inputs shared by tests/test_traj_ref.py (CPU: the reference against its defective variants) and tests/test_gpu_traj.py (the
device against the reference): two analytic ball scenes, planner paths through them, and hand-made waypoint batches that
reach every branch of the contract."""
import numpy as np

import dfield_ref
import plan_ref

F32 = np.float32
NS = (3, 4, 63, 64, 65, 128, 255, 256)


def _grid(shape):
    ax = [np.arange(n, dtype=np.float64) for n in shape]
    return np.meshgrid(*ax[::-1], indexing="ij")[::-1]


def balls(shape, step, bl, shells=()):
    """f = distance to the union of balls (centre and radius in lattice units) and of hollow shells (centre, radius, half
    thickness), negative inside the material; flat, x fastest."""
    g = _grid(shape)
    f = np.full(g[0].shape, 1e3)
    for ctr, r in bl:
        f = np.minimum(f, np.sqrt(sum((x - c) ** 2 for x, c in zip(g, ctr))) - r)
    for ctr, r, th in shells:
        f = np.minimum(f, np.abs(np.sqrt(sum((x - c) ** 2 for x, c in zip(g, ctr))) - r) - th)
    return (f * step).astype(F32).ravel()


def scene(dim):
    """dict(shape, origin, step, f, goal): the two-ball 2-D scene (step 0.25: lattice points are exact floats) and a 3-D ball."""
    if dim == 2:
        sc = dict(shape=(64, 48), origin=(-3.0, 1.0), step=0.25, bl=[((30.0, 20.0), 9.4), ((50.0, 35.0), 6.1)], goal=(2, 2))
    else:
        sc = dict(shape=(24, 20, 16), origin=(0.0, 0.0, 0.0), step=0.2, bl=[((11.0, 9.0, 8.0), 5.2)], goal=(0, 0, 0))
    sc["f"] = balls(sc["shape"], sc["step"], sc["bl"])
    return sc


def status_scene(dim):
    """scene(dim) with a hollow shell added: its cavity is free but no path leaves it, so a start there has planner status 3.
    With status_starts and a small max_points (CUT) the planner's paths carry every status 0 .. 4."""
    sc = scene(dim)
    sc["shells"] = [((12.0, 38.0), 5.0, 1.3)] if dim == 2 else [((18.0, 14.0, 11.0), 3.5, 1.2)]
    sc["f"] = balls(sc["shape"], sc["step"], sc["bl"], sc["shells"])
    return sc


CUT = 9                                                  # max_points of the cut batch: longer paths end with status 4, points kept


def status_starts(sc):
    """starts(sc) and the centre of the shell's cavity (status 3)."""
    return np.concatenate([starts(sc), world(sc, sc["shells"][0][0])[None]])


def offgrid_scene():
    """A 2-D scene whose lattice coordinates are not exact floats (origin -0.05, step 0.1) with OFFGRID_STARTS two and four
    cells from the goal along x: resampled to OFFGRID_NS waypoints, a waypoint lands exactly on a path point Q_k, and
    Q_{k-1} + 1 (Q_k - Q_{k-1}) is not Q_k there, so a segment search by < instead of <= changes bits."""
    sc = dict(shape=(24, 16), origin=(-0.05, -0.05), step=0.1, bl=[((16.0, 9.0), 3.2)], goal=(0, 4))
    sc["f"] = balls(sc["shape"], sc["step"], sc["bl"])
    return sc


OFFGRID_STARTS = ((2, 4), (4, 4), (9, 2), (20, 3), (7, 12))
OFFGRID_NS = (3, 5)


def ref_dist(sc):
    return dfield_ref.distance_field(sc["f"], sc["shape"], sc["origin"], sc["step"], 0.0)[0]


def world(sc, cells):
    return (np.array(sc["origin"], np.float64) + np.array(cells, np.float64) * sc["step"]).astype(F32)


def starts(sc, m=40, seed=3):
    """m random starts in the far half of the lattice, then: the goal itself (a path of one point), a start outside the lattice
    (status 1), one inside a ball (status 2), a NaN (status 1)."""
    dim = len(sc["shape"])
    rng = np.random.default_rng(seed)
    hi = np.array(sc["shape"]) - 1
    s = (np.array(sc["origin"]) + rng.uniform(0.5, 1.0, (m, dim)) * hi * sc["step"]).astype(F32)
    extra = np.stack([world(sc, sc["goal"]), world(sc, -3 * np.ones(dim)), world(sc, sc["bl"][0][0]), np.full(dim, np.nan, F32)])
    return np.concatenate([s, extra.astype(F32)])


def plan(sc, dist, st=None, **opts):
    """(pb, cost, policy, off, pts, start_cost, status) of the planner reference towards the scene's goal."""
    kw = dict(clearance=0.0, margin=4 * sc["step"], gain=4.0)
    kw.update(opts)
    pb = plan_ref.Problem(dist, sc["shape"], sc["origin"], sc["step"], [world(sc, sc["goal"])], **kw)
    rc = plan_ref.solve_dijkstra(pb)
    pol = plan_ref.policy(pb, rc)
    off, pts, scost, status = plan_ref.paths(pb, rc, pol, starts(sc) if st is None else st, rc.size)
    return pb, rc, pol, off, pts, scost, status


def status_paths(sc, dist):
    """[(off, pts, status)] of the planner reference on status_scene's starts: the whole paths (statuses 0 .. 3 and a path of one
    point), then the same starts cut at CUT points (status 4 as well)."""
    pb, rc, pol, off, pts, scost, status = plan(sc, dist, status_starts(sc))
    off4, pts4, _, status4 = plan_ref.paths(pb, rc, pol, status_starts(sc), CUT)
    return [(off, pts, status), (off4, pts4, status4)]


def check_status_paths(batches):
    """The populations the status batches must hold, asserted alike on the reference's paths and on the device's."""
    (off, _, st), (off4, _, st4) = batches
    assert set(np.unique(st)) == {0, 1, 2, 3} and ((off[1:] - off[:-1])[st == 0] == 1).any()
    assert set(np.unique(st4)) == {0, 1, 2, 3, 4} and (st4 == 4).sum() >= 5 and np.all((off4[1:] - off4[:-1])[st4 == 4] == CUT)
    assert np.all((off4[1:] - off4[:-1])[(st4 != 0) & (st4 != 4)] == 0)


def _line(a, b, N):
    t = np.linspace(0.0, 1.0, N)[:, None]
    return (np.asarray(a, np.float64) * (1 - t) + np.asarray(b, np.float64) * t).astype(F32)


def hand_made(sc, dist, N):
    """(x [7, N, dim], opts, names): free straight line (stops in its first iteration), a line through the first ball, a line that
    leaves the lattice, a line along the lattice's last cells, a zig-zag next to the ball (trust region), a trajectory whose
    waypoints 1 and 2 sit on lattice points with e exactly 0 and exactly margin, a trajectory with a NaN.  opts carries the
    clearance and margin that make those two values exact."""
    shape, dim, step = sc["shape"], len(sc["shape"]), sc["step"]
    hi = np.array(shape) - 1
    ctr = np.array(sc["bl"][0][0])
    rad = sc["bl"][0][1]
    lo_c = np.ones(dim)
    free = _line(world(sc, lo_c), world(sc, np.where(np.arange(dim) == 0, hi[0] - 1, 1.0)), N)
    through = _line(world(sc, ctr - np.eye(dim)[0] * (rad + 4)), world(sc, ctr + np.eye(dim)[0] * (rad + 4)), N)
    leaves = _line(world(sc, hi - 3), world(sc, hi + 4), N)
    last = _line(world(sc, np.where(np.arange(dim) == 0, 1.0, hi)), world(sc, hi), N)
    zz = _line(world(sc, ctr - np.eye(dim)[0] * (rad + 3) + np.eye(dim)[1] * rad), world(sc, ctr + np.eye(dim)[0] * (rad + 3) + np.eye(dim)[1] * rad), N)
    zz[1:-1:2, 1] += F32(3 * step)
    # two lattice points below the first ball with finite dist, the second two steps further from it than the first
    d3 = dist.reshape(shape[::-1])
    c0 = [int(round(v)) for v in ctr]
    p1 = tuple(c0[a] - (int(rad) + 3 if a == 1 else 0) for a in range(dim))
    p2 = tuple(p1[a] - (2 if a == 1 else 0) for a in range(dim))
    v1 = d3[p1[::-1]]
    assert np.isfinite(v1) and v1 > 0 and d3[p2[::-1]] > v1
    exact = _line(world(sc, p1), world(sc, lo_c * 8), N)
    exact[1] = world(sc, p1)
    exact[2] = world(sc, p2)
    bad = free.copy()
    bad[N // 2, dim - 1] = np.nan
    x = np.stack([free, through, leaves, last, zz, exact, bad]).astype(F32)
    opts = dict(clearance=F32(v1), margin=F32(d3[p2[::-1]] - v1))
    return x, opts, ("free", "through", "leaves", "last", "zigzag", "exact", "nan")
