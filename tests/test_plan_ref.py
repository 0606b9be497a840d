"""The planner's reference (tests/plan_ref.py) against itself: whole-array relaxation and heapq Dijkstra give the same bits, a
hand-computed corridor, and the invariants of the paths."""
import numpy as np
import pytest

import plan_ref

F32 = np.float32
U32 = np.uint32


def _field(shape, seed, step):
    """A rough analytic distance-like grid: distance to a few random balls, negative inside them."""
    rng = np.random.default_rng(seed)
    ax = [np.arange(n, dtype=np.float64) * step for n in shape]
    g = np.meshgrid(*ax[::-1], indexing="ij")[::-1]
    d = np.full(g[0].shape, np.inf)
    for _ in range(5):
        ctr = [rng.uniform(0, (n - 1) * step) for n in shape]
        r = rng.uniform(1.0, 3.0) * step
        d = np.minimum(d, np.sqrt(sum((c - x) ** 2 for c, x in zip(ctr, g))) - r)
    return d.astype(F32).ravel()


CASES = [((23, 17), 0.25, 0, 0.0), ((23, 17), 0.25, 1, 4.0), ((19, 22), 0.1, 1, 20.0), ((19, 22), 0.1, 0, 4.0),
         ((9, 8, 7), 0.5, 1, 0.0), ((9, 8, 7), 0.5, 0, 4.0), ((11, 7, 9), 0.05, 1, 20.0)]


@pytest.mark.parametrize("shape,step,conn,gain", CASES)
def test_sweep_equals_dijkstra(shape, step, conn, gain):
    dist = _field(shape, len(shape) * 7 + conn, step)
    origin = (-1.0, 0.5, 2.0)[:len(shape)]
    free = np.flatnonzero(dist >= 0)
    rng = np.random.default_rng(5)
    cells = rng.choice(free, 2, replace=False)
    nx, ny = shape[0], shape[1]
    ijk = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], axis=1)[:, :len(shape)]
    goals = (np.array(origin) + ijk * step).astype(F32)
    pb = plan_ref.Problem(dist, shape, origin, step, goals, clearance=0.0, margin=3 * step, gain=gain, connectivity=conn)
    assert pb.goals_kept == 2
    goal_pts = pb.world(np.pad(ijk, ((0, 0), (0, 3 - len(shape)))))
    a, b = plan_ref.solve_sweep(pb), plan_ref.solve_dijkstra(pb)
    assert np.array_equal(a.view(U32), b.view(U32))
    assert np.isfinite(a).sum() > 20 and np.all(np.isinf(a[dist < 0]))
    pol = plan_ref.policy(pb, a)
    fin = np.isfinite(a)
    assert np.all(pol[~fin] == 255) and np.all(pol[fin] != 255) and (pol == 13).sum() == 2
    # every finite non-goal point has a strictly cheaper policy target, and paths obey the invariants
    starts = (np.array(origin) + np.stack([rng.uniform(-1, n, 40) for n in shape], axis=1) * step).astype(F32)
    off, pts, sc, st = plan_ref.paths(pb, a, pol, starts, max_points=10 ** 6)
    assert set(np.unique(st)) <= {0, 1, 2, 3} and (st == 0).sum() > 3
    for t in np.flatnonzero(st == 0):
        plan_ref.check_path_invariants(pb, a, pts[off[t]:off[t + 1]])
        assert np.any(np.all(pts[off[t + 1] - 1] == goal_pts, axis=1))
    assert np.all(off[1:][st != 0] == off[:-1][st != 0])


def test_hand_computed_corridor():
    """5 x 3 lattice, step 1, walls along j = 0 and j = 2, goal at (0, 1): cost i along the corridor, every policy byte 12
    (dx = -1), the path from (4, 1) visits the five corridor points."""
    dist = np.array([[-1] * 5, [1] * 5, [-1] * 5], F32).ravel()
    pb = plan_ref.Problem(dist, (5, 3), (0.0, 0.0), 1.0, [[0.2, 0.9]], clearance=0.0, margin=0.0, gain=4.0, connectivity=1)
    cost = plan_ref.solve_dijkstra(pb)
    want = np.full((3, 5), np.inf, F32)
    want[1] = [0, 1, 2, 3, 4]
    assert np.array_equal(cost.view(U32), want.ravel().view(U32))
    assert np.array_equal(plan_ref.solve_sweep(pb).view(U32), cost.view(U32))
    pol = plan_ref.policy(pb, cost).reshape(3, 5)
    assert np.all(pol[0] == 255) and np.all(pol[2] == 255) and list(pol[1]) == [13, 12, 12, 12, 12]
    off, pts, sc, st = plan_ref.paths(pb, cost, pol, [[4.0, 1.0], [2.0, 0.0], [9.0, 1.0], [np.nan, 1.0]], max_points=100)
    assert list(st) == [0, 2, 1, 1] and list(off) == [0, 5, 5, 5, 5]
    assert np.array_equal(pts, np.array([[4, 1], [3, 1], [2, 1], [1, 1], [0, 1]], F32))
    assert sc[0] == 4 and np.isinf(sc[1]) and np.isnan(sc[2])
    # gain: contact cost 1 + gain on the whole corridor (dist = clearance = 1, margin 1): every weight is 5
    pb2 = plan_ref.Problem(dist, (5, 3), (0.0, 0.0), 1.0, [[0.0, 1.0]], clearance=1.0, margin=1.0, gain=4.0)
    assert list(plan_ref.solve_dijkstra(pb2).reshape(3, 5)[1]) == [0, 5, 10, 15, 20]
    # max_points cuts the walk off with status 4 and keeps the prefix
    off, pts, sc, st = plan_ref.paths(pb, cost, pol, [[4.0, 1.0]], max_points=3)
    assert list(st) == [4] and np.array_equal(pts, np.array([[4, 1], [3, 1], [2, 1]], F32))


def test_no_diagonal_squeeze_and_pocket():
    """Two blocked corners touching diagonally are not passed between; a closed pocket stays at +inf with status 3."""
    d = np.ones((4, 4), F32)
    d[1, 2] = d[2, 1] = -1.0
    pb = plan_ref.Problem(d.ravel(), (4, 4), (0.0, 0.0), 1.0, [[0.0, 0.0]], connectivity=1)
    cost = plan_ref.solve_dijkstra(pb).reshape(4, 4)
    assert cost[1, 1] == np.sqrt(F32(2)) and cost[2, 2] > F32(4)      # around, not through
    p = np.ones((7, 7), F32)
    p[2, 2:5] = p[4, 2:5] = p[2:5, 2] = p[2:5, 4] = -1.0               # a ring around (3, 3)
    pb = plan_ref.Problem(p.ravel(), (7, 7), (0.0, 0.0), 1.0, [[0.0, 0.0]])
    cost = plan_ref.solve_sweep(pb)
    pol = plan_ref.policy(pb, cost)
    assert np.isinf(cost.reshape(7, 7)[3, 3]) and pol.reshape(7, 7)[3, 3] == 255
    _, _, _, st = plan_ref.paths(pb, cost, pol, [[3.0, 3.0]], 50)
    assert list(st) == [3]
