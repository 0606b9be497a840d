"""Path planning through a distance field on the GPU (csrc/plan.hip, gpis_plan_*): cost-to-go, policy and paths against the
numpy / heapq reference (tests/plan_ref.py) bit for bit -- the fixed point does not depend on the schedule, so there are no
tolerances -- at every tile edge, over many outer rounds, with ties, for every option, and the error paths."""
import ctypes as C
import itertools

import numpy as np
import pytest

import plan_ref
import replay

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
T2, T3 = 32, 8                                           # tile edges of csrc/plan.h
BOX2 = dict(origin=(-4.9, -14.9), step=(0.1, 0.1), shape=(249, 199))


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _field(f, shape, origin, step, level=0.0, df=None):
    """(DistanceField, its own dist grid flat) of an analytic f grid (flat, x fastest)."""
    import gpismap_amd
    df = df if df is not None else gpismap_amd.DistanceField()
    t = _dev(np.ascontiguousarray(f, F32).ravel())
    df.from_grid(t.data_ptr(), shape, origin, step, level)
    return df, df.get()[0].ravel()


def _grid(shape, origin, step):
    ax = [origin[a] + np.arange(shape[a], dtype=np.float64) * step for a in range(len(shape))]
    return np.meshgrid(*ax[::-1], indexing="ij")[::-1]                  # [x, y(, z)] arrays of shape shape[::-1]


def _balls(shape, origin, step, balls):
    """f = distance to the union of balls (centre in lattice units, radius in lattice units), negative inside."""
    g = _grid(shape, (0.0,) * len(shape), 1.0)
    f = np.full(g[0].shape, 1e3)
    for ctr, r in balls:
        f = np.minimum(f, np.sqrt(sum((x - c) ** 2 for x, c in zip(g, ctr))) - r)
    return (f * step).astype(F32).ravel()


def _pts(cells, origin, step):
    return (np.array(origin, np.float64) + np.array(cells, np.float64) * step).astype(F32)


def _solve_vs_ref(df, dist, shape, origin, step, goals, planner=None, ref="sweep", **opts):
    """Solve on the device and by the reference on the device's own dist; compare every bit.  Returns (planner, pb, cost, pol)."""
    import gpismap_amd
    pl = planner if planner is not None else gpismap_amd.Planner()
    assert df.plan(goals, planner=pl, **opts) is pl
    o = gpismap_amd.plan_opts(len(shape), F32(step), **{k: v for k, v in opts.items() if k != "max_rounds"})
    pb = plan_ref.Problem(dist, shape, origin, step, goals, clearance=o.clearance, margin=o.margin, gain=o.gain,
                          connectivity=o.connectivity)
    rc = plan_ref.solve_sweep(pb) if ref == "sweep" else plan_ref.solve_dijkstra(pb)
    rp = plan_ref.policy(pb, rc)
    cost, pol = pl.get()
    assert cost.shape == tuple(shape)[::-1] and pol.dtype == np.uint8
    assert _bits_equal(cost.ravel(), rc)
    assert np.array_equal(pol.ravel(), rp)
    inf = pl.info()
    fin = np.isfinite(rc)
    assert inf["valid"] == 1 and inf["dim"] == len(shape) and (inf["nx"], inf["ny"], inf["nz"])[:len(shape)] == tuple(shape)
    assert inf["goals"] == pb.goals_given and inf["goals_kept"] == pb.goals_kept
    assert inf["free"] == int(pb.free.sum()) and inf["reachable"] == int(fin.sum())
    assert F32(inf["max_cost"]) == (rc[fin].max() if fin.any() else F32(0)) and inf["step"] == F32(step)
    assert inf["rounds"] >= 1
    return pl, pb, rc, rp


# ---- tile edges ---------------------------------------------------------------------------------------------------------------
def test_tile_edge_shapes_2d():
    origin, step = (-1.0, 2.0), 0.25
    for shape in itertools.product((T2, T2 + 1, 2 * T2 - 1), repeat=2):
        f = _balls(shape, origin, step, [((shape[0] * 0.3, shape[1] * 0.7), 5.3), ((T2 - 0.5, 6.0), 2.2)])
        df, dist = _field(f, shape, origin, step)
        # a lattice corner, both sides of a tile corner (outside the lattice on an axis of one tile: dropped), two goals in one
        # tile, a duplicate
        goals = _pts([(0, 0), (T2 - 1, T2 - 1), (T2, T2), (3, 2), (3, 2), (2, 9)], origin, step)
        _, pb, rc, _ = _solve_vs_ref(df, dist, shape, origin, step, goals)
        assert pb.goals_kept >= 5 and np.isfinite(rc).sum() > 900


def test_tile_edge_shapes_3d():
    origin, step = (0.5, -1.0, 0.0), 0.05
    for shape in itertools.product((T3, T3 + 1, 2 * T3 - 1), repeat=3):
        f = _balls(shape, origin, step, [((shape[0] * 0.3, shape[1] * 0.7, shape[2] * 0.5), 2.4)])
        df, dist = _field(f, shape, origin, step)
        goals = _pts([(0, 0, 0), (T3 - 1, T3 - 1, T3 - 1), (T3, T3, T3), (1, 2, 0), (1, 2, 0), (2, 0, 1)], origin, step)
        _, pb, rc, _ = _solve_vs_ref(df, dist, shape, origin, step, goals)
        assert pb.goals_kept >= 5 and np.isfinite(rc).sum() > 400


def test_small_and_odd_lattices():
    df, dist = _field(np.ones(4, F32), (2, 2), (0.0, 0.0), 1.0)
    _solve_vs_ref(df, dist, (2, 2), (0.0, 0.0), 1.0, [[1.0, 1.0]])
    df, dist = _field(np.ones(30, F32), (5, 3, 2), (0.0, 0.0, 0.0), 0.5)
    _solve_vs_ref(df, dist, (5, 3, 2), (0.0, 0.0, 0.0), 0.5, [[2.0, 0.5, 0.5]])
    shape, origin, step = (37, 29), (-3.0, 1.0), 0.1
    df, dist = _field(_balls(shape, origin, step, [((18.0, 14.0), 7.4), ((30.0, 5.0), 3.1)]), shape, origin, step)
    _solve_vs_ref(df, dist, shape, origin, step, _pts([(1, 1), (35, 27)], origin, step))
    shape, origin, step = (21, 19, 17), (0.0, 0.0, 0.0), 0.2
    df, dist = _field(_balls(shape, origin, step, [((10.0, 9.0, 8.0), 5.2), ((3.0, 15.0, 12.0), 2.5)]), shape, origin, step)
    _solve_vs_ref(df, dist, shape, origin, step, _pts([(0, 0, 0), (20, 18, 16)], origin, step))


# ---- many rounds -------------------------------------------------------------------------------------------------------------
def _serpentine():
    shape, origin, step = (97, 65), (0.0, 0.0), 0.1
    f = np.ones((65, 97), F32)
    for w, i in enumerate(range(4, 97, 8)):              # walls every 8 columns, the gap alternating between the two ends
        f[:, i] = -1.0
        if w % 2 == 0:
            f[61:, i] = 1.0
        else:
            f[:4, i] = 1.0
    return f.ravel(), shape, origin, step


def test_many_rounds_serpentine_and_round_cap():
    import gpismap_amd
    f, shape, origin, step = _serpentine()
    df, dist = _field(f, shape, origin, step)
    goals = _pts([(0, 0)], origin, step)
    pl, pb, rc, _ = _solve_vs_ref(df, dist, shape, origin, step, goals)
    assert np.isfinite(rc.reshape(65, 97)[0, 96]) and rc[np.isfinite(rc)].max() > 12 * 6.0       # the front ran through every corridor
    tile_columns = (shape[0] + T2 - 1) // T2
    assert pl.info()["rounds"] > tile_columns, pl.info()
    assert pl.info()["tile_launches"] >= pl.info()["rounds"]
    # a cap of two rounds: GPIS_ERR_LIMIT and no result
    o = gpismap_amd.plan_opts(2, F32(step), max_rounds=2)
    L = gpismap_amd.lib()
    assert L.gpis_plan_solve(pl.h, df.h, goals.ctypes.data_as(C.POINTER(C.c_float)), 1, C.byref(o), None) == -4
    assert pl.info()["valid"] == 0 and pl.device_ptrs() == (0, 0)
    assert L.gpis_plan_get(pl.h, None, None) == -3
    with pytest.raises(gpismap_amd.GpisError):
        pl.get()


def _smooth(shape, step, seed, k):
    rng = np.random.default_rng(seed)
    g = _grid(shape, (0.0,) * len(shape), step)
    f = np.zeros(g[0].shape)
    for _ in range(6):
        kk = rng.normal(0, k, len(shape))
        f += np.sin(sum(x * c for x, c in zip(g, kk)) + rng.uniform(0, 6.3))
    return f.astype(F32).ravel()


def test_smooth_random_field_against_sweep():
    shape, origin, step = (257, 193), (-3.0, 1.0), 0.05
    df, dist = _field(_smooth(shape, step, 2, 0.8), shape, origin, step, level=-0.4)
    free = np.flatnonzero(dist >= 0)
    cells = [(int(p % 257), int(p // 257)) for p in free[[10, free.size // 2, free.size - 10]]]
    pl, pb, rc, _ = _solve_vs_ref(df, dist, shape, origin, step, _pts(cells, origin, step))
    assert np.isfinite(rc).sum() > 5000 and pl.info()["tile_launches"] > pl.info()["rounds"]


# ---- ties --------------------------------------------------------------------------------------------------------------------
def test_ties_symmetric_box():
    f = np.ones((9, 9, 9), F32)
    f[3:6, 3:6, 3:6] = -1.0
    df, dist = _field(f.ravel(), (9, 9, 9), (0.0, 0.0, 0.0), 1.0)
    for conn in (0, 1):
        _, pb, rc, rp = _solve_vs_ref(df, dist, (9, 9, 9), (0.0, 0.0, 0.0), 1.0, [[4.0, 4.0, 0.0]], connectivity=conn)
        c3 = rc.reshape(9, 9, 9)
        assert _bits_equal(c3, c3[:, :, ::-1]) and _bits_equal(c3, c3[:, ::-1, :]) and _bits_equal(c3, c3.transpose(0, 2, 1))
        # behind the cube the mirror-image moves tie in value and in cost[q]: the smaller direction index wins
        p3 = rp.reshape(9, 9, 9)
        assert p3[8, 4, 4] != 255 and plan_ref.offset(int(p3[8, 4, 4]))[:2] <= (0, 0)


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_options():
    for shape, origin, step, balls, goals in [((37, 29), (-3.0, 1.0), 0.1, [((18.0, 14.0), 7.4)], [(1, 1)]),
                                              ((21, 19, 17), (0.0, 0.0, 0.0), 0.2, [((10.0, 9.0, 8.0), 5.2)], [(0, 0, 0)])]:
        df, dist = _field(_balls(shape, origin, step, balls), shape, origin, step)
        g = _pts(goals, origin, step)
        costs = []
        for gain, margin, conn in [(0.0, None, 1), (4.0, None, 1), (4.0, 0.0, 1), (4.0, None, 0), (0.0, 0.0, 0), (1e4, 1.0, 1)]:
            kw = dict(gain=gain, connectivity=conn)
            if margin is not None:
                kw["margin"] = margin
            costs.append(_solve_vs_ref(df, dist, shape, origin, step, g, **kw)[2])
        assert _bits_equal(costs[0], costs[2]) and not _bits_equal(costs[0], costs[1]) and not _bits_equal(costs[1], costs[3])
        # a clearance at exactly a stored dist value: those points are free
        pos = np.sort(dist[dist > 0])
        v = float(pos[pos.size // 2])
        _, pb, rc, _ = _solve_vs_ref(df, dist, shape, origin, step, g, clearance=v)
        assert np.all(pb.free.ravel()[dist == F32(v)]) and pb.free.sum() < (dist >= 0).sum()
        # a clearance that leaves nothing free
        pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, g, clearance=1e9)
        assert pb.free.sum() == 0 and np.all(np.isinf(rc)) and np.all(rp == 255) and pl.info()["goals_kept"] == 0
    # a field without sites: dist = +inf everywhere, every point free at cost 1
    df, dist = _field(np.ones(23 * 40, F32), (40, 23), (0.0, 0.0), 0.5)
    assert np.all(dist == np.inf)
    _, pb, rc, _ = _solve_vs_ref(df, dist, (40, 23), (0.0, 0.0), 0.5, [[0.0, 0.0]])
    assert np.all(pb.c == 1) and rc.reshape(23, 40)[0, 39] == F32(19.5)


# ---- reachability ------------------------------------------------------------------------------------------------------------
def test_pocket_and_dropped_goals():
    shape, origin, step = (40, 35), (0.0, 0.0), 1.0
    f = np.ones((35, 40), F32)
    f[10, 10:21] = f[20, 10:21] = f[10:21, 10] = f[10:21, 20] = -1.0            # a closed ring
    df, dist = _field(f.ravel(), shape, origin, step)
    pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, [[1.0, 1.0]])
    inside = np.zeros((35, 40), bool)
    inside[12:19, 12:19] = True
    assert np.all(np.isinf(rc.reshape(35, 40)[inside])) and np.all(rp.reshape(35, 40)[inside] == 255)
    assert pb.free[0][inside].all()
    paths, sc, st = pl.paths([[15.0, 15.0], [10.0, 15.0], [1.0, 30.0]])
    assert list(st) == [3, 2, 0] and np.isinf(sc[0]) and np.isinf(sc[1]) and len(paths[0]) == 0 and len(paths[2]) > 20
    # every goal blocked, outside or non-finite: the solve succeeds with nothing reachable
    pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, [[10.0, 12.0], [-3.0, 2.0], [50.0, 2.0], [np.nan, 1.0], [np.inf, 1.0]])
    assert pl.info()["goals_kept"] == 0 and pl.info()["goals"] == 5 and np.all(np.isinf(rc)) and np.all(rp == 255)
    _, sc, st = pl.paths([[1.0, 1.0]])
    assert list(st) == [3]


# ---- paths -------------------------------------------------------------------------------------------------------------------
def _paths_vs_ref(pl, pb, rc, rp, starts, max_points):
    paths, sc, st = pl.paths(starts, max_points=max_points)
    off, pts, rsc, rst = plan_ref.paths(pb, rc, rp, starts, max_points if max_points is not None else rc.size)
    assert np.array_equal(st, rst) and np.array_equal(pl.last_off, off)
    assert np.array_equal(sc.view(U32), rsc.view(U32))
    got = np.concatenate(paths) if off[-1] else np.zeros((0, pb.dim), F32)
    assert _bits_equal(got, pts)
    return paths, sc, st


def test_paths_equal_reference_and_hold_their_invariants():
    for shape, origin, step, balls, goal in [((70, 45), (-3.0, 1.0), 0.1, [((30.0, 20.0), 9.4), ((55.0, 35.0), 6.1)], (2, 2)),
                                             ((21, 19, 17), (0.0, 0.0, 0.0), 0.2, [((10.0, 9.0, 8.0), 5.2)], (0, 0, 0))]:
        df, dist = _field(_balls(shape, origin, step, balls), shape, origin, step)
        pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, _pts([goal], origin, step))
        rng = np.random.default_rng(11)
        lo = np.array(origin)
        hi = lo + (np.array(shape) - 1) * step
        starts = (lo + rng.uniform(-0.08, 1.08, (1000, len(shape))) * (hi - lo)).astype(F32)      # some outside
        starts[5, 0] = np.nan
        starts[6, 1] = np.inf
        paths, sc, st = _paths_vs_ref(pl, pb, rc, rp, starts, None)
        assert set(np.unique(st)) == {0, 1, 2} and (st == 0).sum() > 400
        for t in np.flatnonzero(st == 0)[::15]:
            plan_ref.check_path_invariants(pb, pl.get()[0].ravel(), paths[t])
            assert np.array_equal(paths[t][-1], _pts([goal], origin, step)[0])
        # the cut-off: status 4 with the reference's prefix
        paths, sc, st = _paths_vs_ref(pl, pb, rc, rp, starts, 7)
        assert (st == 4).sum() > 300 and all(len(p) == 7 for p, s in zip(paths, st) if s == 4)
        _paths_vs_ref(pl, pb, rc, rp, starts[:3], 2)
        if len(shape) == 2:
            # more starts than one chunk of the offsets' scan holds: its carry runs across one and two chunk seams
            many = (lo + np.random.default_rng(12).uniform(-0.08, 1.08, (2049, 2)) * (hi - lo)).astype(F32)
            for m in (1024, 1025, 2049):
                _, _, st = _paths_vs_ref(pl, pb, rc, rp, many[:m], 7)
                assert (st == 4).sum() > m // 5                                               # (the mix of the 1000 above)


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_same_bits_for_every_schedule_stream_and_buffer_history():
    import torch
    import gpismap_amd
    f, shape, origin, step = _serpentine()
    df, dist = _field(f, shape, origin, step)
    goals = _pts([(0, 0), (50, 64)], origin, step)
    pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, goals)
    rounds = {}
    for sched in [(1, 1), (8, 0), (3, 100000), (64, 7)]:
        p2 = gpismap_amd.Planner()
        p2.set_schedule(*sched)
        _solve_vs_ref(df, dist, shape, origin, step, goals, planner=p2)
        rounds[sched] = p2.info()["rounds"]
    assert rounds[(1, 1)] > rounds[(3, 100000)]
    # a caller's stream
    s = torch.cuda.Stream()
    p3 = gpismap_amd.Planner()
    p3.solve(df, goals, stream=s.cuda_stream)
    assert _bits_equal(p3.get()[0].ravel(), rc) and np.array_equal(p3.get()[1].ravel(), rp)
    # twice, then after a larger and a smaller problem on the same planner
    _solve_vs_ref(df, dist, shape, origin, step, goals, planner=pl)
    big = (150, 130)
    dfb, distb = _field(_balls(big, origin, step, [((70.0, 60.0), 20.5)]), big, origin, step)
    _solve_vs_ref(dfb, distb, big, origin, step, goals, planner=pl)
    small = (9, 15, 8)
    dfs, dists = _field(_balls(small, (0.0, 0.0, 0.0), step, [((4.0, 7.0, 4.0), 2.2)]), small, (0.0, 0.0, 0.0), step)
    _solve_vs_ref(dfs, dists, small, (0.0, 0.0, 0.0), step, [[0.0, 0.0, 0.0]], planner=pl)
    _solve_vs_ref(df, dist, shape, origin, step, goals, planner=pl)


def test_plan_outlives_its_field():
    shape, origin, step = (70, 45), (-3.0, 1.0), 0.1
    df, dist = _field(_balls(shape, origin, step, [((30.0, 20.0), 9.4)]), shape, origin, step)
    pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, _pts([(2, 2)], origin, step))
    starts = _pts([(60, 40), (5, 30), (30, 20)], origin, step)
    before = _paths_vs_ref(pl, pb, rc, rp, starts, None)
    _field(_balls((50, 50), origin, step, [((10.0, 10.0), 4.0)]), (50, 50), origin, 0.2, df=df)      # other data, other lattice
    cost, pol = pl.get()
    assert _bits_equal(cost.ravel(), rc) and np.array_equal(pol.ravel(), rp)
    after = _paths_vs_ref(pl, pb, rc, rp, starts, None)
    assert all(_bits_equal(a, b) for a, b in zip(before[0], after[0]))
    df.close()
    assert _bits_equal(pl.get()[0].ravel(), rc)
    _paths_vs_ref(pl, pb, rc, rp, starts, None)


# ---- map level ---------------------------------------------------------------------------------------------------------------
def test_gazebo_map_route():
    """The gazebo map's field on the demo grid, planned with clearance 0 from the first recorded robot position to the last: the
    device against the reference on the device's own dist, and the route the robot drove is found."""
    import gpismap_amd
    frames = replay.load_gazebo()
    gm = gpismap_amd.GPisMap()
    for fr in frames:
        gm.update(fr["thetas"], fr["ranges"], fr["pose"])
    df = gm.distance_field(**BOX2)
    dist = df.get()[0].ravel()
    first, last = frames[0]["pose"][:2], frames[-1]["pose"][:2]
    pl, pb, rc, rp = _solve_vs_ref(df, dist, BOX2["shape"], BOX2["origin"], BOX2["step"][0], last[None], ref="dijkstra",
                                   clearance=0.0)
    paths, sc, st = _paths_vs_ref(pl, pb, rc, rp, first[None], None)
    print("gazebo route: status %d, %d points, cost %.3f, rounds %d, tile launches %d" %
          (st[0], len(paths[0]), sc[0], pl.info()["rounds"], pl.info()["tile_launches"]))
    assert st[0] == 0
    ok, ijk = plan_ref.snap(paths[0], BOX2["shape"], BOX2["origin"], BOX2["step"][0])
    assert ok.all() and np.all(dist.reshape(199, 249)[ijk[:, 1], ijk[:, 0]] >= 0)
    seg = np.diff(paths[0].astype(np.float64), axis=0)
    length = np.sqrt((seg ** 2).sum(1)).sum()
    straight = np.sqrt(((paths[0][-1].astype(np.float64) - paths[0][0]) ** 2).sum())
    assert length >= straight * (1 - 1e-6) and length > 0


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    shape, origin, step = (37, 29), (-3.0, 1.0), 0.1
    df, dist = _field(_balls(shape, origin, step, [((18.0, 14.0), 7.4)]), shape, origin, step)
    goals = _pts([(1, 1)], origin, step)
    pl, pb, rc, rp = _solve_vs_ref(df, dist, shape, origin, step, goals)
    starts = _pts([(35, 27), (2, 20)], origin, step)
    paths0, sc0, st0 = _paths_vs_ref(pl, pb, rc, rp, starts, None)
    off0 = pl.last_off.copy()
    fpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def unchanged():
        cost, pol = pl.get()
        assert _bits_equal(cost.ravel(), rc) and np.array_equal(pol.ravel(), rp)
        m, tot = C.c_longlong(0), C.c_longlong(0)
        assert L.gpis_plan_path_counts(pl.h, C.byref(m), C.byref(tot)) == 0 and (m.value, tot.value) == (2, off0[-1])
        off = np.zeros(3, np.int64)
        pts = np.zeros((off0[-1], 2), F32)
        assert L.gpis_plan_get_paths(pl.h, off.ctypes.data_as(C.POINTER(C.c_longlong)), fpp(pts), None, None) == 0
        assert np.array_equal(off, off0) and _bits_equal(pts, np.concatenate(paths0))

    def solve(plan=None, field=None, g=goals, ng=1, **kw):
        o = gpismap_amd.plan_opts(2, F32(step))
        for k, v in kw.items():
            setattr(o, k, v)
        return L.gpis_plan_solve(pl.h if plan is None else plan, df.h if field is None else field,
                                 fpp(g) if g is not None else None, ng, C.byref(o), None)

    assert L.gpis_plan_solve(None, df.h, fpp(goals), 1, None, None) == -1
    assert L.gpis_plan_solve(pl.h, None, fpp(goals), 1, None, None) == -1
    assert solve(g=None) == -1 and solve(ng=0) == -1 and solve(ng=-4) == -1
    for kw in [dict(margin=-1.0), dict(margin=float("nan")), dict(margin=float("inf")), dict(gain=-0.5), dict(gain=float("nan")),
               dict(gain=float("inf")), dict(gain=10001.0), dict(clearance=float("nan")), dict(clearance=float("inf")),
               dict(clearance=float("-inf")), dict(connectivity=2), dict(connectivity=-1), dict(max_rounds=-1)]:
        assert solve(**kw) == -1, kw
    unchanged()
    empty = gpismap_amd.DistanceField()
    assert solve(field=empty.h) == -3
    assert L.gpis_plan_solve(pl.h, empty.h, fpp(goals), 1, None, None) == -3
    unchanged()
    # paths: argument, limit
    assert L.gpis_plan_paths(None, fpp(starts), 2, 10, None) == -1
    assert L.gpis_plan_paths(pl.h, None, 2, 10, None) == -1
    assert L.gpis_plan_paths(pl.h, fpp(starts), 0, 10, None) == -1
    assert L.gpis_plan_paths(pl.h, fpp(starts), 2, 1, None) == -1
    assert L.gpis_plan_paths(pl.h, fpp(starts), (1 << 24) + 1, 10, None) == -4
    unchanged()
    o = gpismap_amd.gpis_plan_opts()
    assert L.gpis_plan_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_plan_default_opts(2, 0.0, C.byref(o)) == -1
    assert L.gpis_plan_default_opts(2, 0.1, None) == -1 and L.gpis_plan_set_schedule(pl.h, -1, 0) == -1
    assert L.gpis_plan_default_opts(3, 0.5, C.byref(o)) == 0
    assert (o.clearance, o.margin, o.gain, o.connectivity, o.max_rounds) == (0.0, 2.0, 4.0, 1, 0)
    assert L.gpis_plan_info(None, None, 0) == -1 and L.gpis_plan_get(None, None, None) == -1
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.plan_opts(2, 0.1, speed=3)
    # state: nothing solved yet, or solved but no paths
    fresh = gpismap_amd.Planner()
    buf = np.zeros(8, F32)
    assert fresh.info()["valid"] == 0 and L.gpis_plan_get(fresh.h, fpp(buf), None) == -3
    assert L.gpis_plan_paths(fresh.h, fpp(starts), 2, 10, None) == -3
    assert L.gpis_plan_path_counts(fresh.h, None, None) == -3 and L.gpis_plan_get_paths(fresh.h, None, None, None, None) == -3
    fresh.solve(df, goals)
    assert L.gpis_plan_path_counts(fresh.h, None, None) == -3 and L.gpis_plan_get_paths(fresh.h, None, None, None, None) == -3
    # a new solve drops the old paths; after an error the planner works again
    _solve_vs_ref(df, dist, shape, origin, step, goals, planner=pl)
    assert L.gpis_plan_path_counts(pl.h, None, None) == -3
    _paths_vs_ref(pl, pb, rc, rp, starts, None)
    unchanged()
