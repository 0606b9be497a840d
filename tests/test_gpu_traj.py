"""Trajectory smoothing on the GPU (csrc/traj.hip, gpis_traj_*): resampling, descent and evaluation against the numpy reference
(tests/traj_ref.py) on the device's own dist, bit for bit -- every sum has one order, so there are no tolerances -- at every
wavefront edge of N, for every option, for planner and caller inputs, and the error paths."""
import ctypes as C
import functools

import numpy as np
import pytest

import replay
import traj_cases
import traj_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
KEYS = ("x", "status", "iterations", "length", "smooth", "obstacle", "min_dist", "nonfinite", "collides")


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _field(f, shape, origin, step, df=None):
    import gpismap_amd
    df = df if df is not None else gpismap_amd.DistanceField()
    t = _dev(np.ascontiguousarray(f, F32).ravel())
    df.from_grid(t.data_ptr(), shape, origin, step, 0.0)
    return df, df.get()[0].ravel()


def _equal(got, ref, what=""):
    for k in KEYS:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype)
        if u.dtype == F32:
            u, v = u.view(U32), v.view(U32)
        assert np.array_equal(u, v), (what, k, np.flatnonzero((u != v).reshape(u.shape[0], -1).any(axis=1))[:8])


@functools.lru_cache(maxsize=None)
def _scene(dim):
    """(scene, field, its dist, planner with the scene's paths, the reference's packed paths)."""
    import gpismap_amd
    sc = traj_cases.scene(dim)
    df, dist = _field(sc["f"], sc["shape"], sc["origin"], sc["step"])
    pl = df.plan([traj_cases.world(sc, sc["goal"])], planner=gpismap_amd.Planner(), clearance=0.0, margin=4 * sc["step"], gain=4.0)
    paths, scost, st = pl.paths(traj_cases.starts(sc))
    off = pl.last_off.copy()
    pts = np.concatenate(paths) if off[-1] else np.zeros((0, dim), F32)
    return sc, df, dist, pl, (off, pts, st)


def _opts(sc, **kw):
    import gpismap_amd
    o = gpismap_amd.traj_opts(len(sc["shape"]), F32(sc["step"]), **kw)
    return {k: getattr(o, k) for k in traj_ref.OPT_NAMES}


def _ref(sc, dist, x, ist, **kw):
    return traj_ref.optimize(dist, sc["shape"], sc["origin"], sc["step"], x, ist, _opts(sc, **kw))


@functools.lru_cache(maxsize=None)
def _status_scene(dim):
    """(scene with a shell, field, its dist, planner solved towards the scene's goal)."""
    import gpismap_amd
    sc = traj_cases.status_scene(dim)
    df, dist = _field(sc["f"], sc["shape"], sc["origin"], sc["step"])
    pl = df.plan([traj_cases.world(sc, sc["goal"])], planner=gpismap_amd.Planner(), clearance=0.0, margin=4 * sc["step"], gain=4.0)
    return sc, df, dist, pl


def _packed(pl, paths, st, dim):
    off = pl.last_off.copy()
    return off, (np.concatenate(paths) if off[-1] else np.zeros((0, dim), F32)), st


# ---- waypoint counts and inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_from_paths_every_status_and_waypoint_count(dim):
    """Planner paths with every status -- 0, a path of one point, 1 (outside, NaN), 2 (inside a ball), 3 (enclosed by a shell) and,
    in a second batch cut at max_points, 4 (points kept, yet no input) -- resampled on the device to every N around the wavefront
    edges: the waypoints (iters = 0) and two iterations against the reference."""
    import gpismap_amd
    sc, df, dist, pl = _status_scene(dim)
    starts = traj_cases.status_starts(sc)
    tj = gpismap_amd.Trajectories()
    batches = []
    for max_points in (None, traj_cases.CUT):
        paths, scost, st = pl.paths(starts, max_points=max_points)
        off, pts, st = _packed(pl, paths, st, dim)
        batches.append((off, pts, st))
        for N in traj_cases.NS:
            x, ist = traj_ref.resample(off, pts, st, N)
            assert np.array_equal(ist == 0, st == 0)
            for iters in (0, 2):
                assert df.smooth(pl, N=N, trajectories=tj, iters=iters) is tj
                got = tj.get()
                ref = _ref(sc, dist, x, ist, iters=iters)
                _equal(got, ref, (dim, max_points, N, iters))
                if iters == 0:
                    assert np.array_equal(got["x"].view(U32), x.view(U32)) and np.all(got["iterations"] == 0)
            bad = st != 0
            assert np.all(got["status"][bad] == 2) and np.all(np.isnan(got["x"][bad])) and np.all(np.isnan(got["min_dist"][bad]))
            assert not got["nonfinite"][bad].any() and not got["collides"][bad].any() and np.all(got["status"][~bad] <= 1)
            inf = tj.info()
            assert (inf["input"], inf["valid"], inf["m"], inf["N"], inf["dim"]) == (1, 1, len(st), N, dim)
    traj_cases.check_status_paths(batches)


def test_segment_search_on_a_lattice_of_inexact_coordinates():
    """Lattice origin -0.05, step 0.1: waypoints land exactly on path points whose neighbours' difference rounds, so a search by <
    instead of <= would change bits.  The device equals the reference, and the reference differs from that variant here."""
    import gpismap_amd
    sc = traj_cases.offgrid_scene()
    df, dist = _field(sc["f"], sc["shape"], sc["origin"], sc["step"])
    pl = df.plan([traj_cases.world(sc, sc["goal"])], planner=gpismap_amd.Planner(), clearance=0.0, margin=4 * sc["step"], gain=4.0)
    paths, scost, st = pl.paths(np.stack([traj_cases.world(sc, c) for c in traj_cases.OFFGRID_STARTS]))
    off, pts, st = _packed(pl, paths, st, 2)
    assert np.all(st == 0)
    for N in traj_cases.OFFGRID_NS:
        x, ist = traj_ref.resample(off, pts, st, N)
        lt, _ = traj_ref.resample(off, pts, st, N, variant="search_lt")
        assert (x.view(U32) != lt.view(U32)).any(), N
        got = df.smooth(pl, N=N, iters=0).get()
        assert np.array_equal(got["x"].view(U32), x.view(U32)), N
        _equal(got, _ref(sc, dist, x, ist, iters=0), N)


@pytest.mark.parametrize("dim", [2, 3])
def test_default_iterations_mix_early_and_capped(dim):
    sc, df, dist, pl, (off, pts, st) = _scene(dim)
    tj = pl.trajectories(64)
    got = tj.optimize(df).get()
    x, ist = traj_ref.resample(off, pts, st, 64)
    ref = _ref(sc, dist, x, ist)
    _equal(got, ref, dim)
    ok = ist == 0
    assert (got["status"][ok] == 0).sum() >= 3 and (got["status"][ok] == 1).sum() >= 3 and np.all(got["status"][~ok] == 2)
    assert np.all(np.isnan(got["x"][~ok])) and np.all(np.isnan(got["length"][~ok])) and np.all(got["collides"][~ok] == 0)
    # iters = 1 from the same input; the input is kept, so the call order does not matter
    _equal(tj.optimize(df, iters=1).get(), _ref(sc, dist, x, ist, iters=1), "iters=1")
    _equal(tj.optimize(df).get(), ref, "again")


@pytest.mark.parametrize("dim", [2, 3])
def test_hand_made_waypoints_and_batch_sizes(dim):
    """Caller waypoints that reach every branch (outside the lattice, the last cell, inside an obstacle, the trust region, e
    exactly 0 and margin, a NaN trajectory) for m = 7, m = 1 and m = 600 (more workgroups than CUs), sub = 0, 1, 16."""
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(dim)
    tj = gpismap_amd.Trajectories()
    for N in (3, 64, 65, 256):
        hx, hopts, names = traj_cases.hand_made(sc, dist, N)
        for sub, iters in ((0, 5), (1, 0), (16, 3)):
            got = df.smooth(hx, trajectories=tj, iters=iters, sub=sub, **hopts).get()
            ref = _ref(sc, dist, hx, None, iters=iters, sub=sub, **hopts)
            _equal(got, ref, (dim, N, sub))
        k = names.index("nan")
        assert got["status"][k] == 2 and np.array_equal(got["x"][k].view(U32), hx[k].view(U32))
        assert got["nonfinite"][names.index("leaves")] > 0 and got["collides"][names.index("through")] == 1
    hx, hopts, names = traj_cases.hand_made(sc, dist, 64)
    _equal(df.smooth(hx[4:5], trajectories=tj, iters=4, **hopts).get(), _ref(sc, dist, hx[4:5], None, iters=4, **hopts), "m=1")
    rng = np.random.default_rng(5)
    big = np.repeat(hx[:6], 100, axis=0)
    big[:, 1:-1] += rng.normal(0, 0.3 * sc["step"], big[:, 1:-1].shape).astype(F32)
    _equal(df.smooth(big, trajectories=tj, iters=3, **hopts).get(), _ref(sc, dist, big, None, iters=3, **hopts), "m=600")
    # a smaller batch on the grown buffers
    _equal(df.smooth(hx, trajectories=tj, iters=2, **hopts).get(), _ref(sc, dist, hx, None, iters=2, **hopts), "shrunk")


def test_field_without_sites_and_planes():
    import gpismap_amd
    shape, origin, step = (40, 23), (0.0, 0.0), 0.5
    sc = dict(shape=shape, origin=origin, step=step, bl=[((20.0, 11.0), 3.0)])
    df, dist = _field(np.ones(23 * 40, F32), shape, origin, step)
    assert np.all(dist == np.inf)
    hx, _, _ = traj_cases.hand_made(sc, traj_cases.balls(shape, step, sc["bl"]), 33)
    got = df.smooth(hx, trajectories=gpismap_amd.Trajectories(), iters=3).get()
    _equal(got, _ref(sc, dist, hx, None, iters=3), "no sites")
    assert np.all(got["collides"] == 0) and got["min_dist"][0] == np.inf and got["nonfinite"][0] > 0
    # a plane x = 6.2 cells: the distance field of a half space
    g = np.arange(shape[0], dtype=np.float64)[None, :] - 6.2 + np.zeros((shape[1], 1))
    df2, dist2 = _field((g * step).astype(F32).ravel(), shape, origin, step)
    got = df2.smooth(hx, trajectories=gpismap_amd.Trajectories()).get()
    _equal(got, _ref(sc, dist2, hx, None), "plane")


@pytest.mark.parametrize("N", [5, 70])
def test_overflowing_step_stays_nan(N):
    """Finite waypoints whose a_i overflows: the metric row meets inf - inf, the largest step R is NaN as numpy's max gives it, so
    no stop by tol: status 1 after every iteration, NaN waypoints.  Only here the comparison is not of bits: a NaN's sign and
    payload are not part of the contract.  The finite trajectory beside it keeps its bits."""
    import gpismap_amd
    sc, df, dist, pl, _ = _scene(2)
    x = np.zeros((2, N, 2), F32)
    x[:, :, 0] = np.linspace(0, 1, N)
    x[0, 1:-1:2, 1], x[0, 2:-1:2, 1] = 3e38, -3e38
    got = df.smooth(x, trajectories=gpismap_amd.Trajectories(), iters=4).get()
    ref = _ref(sc, dist, x, None, iters=4)
    assert ref["status"][0] == 1 and ref["iterations"][0] == 4 and np.all(np.isnan(ref["x"][0, 1:-1]))
    for k in KEYS:
        assert np.array_equal(got[k], ref[k], equal_nan=got[k].dtype == F32), k
    _equal({k: got[k][1:] for k in KEYS}, {k: ref[k][1:] for k in KEYS}, "finite")


# ---- options -------------------------------------------------------------------------------------------------------------------
def test_every_option_off_its_default_and_exact_thresholds():
    import gpismap_amd
    sc, df, dist, pl, (off, pts, st) = _scene(2)
    step = F32(sc["step"])
    tj = pl.trajectories(33)
    x, ist = traj_ref.resample(off, pts, st, 33)
    base = tj.optimize(df, iters=6).get()
    for kw in [dict(clearance=step), dict(margin=F32(5) * step), dict(w_smooth=0.5), dict(w_obs=step), dict(rate=0.3),
               dict(max_move=F32(0.01) * step), dict(tol=F32(0.2) * step), dict(sub=7), dict(w_obs=0.0), dict(rate=0.0)]:
        got = tj.optimize(df, iters=6, **kw).get()
        _equal(got, _ref(sc, dist, x, ist, iters=6, **kw), kw)
        assert any(not np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(base[k]).view(np.uint8))
                   for k in KEYS), kw
    # exact thresholds from representable numbers: one interior point displaced by 1 along y from a straight line in free space.
    # a_1 = (0, 2), delta_1 = (1 * 1 * 2) / 2 = (0, 1), R = 1.  rate * R == max_move: kappa = rate, no division.
    line = np.array([[[0.0, 8.0], [1.0, 9.0], [2.0, 8.0]]], F32) + F32([-2.0, 1.0])
    free = dict(w_obs=0.0, w_smooth=1.0)
    for rate, mm, tol, want_status in [(0.25, 0.25, 0.25, 1), (0.25, 0.25, 0.2500001, 0), (0.5, 0.25, 0.25, 1), (0.5, 0.25, 0.26, 0)]:
        kw = dict(free, rate=rate, max_move=mm, tol=tol, iters=1)
        got = df.smooth(line, trajectories=tj, **kw).get()
        _equal(got, traj_ref.optimize(dist, sc["shape"], sc["origin"], sc["step"], line, None, _opts(sc, **kw)), kw)
        assert got["status"][0] == want_status and got["x"][0, 1, 1] == F32(10.0) - F32(0.25), (kw, got["x"][0, 1])


# ---- handles, streams, lifetime ------------------------------------------------------------------------------------------------
def test_caller_stream_and_result_outlives_field_and_planner():
    import torch
    import gpismap_amd
    sc = traj_cases.scene(2)
    df, dist = _field(sc["f"], sc["shape"], sc["origin"], sc["step"])
    pl = df.plan([traj_cases.world(sc, sc["goal"])], planner=gpismap_amd.Planner(), clearance=0.0, margin=4 * sc["step"])
    paths, scost, st = pl.paths(traj_cases.starts(sc))
    off, pts = pl.last_off.copy(), np.concatenate(paths)
    x, ist = traj_ref.resample(off, pts, st, 48)
    ref = _ref(sc, dist, x, ist, iters=8)
    s = torch.cuda.Stream()
    tj = pl.trajectories(48)
    _equal(tj.optimize(df, stream=s.cuda_stream, iters=8).get(), ref, "stream")
    assert all(tj.device_ptrs())
    pl.close()
    df.from_grid(_dev(np.ones(20 * 20, F32)).data_ptr(), (20, 20), (0.0, 0.0), 0.1, 0.0)
    _equal(tj.get(), ref, "after the planner and another field")
    df.close()
    _equal(tj.get(), ref, "after the field")


def test_gazebo_map_route_smoothed():
    """The gazebo map's route of test_gpu_plan.py::test_gazebo_map_route, smoothed with the default options: bits equal to the
    reference on the device's own dist, no collision, shorter than the lattice path."""
    import gpismap_amd
    from test_gpu_plan import BOX2
    frames = replay.load_gazebo()
    gm = gpismap_amd.GPisMap()
    for fr in frames:
        gm.update(fr["thetas"], fr["ranges"], fr["pose"])
    df = gm.distance_field(**BOX2)
    dist = df.get()[0].ravel()
    first, last = frames[0]["pose"][:2], frames[-1]["pose"][:2]
    pl = df.plan(last[None], clearance=0.0)
    paths, sc0, st = pl.paths(first[None])
    assert st[0] == 0
    got = df.smooth(pl, N=64).get()
    x, ist = traj_ref.resample(pl.last_off, paths[0], st, 64)
    ref = traj_ref.optimize(dist, BOX2["shape"], BOX2["origin"], BOX2["step"][0], x, ist)
    _equal(got, ref, "gazebo")
    plen = np.sqrt((np.diff(paths[0].astype(np.float64), axis=0) ** 2).sum(1)).sum()
    print("gazebo route smoothed: status %d, %d iterations, length %.3f (lattice path %.3f), min_dist %.3f" %
          (got["status"][0], got["iterations"][0], got["length"][0], plen, got["min_dist"][0]))
    assert got["collides"][0] == 0 and got["length"][0] < plen


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    sc, df, dist, pl, (off, pts, st) = _scene(2)
    tj = pl.trajectories(20)
    x, ist = traj_ref.resample(off, pts, st, 20)
    ref = _ref(sc, dist, x, ist, iters=4)
    _equal(tj.optimize(df, iters=4).get(), ref, "first")
    fpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    hx = np.zeros((2, 5, 2), F32)

    def opt(traj=None, field=None, **kw):
        o = gpismap_amd.traj_opts(2, F32(sc["step"]), iters=4)
        for k, v in kw.items():
            setattr(o, k, v)
        return L.gpis_traj_optimize(tj.h if traj is None else traj, df.h if field is None else field, C.byref(o), None)

    nan, inf = float("nan"), float("inf")
    for kw in [dict(margin=0.0), dict(margin=-1.0), dict(margin=nan), dict(margin=inf), dict(clearance=nan), dict(clearance=inf),
               dict(w_smooth=-1.0), dict(w_smooth=nan), dict(w_obs=-1.0), dict(w_obs=inf), dict(rate=-0.1), dict(rate=nan),
               dict(max_move=-1.0), dict(max_move=inf), dict(tol=-1.0), dict(tol=nan), dict(iters=-1), dict(sub=-1), dict(sub=17)]:
        assert opt(**kw) == -1, kw
    assert L.gpis_traj_optimize(None, df.h, None, None) == -1 and L.gpis_traj_optimize(tj.h, None, None, None) == -1
    sc3, df3, _, _, _ = _scene(3)
    assert opt(field=df3.h) == -1                        # a field of another dim
    empty = gpismap_amd.DistanceField()
    assert opt(field=empty.h) == -3 and L.gpis_traj_optimize(tj.h, empty.h, None, None) == -3
    for N in (2, 257, 0, -1):
        assert L.gpis_traj_from_paths(tj.h, pl.h, N) == -1 and L.gpis_traj_set(tj.h, fpp(hx), 2, N, 2) == -1
    assert L.gpis_traj_from_paths(tj.h, None, 8) == -1 and L.gpis_traj_set(tj.h, None, 2, 5, 2) == -1
    assert L.gpis_traj_set(tj.h, fpp(hx), 0, 5, 2) == -1 and L.gpis_traj_set(tj.h, fpp(hx), 2, 5, 4) == -1
    assert L.gpis_traj_set(tj.h, fpp(hx), (1 << 20) + 1, 5, 2) == -4
    fresh_pl = gpismap_amd.Planner()
    assert L.gpis_traj_from_paths(tj.h, fresh_pl.h, 8) == -3
    fresh_pl.solve(df, [traj_cases.world(sc, sc["goal"])])
    assert L.gpis_traj_from_paths(tj.h, fresh_pl.h, 8) == -3                     # solved, but no paths
    _equal(tj.get(), ref, "after the errors")
    inf0 = tj.info()
    assert (inf0["input"], inf0["valid"], inf0["m"], inf0["N"]) == (1, 1, len(st), 20)
    # state: nothing set, or an input without a result
    fresh = gpismap_amd.Trajectories()
    assert fresh.info()["input"] == 0 and opt(traj=fresh.h) == -3 and fresh.device_ptrs() == (0, 0, 0)
    assert L.gpis_traj_get(fresh.h, *[None] * 9) == -3
    fresh.set(hx)
    assert fresh.info()["valid"] == 0 and L.gpis_traj_get(fresh.h, *[None] * 9) == -3
    with pytest.raises(gpismap_amd.GpisError):
        fresh.get()
    # after the errors the handle works again
    _equal(tj.optimize(df, iters=4).get(), ref, "again")
