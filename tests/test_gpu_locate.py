"""Pose-hypothesis scoring on the GPU (csrc/locate.hip, gpis3_locate_depth_field / gpis2_locate_scan_field / gpis_locate_*): the
device call against the numpy reference (tests/locate_ref.py) -- cost as float64 bits, inliers and order exactly -- at kernel
level (analytic f grids through from_grid) at every point count, batch size and stride where the kernel takes another path, and
at map level (a gazebo and a synthetic field); the independence of a pose from its batch and its stream; locate-and-refine
against the composition of the references; the field tracker unchanged by a locate call; the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import dfield_ref
import locate_ref
import replay
import track_field_ref
import track_ref
from test_gpu_dfield import BOX2, SYN
from test_gpu_track import SYN_CAM, SYN_TRUE, _bits_equal, _gazebo_map, _perturb2, _same, _synthetic_map
from test_gpu_track_field import LAT2, LAT3, _grid_field, _lat
from test_locate_ref import MAXR2, TH2, TRUE2, TRUE3, depth3, grid2, grid3, ranges2
from test_track_ref import CAM, OFF2, scene2, scene3

pytestmark = pytest.mark.gpu
F32 = np.float32
_CACHE = {}


def df2():
    if "df2" not in _CACHE:
        _CACHE["df2"] = _grid_field(scene2, LAT2)
        _CACHE["dist2"] = _CACHE["df2"].get()[0].ravel()
    return _CACHE["df2"], _CACHE["dist2"]


def df3():
    if "df3" not in _CACHE:
        _CACHE["df3"] = _grid_field(scene3, LAT3)
        _CACHE["dist3"] = _CACHE["df3"].get()[0].ravel()
    return _CACHE["df3"], _CACHE["dist3"]


def _check(out, ref, what):
    (c, n, o), (rc, rn, ro) = out, ref
    assert c.dtype == np.float64 and n.dtype == np.int32 and o.dtype == np.int32, what
    assert _bits_equal(c, rc), (what, np.flatnonzero(c.view(np.uint64) != rc.view(np.uint64))[:8])
    assert np.array_equal(n, rn), what
    assert np.array_equal(o, ro), what


def _masked(ranges, p, seed=11):
    """The scan with all but p beams (a fixed scattered subset, in order) made invalid."""
    keep = np.sort(np.random.default_rng(seed).permutation(ranges.size)[:p])
    out = np.zeros_like(ranges)
    out[keep] = ranges[keep]
    return out


# ---- bits, kernel level ---------------------------------------------------------------------------------------------------
POINTS2 = (0, 1, 37, 63, 64, 65, 128, 270, 360)
BATCH2 = {1: [187], 3: [5, 187, 1030], 4: [0, 187, 189, 1030], 5: [1030, 77, 187, 400, 2]}


@pytest.mark.parametrize("off2", (OFF2, (0.0, 0.05)))
def test_bits_2d_every_point_count_and_batch_size(off2):
    df, dist = df2()
    shape, origin, step = _lat(df)
    poses = grid2()[:1031]
    for p in POINTS2:
        rg = _masked(ranges2(), p)
        loc, _ = track_ref.points2(TH2, rg, off2)
        assert loc.shape[0] == p
        rc, rn, _ = locate_ref.score(dist, shape, origin, step, loc, poses, MAXR2)
        out = df.score_scan(TH2, rg, poses, off2, max_residual=MAXR2, top_k=16)
        _check(out, (rc, rn, locate_ref.rank(rc, 16)), "2-D p %d m 1031" % p)
        assert df._own_locator().info()["points"] == p
        if p == 0:
            assert np.all(out[0] == 0.0) and np.all(out[1] == 0) and out[2].tolist() == list(range(16))
        for m, sel in BATCH2.items():
            out = df.score_scan(TH2, rg, poses[sel], off2, max_residual=MAXR2, top_k=16)
            _check(out, (rc[sel], rn[sel], locate_ref.rank(rc[sel], 16)), "2-D p %d m %d" % (p, m))
    assert rn.max() == 360 and rn.min() < 100        # (the full scan: poses that fit, poses that do not)


def _edge_pose(loc, lat):
    """An unrotated pose that puts a local point exactly on the lattice's last row, (x - ox) / step == nx - 1 in float32: (pose, the
    world x, the point's index).  Not every point has a float32 translation that lands on that x: the first that has one."""
    nx, ox, st = lat["shape"][0], F32(lat["origin"][0]), F32(lat["step"])
    X = F32(ox + F32(nx - 1) * st)
    for _ in range(64):
        if F32((X - ox) / st) == F32(nx - 1):
            break
        X = np.nextafter(X, F32(-np.inf) if F32((X - ox) / st) > F32(nx - 1) else F32(np.inf))
    assert F32((X - ox) / st) == F32(nx - 1)
    for i in range(loc.shape[0]):
        t0 = F32(X - loc[i, 0])
        for t in (t0, np.nextafter(t0, F32(np.inf)), np.nextafter(t0, F32(-np.inf))):
            if F32(loc[i, 0] + t) == X:
                return np.array([t, F32(0.1) - loc[i, 1], 1.0, 0.0, 0.0, 1.0], F32), X, i
    raise AssertionError("no point reaches the last row")


def test_bits_2d_off_lattice_last_row_duplicates_and_top_k():
    df, dist = df2()
    shape, origin, step = _lat(df)
    loc, _ = track_ref.points2(TH2, ranges2(), OFF2)
    p = loc.shape[0]
    batch = grid2()[:1031].copy()
    far = np.array([100.0, 100.0, 1.0, 0.0, 0.0, 1.0], F32)
    edge, X, ie = _edge_pose(loc, LAT2)
    batch[3], batch[900] = far, far                  # every point outside the lattice, twice
    batch[7] = edge                                  # a point on the last row
    batch[1000], batch[1029] = batch[187], batch[187]    # duplicates at distant batch positions
    w = locate_ref.world_points(loc, edge[None, :], 2)[0]
    assert w[ie, 0] == X and F32((X - F32(origin[0])) / F32(step)) == F32(shape[0] - 1)
    assert np.isfinite(dfield_ref.sample(dist, shape, origin, step, w[ie:ie + 1])[0, 0])
    rc, rn, ro = locate_ref.score(dist, shape, origin, step, loc, batch, MAXR2, top_k=0)
    assert rc[3] == p * MAXR2 * MAXR2 and rn[3] == 0 and rc[900] == rc[3] and rc.max() == rc[3]
    assert rn[7] >= 1 and rc[1000] == rc[187] == rc[1029]
    out = df.score_scan(TH2, ranges2(), batch, OFF2, max_residual=MAXR2, top_k=0)
    _check(out, (rc, rn, ro), "2-D special batch")
    o = out[2].tolist()
    assert o.index(187) + 1 == o.index(1000) and o.index(1000) + 1 == o.index(1029)     # ties by the lower index
    assert o.index(3) < o.index(900) and o[-1] >= 900 and out[0][o[-1]] == rc[3]
    for k in (1, 16, 1031, 5000):
        out = df.score_scan(TH2, ranges2(), batch, OFF2, max_residual=MAXR2, top_k=k)
        _check(out, (rc, rn, ro[:min(k, 1031)]), "top_k %d" % k)
        assert df._own_locator().info()["ranked"] == min(k, 1031)


BATCH3 = {1: [171], 4: [171, 0, 1028, 514]}


@pytest.mark.parametrize("stride", (1, 2, 7))
def test_bits_3d_strides_and_batch_sizes(stride):
    df, dist = df3()
    shape, origin, step = _lat(df)
    poses = grid3()
    assert poses.shape == (1029, 12) and _bits_equal(poses[171], TRUE3)
    loc, _ = track_ref.points3(depth3(), CAM, stride)
    assert loc.shape[0] > 0
    rc, rn, _ = locate_ref.score(dist, shape, origin, step, loc, poses, 0.05)
    out = df.score_depth(depth3(), poses, CAM, stride=stride, top_k=0)
    _check(out, (rc, rn, locate_ref.rank(rc, 0)), "3-D stride %d m 1029" % stride)
    i = df._own_locator().info()
    assert (i["held"], i["dim"], i["poses"], i["points"], i["ranked"], i["pixels"]) == (1, 3, 1029, loc.shape[0], 1029, 4800)
    assert rn.max() > 0.9 * loc.shape[0]
    for m, sel in BATCH3.items():
        out = df.score_depth(depth3(), poses[sel], CAM, stride=stride)
        _check(out, (rc[sel], rn[sel], locate_ref.rank(rc[sel], 16)), "3-D stride %d m %d" % (stride, m))


# ---- independence ---------------------------------------------------------------------------------------------------------
def _call2(L, map_h, df, loc, thetas, ranges, poses, off2=None, stream=None, n=None, m=None, **kw):
    import gpismap_amd
    P = lambda a: None if a is None else np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    o = gpismap_amd.locate_opts(2, **kw)
    poses = None if poses is None else np.ascontiguousarray(poses, F32)
    return L.gpis2_locate_scan_field(map_h, df.h if df is not None else None, loc.h if loc is not None else None, P(thetas),
                                     P(ranges), len(thetas) if n is None else n, P(off2), P(poses),
                                     (poses.size // 6 if m is None else m), C.byref(o), stream)


def _call3(L, map_h, df, loc, depth, poses, cam6=None, stream=None, m=None, **kw):
    import gpismap_amd
    P = lambda a: None if a is None else np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    o = gpismap_amd.locate_opts(3, **kw)
    c = C.byref(gpismap_amd._cam(cam6)) if cam6 is not None else None
    poses = None if poses is None else np.ascontiguousarray(poses, F32)
    return L.gpis3_locate_depth_field(map_h, df.h if df is not None else None, loc.h if loc is not None else None, c, P(depth),
                                      P(poses), (poses.size // 12 if m is None else m), C.byref(o), stream)


def test_a_pose_does_not_depend_on_its_batch_or_stream():
    import gpismap_amd
    import torch
    L = gpismap_amd.lib()
    df, dist = df2()
    poses = grid2()[:1031].copy()
    q = poses[187].copy()
    alone = df.score_scan(TH2, ranges2(), q[None, :], OFF2)
    three = df.score_scan(TH2, ranges2(), np.stack([poses[0], poses[1], q]), OFF2)
    poses[1030] = q
    many = df.score_scan(TH2, ranges2(), poses, OFF2)
    assert alone[1][0] == 360 and alone[0][0] > 0
    assert _bits_equal(alone[0][:1], three[0][2:3]) and _bits_equal(alone[0][:1], many[0][1030:]) and _bits_equal(alone[0][:1], many[0][187:188])
    assert alone[1][0] == three[1][2] == many[1][1030]
    # two calls on two streams
    res = []
    for _ in range(2):
        s = torch.cuda.Stream(device=0)
        l = gpismap_amd.Locator()
        assert _call2(L, None, df, l, TH2, ranges2(), poses, off2=np.array(OFF2, F32), stream=C.c_void_p(s.cuda_stream)) == 0
        res.append(l.get())
    for r in res:
        _check(r, many, "stream")


# ---- map level --------------------------------------------------------------------------------------------------------------
def _gz():
    if "gz" not in _CACHE:
        g2, f2 = _gazebo_map()
        _CACHE["gz"] = (g2, f2, g2.distance_field(**BOX2))
    return _CACHE["gz"]


def test_bits_map_level():
    import gpismap_amd
    g2, f2, dfg = _gz()
    shape, origin, step = _lat(dfg)
    fr = f2[len(f2) // 2]
    x, y, th = float(fr["pose"][0]), float(fr["pose"][1]), math.atan2(float(fr["pose"][3]), float(fr["pose"][2]))
    d = np.array([-0.3, -0.1, 0.1, 0.3])
    poses = gpismap_amd.pose_grid2(x + d, y + d, th + np.radians([-6.0, -2.0, 2.0, 6.0]))
    assert poses.shape == (64, 6)
    out = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], poses, top_k=0)
    ref = locate_ref.score_scan(dfg.get()[0].ravel(), shape, origin, step, fr["thetas"], fr["ranges"], poses, OFF2, top_k=0)
    _check(out, ref, "gazebo field")
    assert out[1].max() > 20
    gm = _synthetic_map()
    dfs = gm.distance_field(**SYN)
    shape, origin, step = _lat(dfs)
    depth, _, _ = gm.render_depth(SYN_TRUE, cam6=SYN_CAM)
    a = np.array([-0.03, -0.01, 0.01, 0.03])
    off = np.stack([a.repeat(4), np.tile(a, 4), np.tile(a[::-1], 4)], axis=1)
    poses = gpismap_amd.pose_grid3(SYN_TRUE, off, [(0, 0, 0), (0.01, 0, 0), (0, -0.02, 0), (0, 0, 0.03)])
    assert poses.shape == (64, 12)
    out = gm.score_depth_field(dfs, depth, poses, cam6=SYN_CAM)
    ref = locate_ref.score_depth(dfs.get()[0].ravel(), shape, origin, step, depth, SYN_CAM, poses)
    _check(out, ref, "synthetic field")
    assert out[1].max() > 500
    # the map's own camera when the caller passes none
    d640 = replay.synthetic_depth(1)
    _check(gm.score_depth_field(dfs, d640, poses[:4]), dfs.score_depth(d640, poses[:4], (568.0, 568.0, 310.0, 224.0, 640, 480)), "map camera")


# ---- locate and refine ------------------------------------------------------------------------------------------------------
def test_locate_and_refine_is_the_composition_of_the_references():
    df, dist = df2()
    shape, origin, step = _lat(df)
    poses = grid2()
    loc, _ = track_ref.points2(TH2, ranges2(), OFF2)

    def track_fn(p0):
        return track_field_ref.track_scan(dist, shape, origin, step, TH2, ranges2(), p0, OFF2)
    rp, ri = locate_ref.locate(dist, shape, origin, step, loc, poses, track_fn, refine=8, max_residual=MAXR2, top_k=16)
    pose, info = df.locate_scan(TH2, ranges2(), poses, OFF2, refine=8, max_residual=MAXR2, top_k=16)
    _check((info["cost"], info["inliers"], info["order"]), (ri["cost"], ri["inliers"], ri["order"]), "first ranking")
    assert np.array_equal(info["candidates"], ri["candidates"]) and len(info["tracks"]) == 8
    for t, r in zip(info["tracks"], ri["tracks"]):
        assert (t["status"], t["iterations"], t["inliers"]) == (r["status"], r["iterations"], r["inliers"])
    assert _bits_equal(info["refined"], ri["refined"])
    assert _bits_equal(info["refined_cost"], ri["refined_cost"]) and np.array_equal(info["refined_inliers"], ri["refined_inliers"])
    assert info["best"] == ri["best"] and _bits_equal(pose, rp)
    assert info["tracks"][info["best"]]["status"] == 0
    assert math.hypot(float(pose[0]) - float(TRUE2[0]), float(pose[1]) - float(TRUE2[1])) < 0.5 * LAT2["step"]
    p0, i0 = df.locate_scan(TH2, ranges2(), poses, OFF2, refine=0, max_residual=MAXR2)
    assert _bits_equal(p0, poses[ri["order"][0]]) and i0["tracks"] == []


# ---- the trackers ---------------------------------------------------------------------------------------------------------
def test_field_tracker_unchanged_by_a_locate_call():
    import gpismap_amd
    g2, f2, dfg = _gz()
    fr = f2[5]
    start = _perturb2(fr["pose"], 0.05, 1.0)
    t = gpismap_amd.Tracker()
    before = g2.track_scan_field(dfg, fr["thetas"], fr["ranges"], start, tracker=t)
    poses = np.stack([start, fr["pose"], _perturb2(fr["pose"], 0.2, 4.0)])
    first = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], poses)
    after = g2.track_scan_field(dfg, fr["thetas"], fr["ranges"], start, tracker=t)
    again = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], poses)
    assert before[1]["inliers"] > 20 and _same(before, after)
    _check(again, first, "locate after track")


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    df, _ = df2()
    d3, _ = df3()
    nores = gpismap_amd.DistanceField()
    off = np.array(OFF2, F32)
    poses = grid2()[:5]
    rg = ranges2()
    l = gpismap_amd.Locator()
    assert L.gpis_locate_get(l.h, None, None, None) == -3 and L.gpis_locate_device(l.h, None, None) == -3     # before any call
    assert l.info()["held"] == 0
    with pytest.raises(gpismap_amd.GpisError):
        l.get()
    assert _call2(L, None, df, l, TH2, rg, poses, off2=off) == 0
    a, ia, pa = l.get(), l.info(), l.device_ptrs()
    assert pa[0] != 0 and pa[1] == pa[0] + 8 * 5

    def still_there(what):
        b = l.get()
        assert l.info() == ia and l.device_ptrs() == pa, what
        _check(b, a, what)

    bad_th = TH2.copy(); bad_th[2] = np.nan
    bad_p = poses.copy(); bad_p[4, 3] = np.inf
    arg = dict(no_field=dict(df=None), no_thetas=dict(thetas=None), no_ranges=dict(ranges=None), no_poses=dict(poses=None, m=5),
               no_offset=dict(off2=None), n0=dict(n=0), m0=dict(m=0), m_neg=dict(m=-1), stride0=dict(stride=0), topk=dict(top_k=-1),
               r_neg=dict(max_residual=-1.0), r_nan=dict(max_residual=np.nan), r_inf=dict(max_residual=np.inf),
               theta=dict(thetas=bad_th), pose=dict(poses=bad_p), off_nan=dict(off2=np.array([np.nan, 0.0], F32)),
               dim=dict(df=d3))
    for name, kw in arg.items():
        args = dict(df=df, thetas=TH2, ranges=rg, poses=poses, off2=off)
        args.update(kw)
        f, th, r, p = args.pop("df"), args.pop("thetas"), args.pop("ranges"), args.pop("poses")
        n = args.pop("n", len(TH2))
        assert _call2(L, None, f, l, th, r, p, n=n, **args) == -1, name
        still_there(name)
    assert _call2(L, None, df, None, TH2, rg, poses, off2=off) == -1                       # no locator
    assert _call2(L, None, nores, l, TH2, rg, poses, off2=off) == -3
    still_there("no result in the field")
    # the limits: refused before anything is read past the small arrays or allocated
    assert _call2(L, None, df, l, TH2, rg, poses, off2=off, n=(1 << 26) + 1) == -4
    still_there("beams")
    assert _call2(L, None, df, l, TH2, rg, poses, off2=off, m=(1 << 24) + 1) == -4
    still_there("poses")
    # 3-D
    l3 = gpismap_amd.Locator()
    p3 = grid3()[:4]
    assert _call3(L, None, d3, l3, depth3(), p3, cam6=CAM) == 0
    a3, i3, q3 = l3.get(), l3.info(), l3.device_ptrs()

    def still3(what):
        assert l3.info() == i3 and l3.device_ptrs() == q3, what
        _check(l3.get(), a3, what)

    bad3 = p3.copy(); bad3[1, 7] = np.nan
    for name, kw in dict(no_cam=dict(cam6=None), bad_cam=dict(cam6=(0.0, 50.0, 39.5, 29.5, 80, 60)), size=dict(cam6=(50.0, 50.0, 39.5, 29.5, 0, 60)),
                         no_depth=dict(depth=None), stride0=dict(stride=0), pose=dict(poses=bad3), m0=dict(m=0),
                         r_nan=dict(max_residual=np.nan), dim=dict(df=df), no_field=dict(df=None)).items():
        args = dict(df=d3, depth=depth3(), poses=p3, cam6=CAM)
        args.update(kw)
        f, d, p = args.pop("df"), args.pop("depth"), args.pop("poses")
        assert _call3(L, None, f, l3, d, p, **args) == -1, name
        still3(name)
    assert _call3(L, None, nores, l3, depth3(), p3, cam6=CAM) == -3
    still3("no result in the field")
    assert _call3(L, None, d3, l3, depth3(), p3, cam6=(50.0, 50.0, 39.5, 29.5, 8193, 8192)) == -4
    still3("pixels")
    assert _call3(L, None, d3, l3, depth3(), p3, cam6=CAM, m=(1 << 24) + 1) == -4
    still3("poses")
    with pytest.raises(gpismap_amd.GpisError):
        d3.score_depth(depth3()[:-1], p3, CAM)
    with pytest.raises(gpismap_amd.GpisError):
        df.score_scan(TH2, rg, poses[:, :5], OFF2)
    with pytest.raises(gpismap_amd.GpisError):
        df.score_scan(TH2, rg, poses, OFF2, huber=1.0)
    # after the errors the locators work again; a 2-D locator takes a 3-D call
    assert _call2(L, None, df, l, TH2, rg, poses, off2=off) == 0
    _check(l.get(), a, "again")
    assert _call3(L, None, d3, l, depth3(), p3, cam6=CAM) == 0
    _check(l.get(), a3, "a 3-D call on the 2-D locator")
