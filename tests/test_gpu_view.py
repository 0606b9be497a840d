"""Candidate viewpoints scored on the GPU (csrc/view.hip, gpis*_view_gain_*) against the numpy reference (tests/view_ref.py), against
the library's own single-pose entries (render_*_field, then integrate into a scratch Coverage), and against themselves (batch
position, calls, streams).  Every result is an integer or a float32 taken from one march, so every comparison is for equality.
The reference runs on the device's own dist grid."""
import ctypes as C
import math

import numpy as np
import pytest

import cover_ref
import plan_ref
import view_ref
from test_gpu_cover import _cover, _free, _seen2_first, df2, df3
from test_gpu_plan import _balls, _bits_equal, _field
from test_gpu_track_field import _lat
from test_locate_ref import TH2, TRUE2, TRUE3, depth3
from test_track_ref import CAM, OFF2, pose6, pose12, rot
from test_view_ref import OUTSIDE2, OUTSIDE3, WALL2, YAWS8, candidates2

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = 64                                                # csrc/view.h: poses staged at a time by the gather
SMALL2 = dict(shape=(60, 40), origin=(-0.6, -0.4), step=0.02)
SMALL3 = dict(shape=(24, 20, 16), origin=(-0.6, -0.5, 0.3), step=0.05)
CAM13 = (10.0, 10.0, 6.0, 3.0, 13, 7)                    # 2 x 1 tiles of 8 x 8 pixels, both hanging over the image
TH90 = TH2[::4]
GAP5 = math.radians(5.0)                                 # (TH90's beams are 4 degrees apart)
_CACHE = {}


def small2():
    """A ball on a small 2-D lattice: (field, dist)."""
    if "s2" not in _CACHE:
        _CACHE["s2"] = _field(_balls(SMALL2["shape"], SMALL2["origin"], SMALL2["step"], [((40.0, 20.0), 6.0)]), **SMALL2)
    return _CACHE["s2"]


def small3():
    if "s3" not in _CACHE:
        _CACHE["s3"] = _field(_balls(SMALL3["shape"], SMALL3["origin"], SMALL3["step"], [((12.0, 10.0, 10.0), 3.0)]), **SMALL3)
    return _CACHE["s3"]


def poses2(m, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([pose6(rng.uniform(-3, 3), (rng.uniform(-0.5, 0.1), rng.uniform(-0.35, 0.35))) for _ in range(m)])


def poses3(m, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([pose12(rot(rng.normal(size=3), rng.uniform(0, 0.3)), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2),
                                                                                     rng.uniform(-0.35, -0.15)])) for _ in range(m)])


def half_seen(n, seed=3):
    return np.random.default_rng(seed).random(n) < 0.5


def _scorer():
    import gpismap_amd
    return gpismap_amd.ViewScorer()


def _check(df, dist, seen, sensor, poses, cv=None, v=None, stream=None, pred_of=None, **opts):
    """One call on the device against the reference on the same mask and the device's own dist: gain, hits and every (or the
    listed) predicted measurement, bit for bit; the holder's counters."""
    shape, origin, step = _lat(df)
    dim = len(shape)
    cv = cv if cv is not None else _cover(df).set(seen)
    v = v if v is not None else _scorer()
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 12 if dim == 3 else 6)
    if dim == 3:
        gain, hits = df.view_gain_depth(cv, sensor, poses, scorer=v, stream=stream, **opts)
        rg, rh, rp = view_ref.gain_depth(dist, seen, shape, origin, step, sensor, poses, **opts)
    else:
        gain, hits = df.view_gain_scan(cv, sensor[0], poses, sensor[1], scorer=v, stream=stream, **opts)
        rg, rh, rp = view_ref.gain_scan(dist, seen, shape, origin, step, sensor[0], sensor[1], poses, **opts)
    print("dim %d m %d: gain %s hits %s" % (dim, len(poses), rg[:8].tolist(), rh[:8].tolist()))
    assert gain.dtype == np.int64 and hits.dtype == np.int32
    assert np.array_equal(hits, rh), (hits[:8], rh[:8])
    for k in (range(len(poses)) if pred_of is None else pred_of):
        assert _bits_equal(v.predicted(k), rp[k]), k
    assert np.array_equal(gain, rg), (gain[:8], rg[:8])
    inf = v.info()
    import gpismap_amd
    o = gpismap_amd.view_opts(dim, step, **opts)
    assert inf["valid"] == 1 and inf["dim"] == dim and inf["poses"] == len(poses) and inf["rays"] == rp.shape[1]
    assert inf["targets"] == int(view_ref.targets(seen, dist, o.min_dist).sum()) and inf["samples"] >= 0
    assert np.array_equal(v.gain(), rg) and np.array_equal(v.hits(), rh)
    return rg, rh, rp


# ---- A. against the reference -------------------------------------------------------------------------------------------------
def test_pillar_scene_candidates_2d():
    df, dist = df2()
    _, seen = _seen2_first()
    gain, hits, _ = _check(df, dist, seen, (TH2, OFF2), candidates2())
    assert np.all(hits == 360) and gain.min() > 9000


def test_sphere_and_wall_scene_3d():
    df, dist = df3()
    shape, origin, step = _lat(df)
    seen = cover_ref.integrate_depth(np.zeros(dist.size, bool), shape, origin, step, depth3(), CAM, TRUE3, step)
    P2 = pose12(rot([0.2, 1.0, 0.1], math.radians(25.0)), np.array([-0.3, 0.1, 0.05]))
    gain, hits, _ = _check(df, dist, seen, CAM, np.stack([TRUE3, P2, OUTSIDE3]))
    assert hits[0] == 4800 and gain[0] < 100 < gain[1] and gain[2] == 0 and hits[2] == 0


@pytest.mark.parametrize("m", [1, TILE, TILE + 1])
def test_pose_counts_around_the_tile_2d_and_3d(m):
    df, dist = small2()
    gain, hits, _ = _check(df, dist, half_seen(dist.size), (TH90, (0.03, -0.02)), poses2(m), max_gap=GAP5)
    assert gain.max() > 100 and hits.max() > 0
    df, dist = small3()
    gain, hits, _ = _check(df, dist, half_seen(dist.size), CAM13, poses3(m))            # (13 x 7: both tiles hang over the image)
    assert gain.max() > 100 and hits.max() > 0 and hits.max() <= 91


@pytest.mark.parametrize("count", [0, 2047, 2048, 2049])
def test_target_counts_around_the_chunk(count):
    """`count` unseen points on a small lattice without a surface: the target list is exactly that long."""
    for lat, sensor, poses, opts in ((SMALL2, (TH90, (0.0, 0.0)), poses2(3), dict(max_gap=GAP5)), (SMALL3, CAM13, poses3(3), {})):
        df, dist = _free(**lat)
        n = dist.size
        seen = np.ones(n, bool)
        seen[np.sort(np.random.default_rng(count).permutation(n)[:count])] = False
        v = _scorer()
        gain, hits, _ = _check(df, dist, seen, sensor, poses, v=v, **opts)
        assert v.info()["targets"] == count and np.all(hits == 0) and (gain.max() > 0) == (count > 0) and gain.max() <= count


def _poke(df, index, value):
    """Write one float into the field's dist grid on the device."""
    import gpismap_amd
    L = gpismap_amd.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    v = C.c_float(value)
    assert L.hipMemcpy(C.c_void_p(df.device_ptrs()[0] + 4 * index), C.byref(v), 4, 1) == 0          # (1: host to device)


@pytest.mark.parametrize("min_dist", [-math.inf, 0.05, math.inf])
def test_min_dist_with_nan_and_infinite_distances(min_dist):
    import gpismap_amd
    for lat, ball, sensor, poses, opts in ((SMALL2, ((40.0, 20.0), 6.0), (TH90, (0.03, -0.02)), poses2(3), dict(max_gap=GAP5)),
                                           (SMALL3, ((12.0, 10.0, 10.0), 3.0), CAM13, poses3(3), {})):
        df = gpismap_amd.DistanceField()
        df, _ = _field(_balls(lat["shape"], lat["origin"], lat["step"], [ball]), df=df, **lat)
        n = int(np.prod(lat["shape"]))
        a, b = n // 3 + 1, n // 3 + 8                                    # (unseen both: neither is a multiple of 5)
        _poke(df, a, float("nan"))
        _poke(df, b, -math.inf)
        dist = df.get()[0].ravel()
        assert np.isnan(dist[a]) and dist[b] == -np.inf
        seen = np.zeros(n, bool)
        seen[::5] = True
        gain, _, _ = _check(df, dist, seen, sensor, poses, min_dist=min_dist, **opts)
        tg = view_ref.targets(seen, dist, min_dist)
        assert tg[a] and tg[b] == (min_dist == -math.inf)
        assert gain.max() <= tg.sum() and (gain.max() > 1) == (min_dist < math.inf)      # (+inf leaves the NaN point alone)


def test_a_nan_miss_and_other_misses_outside_the_window():
    df, dist = _free(**SMALL2)
    seen = np.zeros(dist.size, bool)
    for miss in (float("nan"), 0.0, 0.1, 30.0, float("inf")):
        gain, hits, _ = _check(df, dist, seen, (TH90, (0.0, 0.0)), poses2(2), miss=miss, max_gap=GAP5)
        assert np.all(hits == 0) and np.all(gain == 0)
    df3_, dist3_ = _free(**SMALL3)
    gain, hits, _ = _check(df3_, dist3_, np.zeros(dist3_.size, bool), CAM13, poses3(2), miss=float("nan"))
    assert np.all(hits == 0) and np.all(gain == 0)


def test_near_a_wall_the_sector_table_differs_between_poses_and_a_pose_outside():
    df, dist = df2()
    _, seen = _seen2_first()
    P = np.stack([WALL2, candidates2()[3], OUTSIDE2, WALL2])
    gain, hits, pred = _check(df, dist, seen, (TH2, OFF2), P, tnear=0.05)
    assert 0 < (pred[0] < F32(0.2)).sum() < 360 and gain[0] == gain[3] > 0 and 0 < hits[2] < 90


def test_map_level_calls_use_the_maps_camera_and_offset():
    from test_gpu_track import _gazebo_map, _synthetic_map
    g2, f2 = _gazebo_map(ids=range(1))
    lat = dict(shape=(120, 90), origin=(-6.0, -4.5), step=0.1)
    df, dist = _free(**lat)
    seen = half_seen(dist.size)
    cv = _cover(df).set(seen)
    P = np.stack([pose6(0.3, (0.2, -0.1)), pose6(2.0, (-1.0, 1.0))])
    th = f2[0]["thetas"]
    gain, hits = g2.view_gain_scan_field(df, cv, th, P)
    rg, rh, _ = view_ref.gain_scan(dist, seen, lat["shape"], lat["origin"], lat["step"], th, OFF2, P)
    assert np.array_equal(gain, rg) and np.array_equal(hits, rh) and rg.min() > 100
    gm = _synthetic_map(frames=1)
    df3_, dist3_ = _free(**SMALL3)
    seen3 = half_seen(dist3_.size)
    P3 = poses3(1)
    gain, hits = gm.view_gain_depth_field(df3_, _cover(df3_).set(seen3), P3)
    rg, rh, _ = view_ref.gain_depth(dist3_, seen3, SMALL3["shape"], SMALL3["origin"], SMALL3["step"], (568.0, 568.0, 310.0, 224.0, 640, 480), P3)
    assert np.array_equal(gain, rg) and np.array_equal(hits, rh) and rg[0] > 100


# ---- B. against the library's own single-pose entries ---------------------------------------------------------------------------
def test_gain_is_what_integrating_the_rendered_frame_would_add():
    import gpismap_amd
    df, dist = df2()
    cv, seen = _seen2_first()
    P = candidates2()[[0, 3, 7, 9, 14]]
    gain, hits = df.view_gain_scan(cv, TH2, P, OFF2)
    miss = gpismap_amd.view_opts(2, LAT_STEP(df)).miss
    scratch = _cover(df)
    for k in range(5):
        rng, _, status = df.render_scan(TH2, P[k], OFF2)
        d = np.where(status == 0, rng, F32(miss)).astype(F32)
        after = scratch.set(seen).integrate_scan(TH2, d, P[k], OFF2).get()
        assert int(after.sum()) - int(seen.sum()) == gain[k] and int((status == 0).sum()) == hits[k]
    assert np.array_equal(cv.get().ravel(), seen.astype(np.uint8))                 # (scoring leaves the mask alone)
    df3_, dist3_ = small3()
    seen3 = half_seen(dist3_.size)
    cv3 = _cover(df3_).set(seen3)
    P3 = poses3(5)
    gain, hits = df3_.view_gain_depth(cv3, CAM13, P3)
    miss = gpismap_amd.view_opts(3, LAT_STEP(df3_)).miss
    scratch = _cover(df3_)
    for k in range(5):
        dep, _, status = df3_.render_depth(P3[k], CAM13)
        d = np.where(status == 0, dep, F32(miss)).astype(F32)
        after = scratch.set(seen3).integrate_depth(d, P3[k], CAM13).get()
        assert int(after.sum()) - int(seen3.sum()) == gain[k] and int((status == 0).sum()) == hits[k]
    assert gain.max() > 100


def LAT_STEP(df):
    return df.info()["step"]


# ---- C. independence ------------------------------------------------------------------------------------------------------------
def test_batch_position_calls_and_streams():
    import torch
    for (df, dist), sensor, P, opts in ((small2(), (TH90, (0.03, -0.02)), poses2(TILE + 1), dict(max_gap=GAP5)),
                                        (small3(), CAM13, poses3(TILE + 1), {})):
        dim = df.info()["dim"]
        P[0] = P[31] = P[64] = P[5]
        cv = _cover(df).set(half_seen(dist.size))
        call = (lambda v, **kw: df.view_gain_depth(cv, sensor, P, scorer=v, **kw, **opts)) if dim == 3 else \
               (lambda v, **kw: df.view_gain_scan(cv, sensor[0], P, sensor[1], scorer=v, **kw, **opts))
        v = _scorer()
        gain, hits = call(v)
        assert gain[0] == gain[31] == gain[64] == gain[5] > 0 and hits[0] == hits[31] == hits[64] == hits[5]
        p5 = v.predicted(5)
        assert all(_bits_equal(v.predicted(k), p5) for k in (0, 31, 64))
        alone = (df.view_gain_depth(cv, sensor, P[5], **opts) if dim == 3 else df.view_gain_scan(cv, sensor[0], P[5], sensor[1], **opts))
        assert alone[0][0] == gain[5] and alone[1][0] == hits[5]
        g2, h2 = call(v)                                                            # again on the same holder
        assert np.array_equal(g2, gain) and np.array_equal(h2, hits)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ga, ha = call(_scorer(), stream=s1.cuda_stream)
        gb, hb = call(v, stream=s2.cuda_stream)
        assert np.array_equal(ga, gain) and np.array_equal(gb, gain) and np.array_equal(ha, hits) and np.array_equal(hb, hits)


# ---- D. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result():
    import gpismap_amd
    L = gpismap_amd.lib()
    ARG, STATE, LIMIT = -1, -3, -4
    fp = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    df, dist = small2()
    df3_, _ = small3()
    other, _ = _free((60, 41), SMALL2["origin"], SMALL2["step"])
    empty = gpismap_amd.DistanceField()
    cv = _cover(df).set(half_seen(dist.size))
    cv_other, cv3, cv_never = _cover(other), _cover(df3_), gpismap_amd.Coverage()
    P, P3 = poses2(3), poses3(2)
    off = np.array([0.03, -0.02], F32)
    cam = gpismap_amd.gpis_cam(*CAM13[:4], 13, 7)
    v, v3 = _scorer(), _scorer()
    gain, hits = df.view_gain_scan(cv, TH90, P, off, scorer=v, max_gap=GAP5)
    gain3, hits3 = df3_.view_gain_depth(cv3, CAM13, P3, scorer=v3)
    pred1 = v.predicted(1)
    o = gpismap_amd.view_opts(2, SMALL2["step"], max_gap=GAP5)
    o3 = gpismap_amd.view_opts(3, SMALL3["step"])
    scan = lambda df_=df, cv_=cv, v_=v, th=fp(TH90), n=90, off_=fp(off), p=fp(P), m=3, o_=o: \
        L.gpis2_view_gain_scan(None, df_.h if df_ is not None else None, cv_.h if cv_ is not None else None,
                               v_.h if v_ is not None else None, th, n, off_, p, m, C.byref(o_) if o_ is not None else None, None)
    depth = lambda df_=df3_, cv_=cv3, c=C.byref(cam), p=fp(P3), m=2, o_=o3: \
        L.gpis3_view_gain_depth(None, df_.h, cv_.h, v3.h, c, p, m, C.byref(o_), None)
    assert scan() == 0 and depth() == 0
    # the march's refusals, cover's for back_off / max_gap, a NaN min_dist
    for bad in (dict(tnear=-0.1), dict(tnear=31.0), dict(min_step=0.0), dict(max_step=0.001), dict(refine=65), dict(max_steps=0),
                dict(slack=-1.0), dict(tfar=float("inf")), dict(back_off=-0.01), dict(back_off=float("nan")), dict(max_gap=0.0),
                dict(max_gap=1.6), dict(min_dist=float("nan"))):
        assert scan(o_=gpismap_amd.view_opts(2, SMALL2["step"], **bad)) == ARG, bad
        assert depth(o_=gpismap_amd.view_opts(3, SMALL3["step"], **bad)) == ARG, bad
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.view_opts(2, 0.02, nonsense=1)
    # a non-finite pose, m < 1, missing arguments, bad frames
    for idx in (0, 7, 17):
        badp = P.copy()
        badp.ravel()[idx] = np.inf if idx else np.nan
        assert scan(p=fp(badp)) == ARG
    badp3 = P3.copy()
    badp3[1, 11] = np.nan
    assert depth(p=fp(badp3)) == ARG
    assert scan(m=0) == ARG and scan(m=-1) == ARG and depth(m=0) == ARG
    assert scan(df_=None) == ARG and scan(cv_=None) == ARG and scan(v_=None) == ARG and scan(th=None) == ARG and scan(p=None) == ARG
    assert scan(off_=None) == ARG and scan(n=0) == ARG and depth(c=None) == ARG                 # (no offset / camera and no map)
    assert scan(th=fp(np.array([0.0, np.inf], F32)), n=2) == ARG
    zero_fx = gpismap_amd.gpis_cam(0.0, 10.0, 6.0, 3.0, 13, 7)
    assert depth(c=C.byref(zero_fx)) == ARG
    # the limits, before the poses are read (the pose array holds 3 poses)
    assert scan(m=65537) == LIMIT and scan(m=65536, n=1025) == LIMIT and depth(m=65537) == LIMIT
    big = gpismap_amd.gpis_cam(500.0, 500.0, 512.0, 512.0, 1024, 1024)
    assert depth(c=C.byref(big), m=65) == LIMIT
    # a field of the other dim, a field without a result, a coverage that is not on the field's lattice
    assert scan(df_=df3_, cv_=cv3) == ARG and depth(df_=df, cv_=cv) == ARG
    assert scan(df_=empty) == STATE and scan(df_=empty, o_=None) == STATE
    assert scan(cv_=cv_other) == STATE and scan(cv_=cv_never) == STATE and scan(cv_=cv3) == STATE and depth(cv_=cv) == STATE
    # reading back: a wrong count, a pose or ray count out of range, a holder without a result
    buf, ibuf, fbuf = np.zeros(8, np.int64), np.zeros(8, np.int32), np.zeros(90, F32)
    ll = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    assert L.gpis_view_get(v.h, ll(buf), ip(ibuf), 2) == ARG and L.gpis_view_get(None, ll(buf), ip(ibuf), 3) == ARG
    assert L.gpis_view_get_predicted(v.h, 3, fp(fbuf), 90) == ARG and L.gpis_view_get_predicted(v.h, -1, fp(fbuf), 90) == ARG
    assert L.gpis_view_get_predicted(v.h, 0, fp(fbuf), 89) == ARG and L.gpis_view_get_predicted(v.h, 0, None, 90) == ARG
    fresh = _scorer()
    assert fresh.info()["valid"] == 0 and L.gpis_view_get(fresh.h, ll(buf), ip(ibuf), 3) == STATE
    assert L.gpis_view_get_predicted(fresh.h, 0, fp(fbuf), 90) == STATE
    with pytest.raises(gpismap_amd.GpisError):
        df.view_gain_scan(cv, TH90, P.ravel()[:17], off)
    with pytest.raises(gpismap_amd.GpisError):
        df.view_gain_scan(cv, TH90, P, None)
    # none of this touched the held results, the mask or the field
    g, h = v.get()
    assert np.array_equal(g, gain) and np.array_equal(h, hits) and _bits_equal(v.predicted(1), pred1) and v.info()["poses"] == 3
    g, h = v3.get()
    assert np.array_equal(g, gain3) and np.array_equal(h, hits3)
    assert np.array_equal(cv.get().ravel(), half_seen(dist.size).astype(np.uint8)) and _bits_equal(df.get()[0].ravel(), dist)


# ---- E. next_view ---------------------------------------------------------------------------------------------------------------
def test_next_view_picks_the_largest_gain_and_plans_through_seen_space():
    df, dist = df2()
    shape, origin, step = _lat(df)
    cv, seen = _seen2_first()
    path, status, pose, gains, clusters = df.next_view(cv, TRUE2[:2], (TH2, OFF2), YAWS8, clearance=0.1)
    assert status == 0 and path.shape[0] > 10 and gains.shape == (2, 8) and gains.dtype == np.int64
    rg, _, _ = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, candidates2())
    assert np.array_equal(gains.ravel(), rg) and _bits_equal(clusters["rep"], cover_ref.frontiers(seen, dist, shape, origin, step, 0.1, 8)["rep_point"])
    best = int(np.argmax(rg))
    assert _bits_equal(pose, candidates2()[best]) and _bits_equal(path[-1], clusters["rep"][best // 8])
    ok, ijk = plan_ref.snap(path, shape, origin, step)
    assert ok.all() and seen[ijk[:, 1] * shape[0] + ijk[:, 0]].all()
    # a fully seen mask: no cluster, status 4
    full = _cover(df).set(np.ones(dist.size, bool))
    p2, st2, pose2, g2, c2 = df.next_view(full, TRUE2[:2], (TH2, OFF2), YAWS8, clearance=0.1)
    assert st2 == 4 and p2.shape == (0, 2) and pose2 is None and g2.shape == (0, 8) and c2["label"].size == 0
    # explore itself is what it was
    path_e, st_e, _ = df.explore(cv, TRUE2[:2], clearance=0.1)
    rpath, rst, _ = cover_ref.explore(seen, dist, shape, origin, step, TRUE2[:2], 0.1, margin=4 * float(F32(step)))
    assert st_e == rst == 0 and _bits_equal(path_e, rpath)


def test_next_view_3d_candidates_turn_about_the_base_pose():
    import gpismap_amd
    df, dist = df3()
    shape, origin, step = _lat(df)
    seen = cover_ref.integrate_depth(np.zeros(dist.size, bool), shape, origin, step, depth3(), CAM, TRUE3, step)
    cv = _cover(df).set(seen)
    yaws = np.array([-0.4, 0.0, 0.4])
    path, status, pose, gains, clusters = df.next_view(cv, (0.0, 0.0, 1.0), CAM, yaws, base_pose=TRUE3)
    nc = clusters["label"].size
    assert nc >= 1 and gains.shape == (nc, 3)
    cand = []
    for r in clusters["rep"]:
        b = TRUE3.copy()
        b[:3] = r
        cand.append(gpismap_amd.pose_grid3(b, np.zeros((1, 3)), np.stack([0 * yaws, 0 * yaws, yaws], axis=1)))
    cand = np.concatenate(cand)
    rg, _, _ = view_ref.gain_depth(dist, seen, shape, origin, step, CAM, cand)
    assert np.array_equal(gains.ravel(), rg)
    if rg.max() > 0:
        assert _bits_equal(pose, cand[int(np.argmax(rg))]) and status in (0, 1, 2, 3)
    else:
        assert status == 4 and pose is None
