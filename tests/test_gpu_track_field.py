"""Tracking against a distance field on the GPU (csrc/track.hip, gpis3_track_depth_field / gpis2_track_scan_field): the device
call against the numpy reference (tests/track_field_ref.py) bit for bit, at kernel level (analytic f grids through from_grid)
and at map level (the fields of the synthetic, bigbird and gazebo maps); pose recovery against the map tracker on the same
input; determinism across runs, streams, update modes and a two-device map; the map tracker unchanged by a field call on the
same tracker; the edges and the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_ref
import replay
import track_field_ref
from test_gpu_dfield import BOX2, BOX3, SYN
from test_gpu_track import (SYN_CAM, SYN_TRUE, _bigbird_map, _bits_equal, _check_bits, _err2, _err3, _gazebo_map, _neighbours,
                            _perturb2, _perturb3, _quarter, _same, _synthetic_map)
from test_track_ref import CAM, OFF2, depth_image, pose6, pose12, rot, scan, scene2, scene3

pytestmark = pytest.mark.gpu
F32 = np.float32

# analytic lattices (as tests/test_track_field_ref.py)
LAT3 = dict(shape=(131, 101, 48), origin=(-1.3, -1.0, 0.8), step=0.02)
LAT2 = dict(shape=(396, 231), origin=(-3.2, -1.9), step=0.02)


def _grid_field(scene, lat):
    import gpismap_amd
    import torch
    x = mesh_ref.lattice(lat["shape"], lat["origin"], [lat["step"]] * len(lat["shape"]))
    f = scene(x.astype(np.float64))[0].astype(F32)
    t = torch.from_numpy(f).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    df = gpismap_amd.DistanceField()
    df.from_grid(t.data_ptr(), lat["shape"], lat["origin"], lat["step"], 0.0)
    return df


def _lat(df):
    i = df.info()
    return i["shape"], i["origin"], i["step"]


def _ref3(df, depth, cam, pose0, **kw):
    shape, origin, step = _lat(df)
    return track_field_ref.track_depth(df.get()[0].ravel(), shape, origin, step, depth, cam, pose0, **kw)


def _ref2(df, thetas, ranges, pose0, off2=OFF2, **kw):
    shape, origin, step = _lat(df)
    return track_field_ref.track_scan(df.get()[0].ravel(), shape, origin, step, thetas, ranges, pose0, off2, **kw)


# ---- bits -----------------------------------------------------------------------------------------------------------------
def test_bits_kernel_level_3d_and_2d():
    df3 = _grid_field(scene3, LAT3)
    T_true = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
    depth = depth_image(scene3, CAM, T_true)
    start = _perturb3(T_true, 0.02, 2.0)
    for kw in (dict(stride=1), dict(stride=2, max_iters=3), dict(stride=1, huber=1e-3, max_residual=0.02)):
        out = df3.track_depth(depth, start, CAM, **kw)
        assert out[1]["inliers"] > 1000 and out[1]["evals"] == 0 and out[1]["k4_ms"] == 0.0
        _check_bits(out, _ref3(df3, depth, CAM, start, **kw), "analytic 3-D %s" % kw)
    df2 = _grid_field(scene2, LAT2)
    th = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)
    T2 = pose6(0.15, (0.3, -0.2))
    ranges = scan(scene2, th, T2)
    for off2 in (OFF2, (0.0, 0.05)):
        start2 = _perturb2(T2, 0.05, 3.0)
        out = df2.track_scan(th, ranges, start2, off2)
        assert out[1]["inliers"] > 300
        _check_bits(out, _ref2(df2, th, ranges, start2, off2), "analytic 2-D offset %s" % (off2,))


def test_bits_map_level():
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    depth, _, st = gm.render_depth(SYN_TRUE, cam6=SYN_CAM)
    start = _perturb3(SYN_TRUE, 0.02, 2.0)
    out = gm.track_depth_field(df, depth, start, cam6=SYN_CAM)
    assert out[1]["points"] > 15000 and out[1]["inliers"] > 10000
    _check_bits(out, _ref3(df, depth, SYN_CAM, start), "synthetic field 320x240")
    gb, frames = _bigbird_map()
    dfb = gb.distance_field(**BOX3)
    for i in (0, 2, 4):
        d, cam = _quarter(frames[i])
        s = _perturb3(frames[i]["pose"], 0.01, 1.0)
        out = gb.track_depth_field(dfb, d, s, cam6=cam)
        assert out[1]["inliers"] > 100
        _check_bits(out, _ref3(dfb, d, cam, s), "bigbird field frame %d at 1/4" % i)
    g2, f2 = _gazebo_map()
    df2 = g2.distance_field(**BOX2)
    for i in (0, len(f2) // 2, len(f2) - 1):
        fr = f2[i]
        s = _perturb2(fr["pose"], 0.05, 1.0)
        out = g2.track_scan_field(df2, fr["thetas"], fr["ranges"], s)
        assert out[1]["inliers"] > 20
        _check_bits(out, _ref2(df2, fr["thetas"], fr["ranges"], s), "gazebo field scan %d" % i)


# ---- recovery -------------------------------------------------------------------------------------------------------------
# Bounds from the first run on an MI355X with a 1.5x margin (DESIGN.md §7f has the measured values).  The synthetic wall is a
# measured miss: against the field it does not converge from 2 cm / 2 degrees either (status 1, 4.8 cm / 0.67 deg, the map
# tracker 4.3 cm / 0.68 deg), and the map tracker started from the field's pose stops (status 0) 4.5 cm off -- the cost of this
# wall has a flat valley away from the true pose, whichever residual is used.  The test guards what was measured.
SYN_FIELD_BOUND = (0.073, 1.01)            # metres, degrees (measured 0.0484 m, 0.671 deg)
SYN_REFINED_BOUND = (0.067, 0.63)          # the map tracker from the field's pose (measured 0.0447 m, 0.421 deg)
BB_FIELD_BOUND = {2: (0.0081, 0.72), 17: (0.018, 1.44)}    # measured 2: 0.0054 m 0.48 deg; 17: 0.0120 m 0.96 deg
GZ_FIELD_BOUND = {(0.1, 2.0): (0.020, 0.21), (0.3, 5.0): (0.020, 0.21)}    # measured 0.0073 - 0.0133 m, 0.08 - 0.14 deg


def test_recovery_synthetic_and_map_refinement():
    """640x480 depth rendered from SYN_TRUE, tracked from a further 2 cm / 2 degrees against the map's field, next to the map
    tracker from the same start; then the map tracker from the field's pose."""
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    depth, _, _ = gm.render_depth(SYN_TRUE)
    start = _perturb3(SYN_TRUE, 0.02, 2.0)
    pf, inf = gm.track_depth_field(df, depth, start)
    pm, inm = gm.track_depth(depth, start)
    pr, inr = gm.track_depth(depth, pf)
    e0, ef, em, er = (_err3(p, SYN_TRUE) for p in (start, pf, pm, pr))
    print("synthetic 640x480 from %.4f m %.3f deg: field %.2e m %.3f deg (status %d, %d iterations, %d inliers of %d); "
          "map %.2e m %.3f deg (status %d); map from the field's pose %.2e m %.3f deg (status %d, %d iterations)"
          % (e0 + ef + (inf["status"], inf["iterations"], inf["inliers"], inf["points"]) + em + (inm["status"],) + er
             + (inr["status"], inr["iterations"])))
    assert inf["status"] in (0, 1) and inf["cost"] < inf["cost0"] and inf["evals"] == 0
    assert ef[1] < e0[1] and er[1] < e0[1]
    assert ef[0] <= SYN_FIELD_BOUND[0] and ef[1] <= SYN_FIELD_BOUND[1]
    assert er[0] <= SYN_REFINED_BOUND[0] and er[1] <= SYN_REFINED_BOUND[1]


def test_recovery_bigbird_held_out_frames():
    frames = replay.load_bigbird()
    errs = []
    for k in (2, 17):
        ids = _neighbours(frames, k, 4)
        gm, _ = _bigbird_map(ids)
        df = gm.distance_field(**BOX3)
        fr = frames[k]
        start = _perturb3(fr["pose"], 0.02, 2.0)
        pose, info = gm.track_depth_field(df, fr["depth"], start, cam6=fr["cam"])
        pm, im = gm.track_depth(fr["depth"], start, cam6=fr["cam"])
        e0, e, em = _err3(start, fr["pose"]), _err3(pose, fr["pose"]), _err3(pm, fr["pose"])
        print("bigbird frame %d (map %s): start %.4f m %.3f deg -> field %.2e m %.3f deg (status %d, %d iterations, %d of %d "
              "inliers); map %.2e m %.3f deg" % ((k, ids) + e0 + e + (info["status"], info["iterations"], info["inliers"],
                                                                      info["points"]) + em))
        errs.append((k, e))
        assert info["status"] in (0, 1) and e[0] < em[0]
    for k, e in errs:
        assert e[0] <= BB_FIELD_BOUND[k][0] and e[1] <= BB_FIELD_BOUND[k][1], (k, e)


def test_recovery_gazebo_scans():
    frames = replay.load_gazebo()
    for k in (6, 14, 22):
        gm, _ = _gazebo_map(range(k))
        df = gm.distance_field(**BOX2)
        fr = frames[k]
        for (dt, deg), bound in GZ_FIELD_BOUND.items():
            start = _perturb2(fr["pose"], dt, deg)
            pose, info = gm.track_scan_field(df, fr["thetas"], fr["ranges"], start)
            pm, im = gm.track_scan(fr["thetas"], fr["ranges"], start)
            e0, e, em = _err2(start, fr["pose"]), _err2(pose, fr["pose"]), _err2(pm, fr["pose"])
            print("gazebo scan %d from %.3f m %.2f deg: field %.2e m %.3f deg (status %d, %d iterations, %d of %d inliers); "
                  "map %.2e m %.3f deg (status %d)" % ((k,) + e0 + e + (info["status"], info["iterations"], info["inliers"],
                                                                       info["points"]) + em + (im["status"],)))
            assert info["status"] in (0, 1)
            assert e[0] <= bound[0] and e[1] <= bound[1], (k, dt, deg, e)


# ---- invariance -----------------------------------------------------------------------------------------------------------
def _call3(L, map_h, df, t, depth, pose0, cam6=None, stream=None, **kw):
    import gpismap_amd
    P = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    o = gpismap_amd.track_opts(3, **kw)
    c = C.byref(gpismap_amd._cam(cam6)) if cam6 is not None else None
    out = np.zeros(12, F32)
    d, p = np.ascontiguousarray(depth, F32), np.ascontiguousarray(pose0, F32)
    rc = L.gpis3_track_depth_field(map_h, df.h if df is not None else None, t.h, c, P(d), P(p), C.byref(o), P(out), stream)
    return rc, out


def _call2(L, map_h, df, t, fr, pose0, off2=None, stream=None, **kw):
    import gpismap_amd
    P = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    o = gpismap_amd.track_opts(2, **kw)
    out = np.zeros(6, F32)
    th, rg, p = (np.ascontiguousarray(a, F32) for a in (fr["thetas"], fr["ranges"], pose0))
    rc = L.gpis2_track_scan_field(map_h, df.h if df is not None else None, t.h, P(th), P(rg), th.size,
                                  P(off2) if off2 is not None else None, P(p), C.byref(o), P(out), stream)
    return rc, out


def test_deterministic_across_runs_streams_modes_devices():
    import gpismap_amd
    import torch
    L = gpismap_amd.lib()
    gm, frames = _bigbird_map()
    df = gm.distance_field(**BOX3)
    fr = frames[2]
    depth, cam = _quarter(fr, 2)
    start = _perturb3(fr["pose"], 0.01, 1.0)
    t = gpismap_amd.Tracker()
    a = gm.track_depth_field(df, depth, start, cam6=cam, tracker=t)
    assert a[1]["inliers"] > 300
    others = [gm.track_depth_field(df, depth, start, cam6=cam, tracker=t), df.track_depth(depth, start, cam)]
    s = torch.cuda.Stream(device=0)
    t2 = gpismap_amd.Tracker()
    rc, p = _call3(L, gm.h, df, t2, depth, start, cam6=cam, stream=C.c_void_p(s.cuda_stream))
    assert rc == 0
    others.append((p, t2.result()))
    for g in (_bigbird_map(pipeline=False)[0], _bigbird_map(devices=[0, 0])[0]):
        others.append(g.track_depth_field(g.distance_field(**BOX3), depth, start, cam6=cam))
    if gpismap_amd.device_count() >= 2:
        g = _bigbird_map(devices=[0, 1])[0]
        others.append(g.track_depth_field(g.distance_field(**BOX3), depth, start, cam6=cam))
    for o in others:
        assert _same(o, a)
    g2, f2 = _gazebo_map()
    s2, _ = _gazebo_map(pipeline=False)
    th, rg, p2 = f2[5]["thetas"], f2[5]["ranges"], _perturb2(f2[5]["pose"], 0.05, 1.0)
    x = g2.track_scan_field(g2.distance_field(**BOX2), th, rg, p2)
    y = g2.track_scan_field(g2.distance_field(**BOX2), th, rg, p2, tracker=gpismap_amd.Tracker())
    z = s2.track_scan_field(s2.distance_field(**BOX2), th, rg, p2)
    assert x[1]["inliers"] > 20 and _same(x, y) and _same(x, z)


def test_map_tracking_unchanged_by_a_field_call_on_the_same_tracker():
    import gpismap_amd
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    depth, _, _ = gm.render_depth(SYN_TRUE, cam6=SYN_CAM)
    start = _perturb3(SYN_TRUE, 0.01, 1.0)
    fresh = gm.track_depth(depth, start, cam6=SYN_CAM, tracker=gpismap_amd.Tracker())
    t = gpismap_amd.Tracker()
    before = gm.track_depth(depth, start, cam6=SYN_CAM, tracker=t)
    f1 = gm.track_depth_field(df, depth, start, cam6=SYN_CAM, tracker=t)
    after = gm.track_depth(depth, start, cam6=SYN_CAM, tracker=t)
    f2 = gm.track_depth_field(df, depth, start, cam6=SYN_CAM, tracker=t)
    assert _same(before, fresh) and _same(after, fresh) and _same(f1, f2)
    assert fresh[1]["evals"] > 0 and f1[1]["evals"] == 0


# ---- edges and errors -----------------------------------------------------------------------------------------------------
def test_no_sites_or_outside_gives_status_2_and_max_iters_zero():
    import gpismap_amd
    import torch
    depth = replay.synthetic_depth(0)
    cam = (568.0, 568.0, 310.0, 224.0, 640, 480)
    ones = torch.ones(64, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    empty = gpismap_amd.DistanceField().from_grid(ones.data_ptr(), (4, 4, 4), (-0.1, -0.1, 0.9), 0.05, 0.0)
    pose, info = empty.track_depth(depth, replay.IDENTITY_POSE, cam)
    assert info["status"] == 2 and info["inliers"] == 0 and info["passes"] == 1 and info["points"] > 0
    assert _bits_equal(pose, replay.IDENTITY_POSE) and np.all(np.isnan(info["resid"]))
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    far = replay.IDENTITY_POSE.copy()
    far[:3] = (50.0, 0.0, 0.0)
    pose, info = gm.track_depth_field(df, depth, far)
    assert info["status"] == 2 and info["inliers"] == 0 and _bits_equal(pose, far)
    P = _perturb3(replay.IDENTITY_POSE, 0.005, 0.5)
    pose, info = gm.track_depth_field(df, depth, P, max_iters=0)
    assert info["status"] == 1 and info["iterations"] == 0 and info["passes"] == 1
    assert _bits_equal(pose, P) and info["cost"] == info["cost0"] > 0
    _check_bits((pose, info), _ref3(df, depth, cam, P, max_iters=0), "evaluate only")
    # 2-D: a field without sites
    g2, f2 = _gazebo_map(range(3))
    ones2 = torch.ones(16, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    e2 = gpismap_amd.DistanceField().from_grid(ones2.data_ptr(), (4, 4), (0.0, 0.0), 1.0, 0.0)
    pose, info = e2.track_scan(f2[1]["thetas"], f2[1]["ranges"], f2[1]["pose"], OFF2)
    assert info["status"] == 2 and info["inliers"] == 0


def test_errors_and_map_defaults():
    import gpismap_amd
    L = gpismap_amd.lib()
    gm = _synthetic_map(frames=2)
    df = gm.distance_field(**SYN)
    cam = (142.0, 142.0, 77.5, 56.0, 160, 120)
    depth, _, _ = gm.render_depth(SYN_TRUE, cam6=cam)
    start = _perturb3(SYN_TRUE, 0.01, 1.0)
    t = gpismap_amd.Tracker()
    a = gm.track_depth_field(df, depth, start, cam6=cam, tracker=t)
    assert a[1]["inliers"] > 500

    def still_there():
        assert _same((a[0], t.result()), a)

    # level and max_var are not read
    for kw in (dict(level=np.inf), dict(level=np.nan), dict(max_var=np.nan), dict(max_var=-1.0), dict(level=0.3, max_var=0.0)):
        rc, p = _call3(L, gm.h, df, t, depth, start, cam6=cam, **kw)
        assert rc == 0 and _same((p, t.result()), a), kw
    # argument errors
    bad_pose = start.copy(); bad_pose[4] = np.nan
    for kw in (dict(pose0=bad_pose), dict(cam6=(0.0, 142.0, 77.5, 56.0, 160, 120)), dict(stride=0), dict(max_iters=-1),
               dict(huber=0.0), dict(max_residual=np.nan), dict(damping=np.inf), dict(eps_t=-1.0), dict(min_inliers=-1)):
        args = dict(pose0=start, cam6=cam)
        args.update(kw)
        pose0 = args.pop("pose0")
        rc, _ = _call3(L, gm.h, df, t, depth, pose0, **args)
        assert rc == -1, kw
        still_there()
    assert _call3(L, None, df, t, depth, start, cam6=None)[0] == -1          # no camera without a map
    assert _call3(L, gm.h, None, t, depth, start, cam6=cam)[0] == -1         # no field
    still_there()
    # a field of another dim: an argument error; a field without a result: a state error
    g2, f2 = _gazebo_map(range(5))
    df2 = g2.distance_field(**BOX2)
    assert _call3(L, gm.h, df2, t, depth, start, cam6=cam)[0] == -1
    still_there()
    nores = gpismap_amd.DistanceField()
    assert _call3(L, gm.h, nores, t, depth, start, cam6=cam)[0] == -3
    still_there()
    assert _call3(L, gm.h, df, t, depth, start, cam6=(142.0, 142.0, 77.5, 56.0, 8193, 8192))[0] == -4
    still_there()
    with pytest.raises(gpismap_amd.GpisError):
        df.track_depth(depth[:-1], start, cam)
    # 2-D
    fr = f2[3]
    t2 = gpismap_amd.Tracker()
    b = g2.track_scan_field(df2, fr["thetas"], fr["ranges"], fr["pose"], tracker=t2)
    assert b[1]["inliers"] > 20
    assert _call2(L, None, df2, t2, fr, fr["pose"])[0] == -1                 # no offset without a map
    assert _call2(L, g2.h, df, t2, fr, fr["pose"])[0] == -1                  # a 3-D field
    assert _call2(L, g2.h, nores, t2, fr, fr["pose"])[0] == -3
    bad_th = dict(fr, thetas=fr["thetas"].copy()); bad_th["thetas"][2] = np.nan
    assert _call2(L, g2.h, df2, t2, bad_th, fr["pose"])[0] == -1
    assert _same((b[0], t2.result()), b)
    # more than 2^26 beams: refused before thetas is read, also when it holds a NaN (the arrays are whole, so another order of
    # the checks would read valid memory and return another code); the result kept
    big = np.zeros((1 << 26) + 1, F32)
    assert _call2(L, g2.h, df2, t2, dict(thetas=big, ranges=big), fr["pose"])[0] == -4
    assert _same((b[0], t2.result()), b)
    big_nan = np.zeros((1 << 26) + 1, F32); big_nan[2] = np.nan
    assert _call2(L, g2.h, df2, t2, dict(thetas=big_nan, ranges=big), fr["pose"])[0] == -4
    assert _same((b[0], t2.result()), b)
    del big, big_nan
    # the map's camera / sensor offset when the caller passes none: the same bits as passing them
    d640 = replay.synthetic_depth(1)
    rc, p = _call3(L, gm.h, df, t, d640, start)
    r1 = (p, t.result())
    rc2, p2 = _call3(L, None, df, t, d640, start, cam6=(568.0, 568.0, 310.0, 224.0, 640, 480))
    assert rc == 0 and rc2 == 0 and r1[1]["inliers"] > 1000 and _same((p2, t.result()), r1)
    rc, p = _call2(L, g2.h, df2, t2, fr, fr["pose"])
    r2 = (p, t2.result())
    rc2, p2 = _call2(L, None, df2, t2, fr, fr["pose"], off2=np.array(OFF2, F32))
    assert rc == 0 and rc2 == 0 and _same((p2, t2.result()), r2) and _same(r2, b)
    # after the errors the tracker works again
    assert _same(gm.track_depth_field(df, depth, start, cam6=cam, tracker=t), a)
