"""Rendering on the GPU (csrc/render.hip, gpis3_render_depth / gpis2_render_scan / gpis_render_*): the device render against the
numpy reference (tests/render_ref.py) driven by the same map's host test(), bit for bit; the reference driven by the CPU oracle;
determinism across runs, chunkings, update modes and a two-shard map; the geometry of the synthetic scene and of the real
sequences; a rendered depth image fed back to update(); the error paths."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import render_ref
import replay

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
LEVEL = -0.2                      # -fbias of both maps
# 0.9 x the search half-width in float32, as the maps resolve far_step: 3-D 3 x the 0.025 cluster half length, 2-D
# 4 x map_scale_param 1.2
FAR3 = float(F32(0.9) * F32(np.float64(F32(0.025)) * 3.0))
FAR2 = float(F32(0.9) * F32(np.float64(F32(1.2)) * 4.0))
OFF2 = (0.08, 0.0)                # the 2-D map's default sensor offset
SYN_CAM = (284.0, 284.0, 155.0, 112.0, 320, 240)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _same(x, y):
    return _bits_equal(x[0], y[0]) and _bits_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


def _synthetic_map(frames=5, **kw):
    import gpismap_amd
    gm = gpismap_amd.GPisMap3(**kw)
    for fr in range(frames):
        gm.update(replay.synthetic_depth(fr), replay.IDENTITY_POSE)
    return gm


def _bigbird_map(nframes=5, devices=None, pipeline=True):
    import gpismap_amd
    frames = replay.load_bigbird()
    gm = gpismap_amd.GPisMap3(frames[0]["cam"], devices=devices)
    if not pipeline:
        gm.set_pipeline(False)
    for i in range(nframes):
        if i:
            gm.set_camera(frames[i]["cam"])
        gm.update(frames[i]["depth"], frames[i]["pose"])
    return gm, frames


def _gazebo_map(pipeline=True):
    import gpismap_amd
    gm = gpismap_amd.GPisMap()
    if not pipeline:
        gm.set_pipeline(False)
    frames = replay.load_gazebo()
    for fr in frames:
        gm.update(fr["thetas"], fr["ranges"], fr["pose"])
    return gm, frames


def _scaled(cam, k):
    return (cam[0] / k, cam[1] / k, cam[2] / k, cam[3] / k, int(cam[4]) // k, int(cam[5]) // k)


def _gpu3(gm, pose, cam, r=None, **kw):
    import gpismap_amd
    r = r or gpismap_amd.Renderer()
    out = gm.render_depth(pose, cam6=cam, renderer=r, level=LEVEL, far_step=FAR3, **kw)
    return out, r


def _ref3(test_fn, pose, cam, r, **kw):
    lo, hi = r.box()
    o = render_ref.Opts(3, level=LEVEL, far_step=FAR3, **kw)
    return render_ref.render_depth(test_fn, cam, pose, (lo, hi), o)


def _check_bits(out, r, ref, what):
    d, rec, st, stats = ref
    info = r.info()
    print("%s: %d rays, %d hits, %d passes (%d march), %d samples, %d K4 evaluations"
          % (what, d.size, stats["hits"], info["passes"], info["march_passes"], info["samples"], info["evals"]))
    assert np.array_equal(out[2], st), (what, np.bincount(out[2]), np.bincount(st))
    assert _bits_equal(out[0], d), what
    assert _bits_equal(out[1], rec), what
    assert (info["passes"], info["march_passes"], info["samples"], info["hits"]) == \
        (stats["passes"], stats["march_passes"], stats["samples"], stats["hits"]), what


# ---- bits ---------------------------------------------------------------------------------------------------------------
def test_bits_synthetic_320x240():
    gm = _synthetic_map()
    out, r = _gpu3(gm, replay.IDENTITY_POSE, SYN_CAM)
    assert np.count_nonzero(out[2] == 0) > 0.5 * out[2].size
    _check_bits(out, r, _ref3(lambda x, res: gm.test(x, res), replay.IDENTITY_POSE, SYN_CAM, r), "synthetic 320x240")


def test_bits_bigbird_frame_poses():
    gm, frames = _bigbird_map()
    for i in (0, 2, 4):
        cam = _scaled(frames[i]["cam"], 4)
        out, r = _gpu3(gm, frames[i]["pose"], cam)
        assert np.count_nonzero(out[2] == 0) > 50
        _check_bits(out, r, _ref3(lambda x, res: gm.test(x, res), frames[i]["pose"], cam, r), "bigbird frame %d" % i)


def test_bits_gazebo_frame_poses():
    import gpismap_amd
    gm, frames = _gazebo_map()
    for i in (0, len(frames) // 2, len(frames) - 1):
        r = gpismap_amd.Renderer()
        out = gm.render_scan(frames[i]["thetas"], frames[i]["pose"], renderer=r, level=LEVEL, far_step=FAR2)
        lo, hi = r.box()
        o = render_ref.Opts(2, level=LEVEL, far_step=FAR2)
        ref = render_ref.render_scan(lambda x, res: gm.test(x, res), frames[i]["thetas"], frames[i]["pose"], OFF2, (lo, hi), o)
        assert np.count_nonzero(out[2] == 0) > 50
        _check_bits(out, r, ref, "gazebo frame %d" % i)


def test_defaults_resolve_level_and_far_step():
    """No options: level -fbias and far_step 0.9 x the search half-width -- the same call as the explicit values."""
    import gpismap_amd
    gm = _synthetic_map(frames=2)
    r = gpismap_amd.Renderer()
    a = gm.render_depth(replay.IDENTITY_POSE, cam6=SYN_CAM, renderer=r)
    b, _ = _gpu3(gm, replay.IDENTITY_POSE, SYN_CAM)
    assert _same(a, b)


def test_oracle_cross_check_64x48():
    """bigbird frame 0: the reference driven by the CPU oracle (tiled mode, the kernels' arithmetic) gives the GPU render."""
    gm, frames = _bigbird_map(nframes=1)
    om = oracle_lib.OracleMap3(frames[0]["cam"])
    om.update(frames[0]["depth"], frames[0]["pose"])
    cam = _scaled(frames[0]["cam"], 10)
    out, r = _gpu3(gm, frames[0]["pose"], cam)

    def ofn(x, res):
        assert om.L.orc3_test(om.h, x.ctypes.data_as(C.POINTER(C.c_float)), 3, x.shape[0], res.ctypes.data_as(C.POINTER(C.c_float)))
        return res
    ref = _ref3(ofn, frames[0]["pose"], cam, r)
    hit = out[2] == 0
    print("oracle 64x48: %d GPU hits, %d reference hits, %d records differ"
          % (hit.sum(), (ref[2] == 0).sum(), int(np.count_nonzero(np.any(out[1].view(U32) != ref[1].view(U32), axis=1)))))
    _check_bits(out, r, ref, "oracle 64x48")


# ---- invariance ----------------------------------------------------------------------------------------------------------
def test_deterministic_across_runs_chunks_modes_devices():
    import gpismap_amd
    gm, frames = _bigbird_map()
    pose, cam = frames[2]["pose"], _scaled(frames[2]["cam"], 2)
    a, r = _gpu3(gm, pose, cam)
    b, _ = _gpu3(gm, pose, cam, r=r)
    small = gpismap_amd.Renderer()
    small.set_chunk(1000)
    c, _ = _gpu3(gm, pose, cam, r=small)
    sync, _ = _gpu3(_bigbird_map(pipeline=False)[0], pose, cam)
    multi, _ = _gpu3(_bigbird_map(devices=[0, 0])[0], pose, cam)
    assert np.count_nonzero(a[2] == 0) > 100
    for other in (b, c, sync, multi):
        assert _same(other, a)
    g2, f2 = _gazebo_map()
    s2, _ = _gazebo_map(pipeline=False)
    th, p2 = f2[5]["thetas"], f2[5]["pose"]
    x = g2.render_scan(th, p2)
    m2 = gpismap_amd.Renderer()
    m2.set_chunk(7)
    y = g2.render_scan(th, p2, renderer=m2)
    z = s2.render_scan(th, p2)
    assert _same(x, y) and _same(x, z)


# ---- geometry -------------------------------------------------------------------------------------------------------------
# Bounds from the first run on an MI355X with a 1.5x margin.  Measured: synthetic 303 008 hits (302 693 with var_f <= 0.02),
# distance outside the five surfaces' band median 0, p99 2.33e-4 m, max 3.18e-3 m; bigbird 316 096 pixels valid in both,
# |rendered - measured| median 2.54e-3 m, p90 7.22e-2 m (silhouettes: a pixel on the object's edge in one frame sees the
# fused map's other views), max 0.26 m; gazebo 2700 beams, median 1.56e-2 m, p90 6.11e-2 m, max 17.3 m (beams through gaps).
SYN_BOUNDS = {"p99": 3.5e-4, "max": 4.8e-3}
BB_BOUNDS = {"median": 3.8e-3, "p90": 0.11}
GZ_BOUNDS = {"median": 0.025, "p90": 0.092}


def test_geometry_synthetic_scene():
    """640 x 480 from the identity pose: hits with var_f <= 0.02 lie between the five frames' analytic surfaces
    z = 1 + 0.05 sin(6 (u + 0.01 f)) cos(5 v), within SYN_BOUNDS."""
    import gpismap_amd
    gm = _synthetic_map()
    depth, rec, st = gm.render_depth(replay.IDENTITY_POSE)
    W, H = 640, 480
    k = np.arange(W * H)
    u = ((k // H) - 310.0) / 568.0
    v = ((k % H) - 224.0) / 568.0
    zf = np.stack([1 + 0.05 * np.sin(6 * (u + 0.01 * f)) * np.cos(5 * v) for f in range(5)])
    conf = (st == 0) & (rec[:, 4] <= 0.02)
    below = zf.min(0) - depth
    above = depth - zf.max(0)
    out = np.maximum(np.maximum(below, above), 0)[conf]
    print("synthetic 640x480: %d hits, %d confident, outside the surfaces' band: median %.2e p99 %.2e max %.2e m"
          % ((st == 0).sum(), conf.sum(), np.median(out), np.percentile(out, 99), out.max()))
    assert conf.sum() > 0.5 * W * H
    assert np.percentile(out, 99) <= SYN_BOUNDS["p99"] and out.max() <= SYN_BOUNDS["max"]


def test_geometry_bigbird():
    """The map of the first five frames rendered at every frame's pose and camera against that frame's measured depth, where
    both are valid (0.4 < z < 4)."""
    gm, frames = _bigbird_map()
    diffs = []
    for fr in frames:
        d, rec, st = gm.render_depth(fr["pose"], cam6=fr["cam"])
        m = fr["depth"]
        ok = (st == 0) & (m > 0.4) & (m < 4.0)
        diffs.append(np.abs(d[ok] - m[ok]).astype(np.float64))
    a = np.concatenate(diffs)
    med, p90 = float(np.median(a)), float(np.percentile(a, 90))
    print("bigbird: %d pixels valid in both, |rendered - measured| median %.3e p90 %.3e max %.3e m" % (a.size, med, p90, a.max()))
    assert a.size > 20000
    assert med <= BB_BOUNDS["median"] and p90 <= BB_BOUNDS["p90"]


def test_geometry_gazebo():
    gm, frames = _gazebo_map()
    diffs = []
    for fr in frames[::3]:
        r, rec, st = gm.render_scan(fr["thetas"], fr["pose"])
        m = fr["ranges"]
        ok = (st == 0) & (m > 0.2) & (m < 30.0)
        diffs.append(np.abs(r[ok] - m[ok]).astype(np.float64))
    a = np.concatenate(diffs)
    med, p90 = float(np.median(a)), float(np.percentile(a, 90))
    print("gazebo: %d beams valid in both, |rendered - measured| median %.3e p90 %.3e max %.3e m" % (a.size, med, p90, a.max()))
    assert a.size > 1000
    assert med <= GZ_BOUNDS["median"] and p90 <= GZ_BOUNDS["p90"]


# ---- round trip -------------------------------------------------------------------------------------------------------------
def test_rendered_depth_feeds_update():
    import gpismap_amd
    gm = _synthetic_map()
    depth, _, st = gm.render_depth(replay.IDENTITY_POSE)
    assert depth.shape == (640 * 480,) and np.count_nonzero(st == 0) > 100000
    fresh = gpismap_amd.GPisMap3()
    fresh.update(depth, replay.IDENTITY_POSE)
    assert fresh.num_points() > 1000
    d2, _, s2 = fresh.render_depth(replay.IDENTITY_POSE)
    both = (st == 0) & (s2 == 0)
    assert both.sum() > 100000
    assert float(np.median(np.abs(d2[both] - depth[both]))) < 2e-3


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors():
    import gpismap_amd
    L = gpismap_amd.lib()
    gm = _synthetic_map(frames=1)
    r = gpismap_amd.Renderer()
    cam = (142.0, 142.0, 77.5, 56.0, 160, 120)
    a = gm.render_depth(replay.IDENTITY_POSE, cam6=cam, renderer=r)
    assert np.count_nonzero(a[2] == 0) > 1000

    def call3(pose=replay.IDENTITY_POSE, cam6=cam, map_h=None, r_h=None, **kw):
        p = np.ascontiguousarray(pose, F32)
        o = gpismap_amd.render_opts(3, **kw)
        c = C.byref(gpismap_amd._cam(cam6)) if cam6 is not None else None
        return L.gpis3_render_depth(gm.h if map_h is None else map_h, r.h if r_h is None else r_h, c,
                                    p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(o), None)

    def still_there():
        assert _same(r.get(), a)

    bad_pose = replay.IDENTITY_POSE.copy(); bad_pose[4] = np.nan
    inf_pose = replay.IDENTITY_POSE.copy(); inf_pose[0] = np.inf
    for kw in (dict(pose=bad_pose), dict(pose=inf_pose), dict(cam6=(0.0, 142.0, 77.5, 56.0, 160, 120)),
               dict(cam6=(142.0, np.nan, 77.5, 56.0, 160, 120)), dict(cam6=(142.0, 142.0, 77.5, 56.0, 0, 120)),
               dict(cam6=(142.0, 142.0, 77.5, 56.0, 160, -1)), dict(tnear=2.0, tfar=1.0), dict(tnear=1.0, tfar=1.0),
               dict(tnear=-0.1), dict(tfar=np.inf), dict(min_step=0.0), dict(max_step=-1.0), dict(min_step=0.1, max_step=0.01),
               dict(far_step=0.0), dict(far_step=np.inf), dict(min_step=np.nan), dict(level=np.inf), dict(max_var=np.nan),
               dict(refine=-1), dict(refine=65), dict(max_steps=0)):
        assert call3(**kw) == -1, kw
        still_there()
    assert L.gpis3_render_depth(gm.h, r.h, None, None, None, None) == -1
    assert L.gpis3_render_depth(None, r.h, None, replay.IDENTITY_POSE.ctypes.data_as(C.POINTER(C.c_float)), None, None) == -1
    assert L.gpis3_render_depth(gm.h, None, None, replay.IDENTITY_POSE.ctypes.data_as(C.POINTER(C.c_float)), None, None) == -1
    still_there()
    # more than 2^26 rays: refused before anything is allocated, the result kept
    assert call3(cam6=(142.0, 142.0, 77.5, 56.0, 8193, 8192)) == -4
    assert call3(cam6=(142.0, 142.0, 77.5, 56.0, 1 << 20, 1 << 20)) == -4
    still_there()
    # 2-D arguments
    g2, f2 = _gazebo_map()
    th, p2 = f2[0]["thetas"], f2[0]["pose"]
    r2 = gpismap_amd.Renderer()
    b = g2.render_scan(th, p2, renderer=r2)
    P = lambda x: np.ascontiguousarray(x, F32).ctypes.data_as(C.POINTER(C.c_float))
    bad_th = th.copy(); bad_th[3] = np.nan
    bad_p2 = p2.copy(); bad_p2[2] = np.inf
    assert L.gpis2_render_scan(g2.h, r2.h, P(bad_th), th.size, P(p2), None, None) == -1
    assert L.gpis2_render_scan(g2.h, r2.h, P(th), th.size, P(bad_p2), None, None) == -1
    assert L.gpis2_render_scan(g2.h, r2.h, P(th), 0, P(p2), None, None) == -1
    assert L.gpis2_render_scan(g2.h, r2.h, None, th.size, P(p2), None, None) == -1
    o = gpismap_amd.render_opts(2, tnear=5.0, tfar=1.0)
    assert L.gpis2_render_scan(g2.h, r2.h, P(th), th.size, P(p2), C.byref(o), None) == -1
    assert _same(r2.get(), b)
    # more than 2^26 beams: refused before thetas is read, also when it holds a NaN (the array is whole, so another order of
    # the checks would read valid memory and return another code); the result kept
    big = np.zeros((1 << 26) + 1, F32)
    assert L.gpis2_render_scan(g2.h, r2.h, P(big), big.size, P(p2), None, None) == -4
    assert _same(r2.get(), b)
    big[2] = np.nan
    assert L.gpis2_render_scan(g2.h, r2.h, P(big), big.size, P(p2), None, None) == -4
    assert _same(r2.get(), b)
    del big
    # the map's own camera when the caller passes none: the same bits as the same values passed
    x = gm.render_depth(replay.IDENTITY_POSE, renderer=r)
    assert x[0].size == 640 * 480 and np.count_nonzero(x[2] == 0) > 1000
    assert _same(gm.render_depth(replay.IDENTITY_POSE, cam6=(568.0, 568.0, 310.0, 224.0, 640, 480), renderer=r), x)
    # a map with no tree: an error, no result
    empty = gpismap_amd.GPisMap3()
    assert call3(map_h=empty.h) == -3
    assert L.gpis_render_get(r.h, None, None, None) == -3
    assert r.device_ptrs() == (0, 0, 0)
    e2 = gpismap_amd.GPisMap()
    with pytest.raises(gpismap_amd.GpisError):
        e2.render_scan(th, p2, renderer=r2)
    assert L.gpis_render_get(r2.h, None, None, None) == -3
    with pytest.raises(gpismap_amd.GpisError):
        gm.render_depth(replay.IDENTITY_POSE, bogus=1.0)
    assert L.gpis_render_set_chunk(r.h, -1) == -1
    # after an error the renderer works again
    assert _same(gm.render_depth(replay.IDENTITY_POSE, cam6=cam, renderer=r), a)
