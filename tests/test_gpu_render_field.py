"""Rendering from a distance field on the GPU (csrc/render.hip, gpis3_render_depth_field / gpis2_render_scan_field): the device
call against the numpy reference (tests/render_field_ref.py) bit for bit, at kernel level (analytic f grids through from_grid)
and at map level (the fields of the synthetic, bigbird and gazebo maps); determinism across runs, streams, thread-to-pixel
mappings, a renderer that held a map render and a two-device map; the depth against the map renderer on the same pose; a rendered
image tracked back to its pose; the map renderer unchanged by a field render on the same Renderer; the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_ref
import render_field_ref
import replay
import track_field_ref
from test_gpu_dfield import BOX2, BOX3, SYN, _bigbird_map, _gazebo_map
from test_gpu_track import SYN_CAM, SYN_TRUE, _synthetic_map
from test_track_ref import CAM, OFF2, pose6, pose12, rot, scene2, scene3

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32

# analytic lattices (as tests/test_track_field_ref.py)
LAT3 = dict(shape=(131, 101, 48), origin=(-1.3, -1.0, 0.8), step=0.02)
LAT2 = dict(shape=(396, 231), origin=(-3.2, -1.9), step=0.02)
T3 = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
T2 = pose6(0.15, (0.3, -0.2))
THETAS = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)
CAM640 = (568.0, 568.0, 310.0, 224.0, 640, 480)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _same(x, y):
    return _bits_equal(x[0], y[0]) and _bits_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


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
    return df.get()[0].ravel(), i["shape"], i["origin"], i["step"]


def _counters(r):
    i = r.info()
    return int(i["samples"]), int(i["hits"]), int(i["max_samples"])


def _check_bits(out, r, ref, what):
    d, rec, st, stats = ref
    info = r.info()
    print("%s: %d rays, %d hits, %d samples (%.2f per ray, max %d), status counts %s"
          % (what, d.size, stats["hits"], stats["samples"], stats["samples"] / d.size, stats["max_samples"], np.bincount(st, minlength=3)))
    assert info["field"] == 1 and info["valid"] == 1 and info["rays"] == d.size and info["evals"] == 0
    assert np.array_equal(out[2], st), (what, np.bincount(out[2]), np.bincount(st))
    assert _bits_equal(out[0], d), what
    assert out[1].shape == rec.shape and _bits_equal(out[1], rec), what
    assert _counters(r) == (stats["samples"], stats["hits"], stats["max_samples"]), what


def _both3(df, pose, cam, r=None, **kw):
    import gpismap_amd
    r = r or gpismap_amd.Renderer()
    out = df.render_depth(pose, cam, renderer=r, **kw)
    dist, shape, origin, step = _lat(df)
    return out, r, render_field_ref.render_depth(dist, shape, origin, step, cam, pose, **kw)


def _both2(df, thetas, pose, off2, r=None, **kw):
    import gpismap_amd
    r = r or gpismap_amd.Renderer()
    out = df.render_scan(thetas, pose, off2, renderer=r, **kw)
    dist, shape, origin, step = _lat(df)
    return out, r, render_field_ref.render_scan(dist, shape, origin, step, thetas, pose, off2, **kw)


# ---- bits -----------------------------------------------------------------------------------------------------------------
def test_bits_kernel_level_3d():
    df = _grid_field(scene3, LAT3)
    inside = pose12(np.eye(3), np.array([0.1, -0.05, 1.1]))                     # the centre of the sphere
    away = pose12(rot([0, 1, 0], math.pi), np.array([0.0, 0.0, 0.5]))           # in front of the lattice, looking away from it
    cases = [(T3, CAM, {}), (T3, CAM, dict(refine=0)), (T3, CAM, dict(refine=3, slack=0.0)), (T3, CAM, dict(max_steps=5)),
             (T3, CAM, dict(max_steps=1)), (inside, CAM, dict(tnear=0.01)), (away, CAM, {}),
             (T3, (400.0, 400.0, 319.5, 239.5, 640, 480), dict(min_step=0.004, max_step=0.25)),
             (T3, (61.0, 59.0, 20.3, 17.1, 43, 37), {})]                        # an image no tile size divides
    seen = set()
    for pose, cam, kw in cases:
        out, r, ref = _both3(df, pose, cam, **kw)
        _check_bits(out, r, ref, "analytic 3-D %dx%d %s" % (cam[4], cam[5], kw))
        seen |= set(np.unique(ref[2]).tolist())
        lo, hi = render_field_ref.box(LAT3["shape"], LAT3["origin"], LAT3["step"])
        assert _bits_equal(r.box()[0], lo) and _bits_equal(r.box()[1], hi)
    assert seen == {0, 1, 2}
    out, r, ref = _both3(df, away, CAM)
    assert np.all(out[2] == 1) and _counters(r) == (0, 0, 0)
    out, r, ref = _both3(df, T3, CAM, max_steps=1)
    assert np.all(out[2] == 2) and _counters(r) == (out[2].size, 0, 1)
    out, r, ref = _both3(df, inside, CAM, tnear=0.01)
    assert np.count_nonzero(out[2] == 0) > 2000


def test_bits_kernel_level_2d():
    df = _grid_field(scene2, LAT2)
    inside = pose6(0.0, (2.0 - OFF2[0], 0.6))                                   # the sensor at the centre of the pillar
    for pose, off2, kw in ((T2, OFF2, {}), (T2, (0.0, 0.05), dict(refine=0)), (T2, OFF2, dict(max_steps=4)),
                           (inside, OFF2, dict(tnear=0.01)), (pose6(0.3, (20.0, 0.0)), OFF2, {}),
                           (T2, OFF2, dict(slack=1.0, min_step=0.003, max_step=0.5, refine=12))):
        out, r, ref = _both2(df, THETAS, pose, off2, **kw)
        _check_bits(out, r, ref, "analytic 2-D offset %s %s" % (off2, kw))
    out, r, ref = _both2(df, THETAS, T2, OFF2)
    assert np.all(out[2] == 0) and out[1].shape == (360, 3)


def test_bits_map_level():
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    for pose, cam in ((replay.IDENTITY_POSE, CAM640), (SYN_TRUE, SYN_CAM)):
        out, r, ref = _both3(df, pose, cam)
        assert np.count_nonzero(out[2] == 0) > 0.5 * out[2].size
        _check_bits(out, r, ref, "synthetic field %dx%d" % (cam[4], cam[5]))
    # through the map's entry with the map's camera: the same bits
    assert _same(gm.render_depth_field(df, replay.IDENTITY_POSE), df.render_depth(replay.IDENTITY_POSE, CAM640))
    frames = replay.load_bigbird()
    gb = _bigbird_map()
    dfb = gb.distance_field(**BOX3)
    for i in (0, 2, 4):
        out, r, ref = _both3(dfb, frames[i]["pose"], frames[i]["cam"])
        assert np.count_nonzero(out[2] == 0) > 1000
        _check_bits(out, r, ref, "bigbird field, pose of frame %d" % i)
    f2 = replay.load_gazebo()
    g2 = _gazebo_map()
    df2 = g2.distance_field(**BOX2)
    import gpismap_amd
    for i in (0, len(f2) // 2, len(f2) - 1):
        fr = f2[i]
        r = gpismap_amd.Renderer()
        out = g2.render_scan_field(df2, fr["thetas"], fr["pose"], renderer=r)
        dist, shape, origin, step = _lat(df2)
        ref = render_field_ref.render_scan(dist, shape, origin, step, fr["thetas"], fr["pose"], OFF2)
        assert np.count_nonzero(out[2] == 0) > 100
        _check_bits(out, r, ref, "gazebo field, pose of scan %d" % i)


# ---- invariance -----------------------------------------------------------------------------------------------------------
def _call3(L, map_h, df, r, pose, cam6=None, stream=None, **kw):
    import gpismap_amd
    p = np.ascontiguousarray(pose, F32)
    step = df.info()["step"] if df is not None and df.info()["dim"] else 0.01
    o = gpismap_amd.render_field_opts(3, step, **kw)
    c = C.byref(gpismap_amd._cam(cam6)) if cam6 is not None else None
    return L.gpis3_render_depth_field(map_h, df.h if df is not None else None, r.h if r is not None else None, c,
                                      p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(o), stream)


def _call2(L, map_h, df, r, thetas, pose, off2=None, stream=None, **kw):
    import gpismap_amd
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    th, p = np.ascontiguousarray(thetas, F32), np.ascontiguousarray(pose, F32)
    off = np.ascontiguousarray(off2, F32) if off2 is not None else None
    step = df.info()["step"] if df is not None and df.info()["dim"] else 0.1
    o = gpismap_amd.render_field_opts(2, step, **kw)
    return L.gpis2_render_scan_field(map_h, df.h if df is not None else None, r.h, P(th), th.size,
                                     P(off) if off is not None else None, P(p), C.byref(o), stream)


def test_deterministic_across_runs_streams_mappings_and_renderers():
    import gpismap_amd
    import torch
    L = gpismap_amd.lib()
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    r = gpismap_amd.Renderer()
    a = df.render_depth(SYN_TRUE, CAM640, renderer=r)
    ca = _counters(r)
    assert np.count_nonzero(a[2] == 0) > 100000
    others = [(df.render_depth(SYN_TRUE, CAM640, renderer=r), _counters(r))]
    # a caller stream against the field's own
    s = torch.cuda.Stream(device=0)
    r2 = gpismap_amd.Renderer()
    assert _call3(L, None, df, r2, SYN_TRUE, cam6=CAM640, stream=C.c_void_p(s.cuda_stream)) == 0
    others.append((r2.get(), _counters(r2)))
    # the other thread-to-pixel mapping
    r3 = gpismap_amd.Renderer()
    r3.set_field_tiles(False)
    others.append((df.render_depth(SYN_TRUE, CAM640, renderer=r3), _counters(r3)))
    # a renderer that held a map render before (another size, the wider record)
    r4 = gpismap_amd.Renderer()
    m = gm.render_depth(SYN_TRUE, cam6=SYN_CAM, renderer=r4)
    assert m[1].shape[1] == 8 and r4.info()["field"] == 0
    others.append((df.render_depth(SYN_TRUE, CAM640, renderer=r4), _counters(r4)))
    assert r4.info()["field"] == 1
    # a field of the same map built again, and by a map on one device listed twice
    for g in (_synthetic_map(), _synthetic_map(devices=[0, 0])):
        rr = gpismap_amd.Renderer()
        others.append((g.render_depth_field(g.distance_field(**SYN), SYN_TRUE, renderer=rr), _counters(rr)))
    for o, c in others:
        assert _same(o, a) and c == ca
    # 2-D
    f2 = replay.load_gazebo()
    g2, s2 = _gazebo_map(), _gazebo_map(pipeline=False)
    th, p2 = f2[5]["thetas"], f2[5]["pose"]
    x = g2.render_scan_field(g2.distance_field(**BOX2), th, p2)
    y = g2.render_scan_field(g2.distance_field(**BOX2), th, p2, renderer=gpismap_amd.Renderer())
    z = s2.render_scan_field(s2.distance_field(**BOX2), th, p2)
    assert np.count_nonzero(x[2] == 0) > 100 and _same(x, y) and _same(x, z)


def test_two_device_map():
    import gpismap_amd
    if gpismap_amd.device_count() < 2:
        pytest.skip("one device")
    frames = replay.load_bigbird()
    a, b = _bigbird_map(), _bigbird_map(devices=[0, 1])
    pose, cam = frames[2]["pose"], frames[2]["cam"]
    x = a.render_depth_field(a.distance_field(**BOX3), pose, cam6=cam)
    y = b.render_depth_field(b.distance_field(**BOX3), pose, cam6=cam)
    assert np.count_nonzero(x[2] == 0) > 1000 and _same(x, y)


def test_map_renderer_unchanged_by_a_field_render_on_the_same_renderer():
    import gpismap_amd
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    fresh_r = gpismap_amd.Renderer()
    fresh = gm.render_depth(SYN_TRUE, cam6=SYN_CAM, renderer=fresh_r)
    r = gpismap_amd.Renderer()
    before = gm.render_depth(SYN_TRUE, cam6=SYN_CAM, renderer=r)
    i0 = r.info()
    f1 = df.render_depth(SYN_TRUE, SYN_CAM, renderer=r)
    after = gm.render_depth(SYN_TRUE, cam6=SYN_CAM, renderer=r)
    i1 = r.info()
    f2 = df.render_depth(SYN_TRUE, SYN_CAM, renderer=r)
    assert _same(before, fresh) and _same(after, fresh) and _same(f1, f2)
    assert before[1].shape[1] == 8 and f1[1].shape[1] == 4
    for k in ("passes", "march_passes", "samples", "evals", "hits", "field", "max_samples"):
        assert i0[k] == i1[k] == fresh_r.info()[k], k
    assert i1["passes"] > 10 and i1["field"] == 0


# ---- against the map renderer -----------------------------------------------------------------------------------------------
# The field render against the map render on the same pose, for the rays that hit in both (the field built without a variance
# gate, as the map render's max_var = +inf), |depth difference| along the ray in lattice steps of the field (0.3 / 32 m).
# Measured on an MI355X: median 0.0725, p99 0.5589 (max 1.56), 291 333 rays hit in both (the map 292 990, the field
# 291 333); guarded with the usual 1.5x margin.
VS_MAP_BOUNDS = {"median": 0.109, "p99": 0.839}


def test_depth_against_the_map_renderer_synthetic():
    gm = _synthetic_map()
    df = gm.distance_field(**SYN)
    pose = SYN_TRUE
    dm, _, sm = gm.render_depth(pose, cam6=CAM640)
    dfd, rec, sf = df.render_depth(pose, CAM640)
    both = (sm == 0) & (sf == 0)
    u = (np.arange(640 * 480) // 480 - CAM640[2]) / CAM640[0]
    v = (np.arange(640 * 480) % 480 - CAM640[3]) / CAM640[1]
    arc = np.sqrt(u * u + v * v + 1.0)
    e = np.abs(dfd[both].astype(np.float64) - dm[both]) * arc[both] / df.info()["step"]
    print("synthetic 640x480: map hits %d, field hits %d, both %d; |depth difference| in steps: median %.4f p90 %.4f p99 %.4f max %.4f"
          % ((sm == 0).sum(), (sf == 0).sum(), both.sum(), np.median(e), np.quantile(e, 0.9), np.quantile(e, 0.99), e.max()))
    assert both.sum() > 0.9 * max((sm == 0).sum(), (sf == 0).sum())
    assert np.median(e) <= VS_MAP_BOUNDS["median"] and np.quantile(e, 0.99) <= VS_MAP_BOUNDS["p99"]


# ---- closed loop ------------------------------------------------------------------------------------------------------------
def test_rendered_depth_tracks_back_to_its_pose():
    """A depth image rendered from a field at T, tracked against the same field from T.  Both calls match their references bit for
    bit, so this is a property of the references: the device result is asserted against track_field_ref on the rendered image,
    which on the analytic field converges (status 0) at T in one iteration."""
    df = _grid_field(scene3, LAT3)
    gm = _synthetic_map()
    dfs = gm.distance_field(**SYN)
    for what, f, T, cam in (("analytic", df, T3, CAM), ("synthetic", dfs, SYN_TRUE, SYN_CAM)):
        depth, rec, st = f.render_depth(T, cam)
        assert np.count_nonzero(st == 0) > 0.5 * st.size
        pose, info = f.track_depth(depth, T, cam)
        dist, shape, origin, step = _lat(f)
        ref = track_field_ref.track_depth(dist, shape, origin, step, depth, cam, T)
        dt = float(np.linalg.norm(pose[:3].astype(np.float64) - T[:3]))
        print("closed loop, %s: status %d, %d iterations, %d inliers of %d, cost %.3e -> %.3e, moved %.2e m"
              % (what, info["status"], info["iterations"], info["inliers"], info["points"], info["cost0"], info["cost"], dt))
        assert (info["status"], info["iterations"], info["passes"], info["points"], info["inliers"]) == \
            (ref["status"], ref["iterations"], ref["passes"], ref["points"], ref["inliers"])
        assert _bits_equal(pose, ref["pose"]) and _bits_equal(info["resid"], ref["resid"])
        if what == "analytic":
            assert info["status"] == 0 and info["inliers"] == info["points"] and dt < 1e-3 * step
    # the rendered image is a valid update() frame
    g2 = _synthetic_map(frames=0)
    g2.set_camera(SYN_CAM)
    g2.update(depth, SYN_TRUE)
    assert g2.num_points() > 100


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_and_map_defaults():
    import gpismap_amd
    L = gpismap_amd.lib()
    gm = _synthetic_map(frames=2)
    df = gm.distance_field(**SYN)
    cam = (142.0, 142.0, 77.5, 56.0, 160, 120)
    r = gpismap_amd.Renderer()
    a = df.render_depth(SYN_TRUE, cam, renderer=r)
    ca = _counters(r)
    assert np.count_nonzero(a[2] == 0) > 5000

    def still_there():
        assert _same(r.get(), a) and _counters(r) == ca and r.info()["field"] == 1

    bad_pose = SYN_TRUE.copy(); bad_pose[4] = np.nan
    for kw in (dict(pose=bad_pose), dict(cam6=(0.0, 142.0, 77.5, 56.0, 160, 120)), dict(cam6=(142.0, 142.0, 77.5, 56.0, 0, 120)),
               dict(tnear=np.nan), dict(tfar=np.inf), dict(tnear=2.0, tfar=1.0), dict(tnear=1.0, tfar=1.0), dict(tnear=-0.1),
               dict(min_step=0.0), dict(min_step=-1.0), dict(min_step=np.nan), dict(min_step=np.inf),
               dict(min_step=0.1, max_step=0.01), dict(max_step=np.nan), dict(slack=-0.5), dict(slack=np.inf), dict(slack=np.nan),
               dict(refine=-1), dict(refine=65), dict(max_steps=0)):
        args = dict(pose=SYN_TRUE, cam6=cam)
        args.update(kw)
        pose = args.pop("pose")
        assert _call3(L, gm.h, df, r, pose, **args) == -1, kw
        still_there()
    assert _call3(L, None, df, r, SYN_TRUE, cam6=None) == -1                 # no camera without a map
    assert _call3(L, gm.h, None, r, SYN_TRUE, cam6=cam) == -1                # no field
    assert _call3(L, gm.h, df, None, SYN_TRUE, cam6=cam) == -1               # no renderer
    assert L.gpis3_render_depth_field(gm.h, df.h, r.h, None, None, None, None) == -1     # no pose
    still_there()
    # a field of the other dim: an argument error; a field without a result: a state error; too many rays: a limit error
    f2 = replay.load_gazebo()
    g2 = _gazebo_map()
    df2 = g2.distance_field(**BOX2)
    assert _call3(L, gm.h, df2, r, SYN_TRUE, cam6=cam) == -1
    still_there()
    nores = gpismap_amd.DistanceField()
    assert _call3(L, gm.h, nores, r, SYN_TRUE, cam6=cam) == -3
    still_there()
    assert _call3(L, gm.h, df, r, SYN_TRUE, cam6=(142.0, 142.0, 77.5, 56.0, 8193, 8192)) == -4
    assert _call3(L, gm.h, df, r, SYN_TRUE, cam6=(142.0, 142.0, 77.5, 56.0, 1 << 20, 1 << 20)) == -4
    still_there()
    with pytest.raises(gpismap_amd.GpisError):
        df.render_depth(SYN_TRUE[:-1], cam)
    with pytest.raises(gpismap_amd.GpisError):
        df.render_depth(SYN_TRUE, cam, no_such_option=1)
    with pytest.raises(gpismap_amd.GpisError):
        nores.render_depth(SYN_TRUE, cam)
    o = gpismap_amd.gpis_render_field_opts()
    assert L.gpis_render_field_default_opts(3, 0.0, C.byref(o)) == -1 and L.gpis_render_field_default_opts(4, 0.01, C.byref(o)) == -1
    assert L.gpis_render_field_default_opts(3, 0.01, None) == -1
    assert L.gpis_render_field_default_opts(2, 0.1, C.byref(o)) == 0
    assert (o.tnear, o.tfar, o.max_steps, o.refine, o.slack, o.max_step) == (F32(0.2), 30.0, 1024, 8, 3.0, np.inf)
    assert o.min_step == F32(0.1) * F32(0.5)
    # 2-D
    fr = f2[3]
    r2 = gpismap_amd.Renderer()
    b = g2.render_scan_field(df2, fr["thetas"], fr["pose"], renderer=r2)
    assert np.count_nonzero(b[2] == 0) > 100 and b[1].shape[1] == 3
    assert _call2(L, None, df2, r2, fr["thetas"], fr["pose"]) == -1            # no offset without a map
    assert _call2(L, g2.h, df, r2, fr["thetas"], fr["pose"]) == -1             # a 3-D field
    assert _call2(L, g2.h, nores, r2, fr["thetas"], fr["pose"]) == -3
    bad_th = fr["thetas"].copy(); bad_th[2] = np.nan
    assert _call2(L, g2.h, df2, r2, bad_th, fr["pose"]) == -1
    assert _call2(L, g2.h, df2, r2, fr["thetas"], fr["pose"], slack=-1.0) == -1
    assert _same(r2.get(), b)
    # more than 2^26 beams: refused before thetas is read, also when it holds a NaN (the array is whole, so another order of
    # the checks would read valid memory and return another code); the result kept
    big = np.zeros((1 << 26) + 1, F32)
    assert _call2(L, g2.h, df2, r2, big, fr["pose"]) == -4
    assert _same(r2.get(), b)
    big[2] = np.nan
    assert _call2(L, g2.h, df2, r2, big, fr["pose"]) == -4
    assert _same(r2.get(), b)
    del big
    # the map's camera / sensor offset when the caller passes none: the same bits as passing them
    assert _call3(L, gm.h, df, r, SYN_TRUE) == 0
    x = r.get()
    assert _call3(L, None, df, r, SYN_TRUE, cam6=CAM640) == 0
    assert x[0].size == 640 * 480 and _same(r.get(), x)
    assert _call2(L, g2.h, df2, r2, fr["thetas"], fr["pose"]) == 0
    y = r2.get()
    assert _call2(L, None, df2, r2, fr["thetas"], fr["pose"], off2=OFF2) == 0
    assert _same(r2.get(), y) and _same(y, b)
    # after the errors the renderer works again
    assert _same(df.render_depth(SYN_TRUE, cam, renderer=r), a)
