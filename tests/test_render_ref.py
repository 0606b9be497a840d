"""The renderer's numpy reference (tests/render_ref.py) on analytic fields and on a small oracle map, and the renderer's C-ABI
symbols.  CPU only."""
import ctypes as C
import os

import numpy as np
import oracle_lib
import render_ref
import replay

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpismap_amd", "libgpismap_amd.so")

SPHERE_C, SPHERE_R = np.array([0.1, -0.05, 1.2]), 0.3
SLAB_Z, SLAB_H = 1.8, 0.05
FIELD_LO, FIELD_HI = np.array([-1.0, -1.0, 0.3]), np.array([1.0, 1.0, 2.2])   # f is NaN outside
CAM = (30.0, 30.0, 15.5, 11.5, 32, 24)


def analytic_fn(field, var=0.01):
    """test_fn of an analytic f (float64 in, float32 record): NaN outside FIELD_LO..FIELD_HI, gradient zero, var_f = var."""
    def fn(x, res):
        p = x.astype(np.float64)
        inside_box = np.all((p >= FIELD_LO) & (p <= FIELD_HI), axis=1)
        f = field(p)
        res[inside_box, 0] = f[inside_box].astype(F32)
        res[:, 4] = F32(var)
        return res
    return fn


def sphere_slab(p):
    return np.minimum(np.linalg.norm(p - SPHERE_C, axis=1) - SPHERE_R, np.abs(p[:, 2] - SLAB_Z) - SLAB_H)


def _box():
    return FIELD_LO.astype(F32) - F32(0.075), FIELD_HI.astype(F32) + F32(0.075)


def _opts(**kw):
    o = render_ref.Opts(3, level=0.0, far_step=0.9 * 0.075, **kw)
    return o


def test_analytic_sphere_and_slab_hits():
    """Every ray of a 32 x 24 camera at the origin hits the sphere or the slab, at the analytic depth within the refinement
    tolerance (8 bisections of a <= 0.01 bracket, then the secant point: 2e-5 in z)."""
    depth, rec, status, st = render_ref.render_depth(analytic_fn(sphere_slab), CAM, replay.IDENTITY_POSE, _box(), _opts())
    assert np.all(status == 0), np.bincount(status)
    u, v, il, _, _ = render_ref.rays3(CAM, replay.IDENTITY_POSE)
    w = np.stack([u, v, np.ones_like(u)], axis=1).astype(np.float64)
    ww = (w * w).sum(1)
    wc = w @ SPHERE_C
    disc = wc ** 2 - ww * (SPHERE_C @ SPHERE_C - SPHERE_R ** 2)
    zs = np.where(disc > 0, (wc - np.sqrt(np.maximum(disc, 0))) / ww, np.inf)
    z_true = np.minimum(zs, SLAB_Z - SLAB_H)
    err = np.abs(depth.astype(np.float64) - z_true)
    print("analytic: %d rays, %d passes, max |z - z_true| %.2e" % (depth.size, st["passes"], err.max()))
    assert (zs < np.inf).sum() > 50 and (zs == np.inf).sum() > 50
    assert err.max() < 2e-5
    assert np.all(np.abs(rec[:, 0]) < 2e-5)
    assert st["hits"] == depth.size


def test_grazing_rays_stop_at_the_step_limit():
    """A ray along z at x = 0 beside the plane x = 5e-4: g stays 5e-4, every step is min_step, and the 3.6 m interval needs
    far more than max_steps samples -> status 2.  Far from the plane (g = 1) the same ray leaves the interval: status 1."""
    cam = (1.0, 1.0, 0.0, 0.0, 1, 1)
    box = (np.array([-1, -1, 0], F32), np.array([1, 1, 5], F32))
    lo, hi = FIELD_LO.copy(), FIELD_HI.copy()
    try:
        FIELD_LO[:], FIELD_HI[:] = (-1, -1, 0), (1, 1, 5)
        d, r, s, st = render_ref.render_depth(analytic_fn(lambda p: np.abs(p[:, 0] - 5e-4)), cam, replay.IDENTITY_POSE, box,
                                              _opts(max_steps=100))
        assert s[0] == 2 and np.isnan(d[0]) and np.all(np.isnan(r[0])) and st["march_passes"] == 100
        d, r, s, st = render_ref.render_depth(analytic_fn(lambda p: np.abs(p[:, 0] - 1.0)), cam, replay.IDENTITY_POSE, box,
                                              _opts())
        assert s[0] == 1 and 355 <= st["march_passes"] <= 365 and st["march_passes"] < 512
    finally:
        FIELD_LO[:], FIELD_HI[:] = lo, hi


def test_rays_starting_inside_are_not_hits():
    """The camera inside a sphere of radius 1: the first samples are inside, leaving the sphere is no hit, the slab behind it is."""
    def field(p):
        return np.minimum(np.linalg.norm(p, axis=1) - 1.0, np.abs(p[:, 2] - SLAB_Z) - SLAB_H)
    depth, rec, status, _ = render_ref.render_depth(analytic_fn(field), CAM, replay.IDENTITY_POSE, _box(), _opts())
    assert np.all(status == 0)
    assert np.all(np.abs(depth - (SLAB_Z - SLAB_H)) < 2e-5)
    # inside everywhere: never a hit
    _, _, s2, _ = render_ref.render_depth(analytic_fn(lambda p: -np.ones(p.shape[0])), CAM, replay.IDENTITY_POSE, _box(), _opts())
    assert np.all(s2 == 1)
    # a crossing whose variance fails max_var does not count
    _, _, s3, _ = render_ref.render_depth(analytic_fn(sphere_slab, var=0.5), CAM, replay.IDENTITY_POSE, _box(), _opts(max_var=0.1))
    assert np.all(s3 == 1)


def test_empty_box_is_a_miss_without_a_pass():
    calls = []
    d, r, s, st = render_ref.render_depth(lambda x, res: calls.append(1), CAM, replay.IDENTITY_POSE, None, _opts())
    assert not calls and np.all(s == 1) and np.all(np.isnan(d)) and st["passes"] == 0


def test_2d_reference_on_a_circle():
    """2-D: a circle of radius 2 around the sensor (offset 0.08, 0), beams over 270 degrees: ranges at the analytic distance."""
    th = np.linspace(-2.35, 2.35, 91).astype(F32)
    pose = np.array([0.5, -0.3, 1, 0, 0, 1], F32)
    ctr = np.array([0.5, -0.3])

    def fn(x, res):
        res[:, 0] = (np.linalg.norm(x.astype(np.float64) - ctr, axis=1) - 2.0).astype(F32) * -1
        res[:, 3] = F32(0.01)
        return res
    o = render_ref.Opts(2, level=0.0, far_step=4.32)
    box = (np.array([-3, -4], F32), np.array([4, 3], F32))
    rng, rec, st, _ = render_ref.render_scan(fn, th, pose, (0.08, 0.0), box, o)
    # inside the circle -> f > 0 here (outside of the surface), the circle is crossed going out: a hit
    assert np.all(st == 0)
    ang = th.astype(np.float64)
    ox = 0.08
    b = ox * np.cos(ang)
    r_true = -b + np.sqrt(b * b - (ox * ox - 4.0))
    assert np.max(np.abs(rng - r_true)) < 1e-4


def test_oracle_map_hits_are_on_the_level():
    """bigbird frame 0 in the CPU oracle, its camera scaled to 64 x 48, from the frame's pose: every hit record has |g| below
    the tolerance of the refinement."""
    fr = replay.load_bigbird()[0]
    om = oracle_lib.OracleMap3(fr["cam"])
    om.update(fr["depth"], fr["pose"])
    c = fr["cam"]
    cam = (c[0] / 10, c[1] / 10, c[2] / 10, c[3] / 10, 64, 48)

    def fn(x, res):
        ok = om.L.orc3_test(om.h, x.ctypes.data_as(C.POINTER(C.c_float)), 3, x.shape[0], res.ctypes.data_as(C.POINTER(C.c_float)))
        assert ok
        return res
    # a box around the frame's points: cluster cells (0.05) plus the search half-width (0.075)
    d, pose = fr["depth"], fr["pose"]
    k = np.nonzero((d > 0.4) & (d < 4.0))[0]
    u, v, _, _, _ = render_ref.rays3(fr["cam"], pose)
    pts = render_ref.points3(u, v, pose, k, d[k])
    box = (pts.min(0) - F32(0.125), pts.max(0) + F32(0.125))
    o = render_ref.Opts(3, level=-0.2, far_step=0.9 * 0.075)
    depth, rec, status, st = render_ref.render_depth(fn, cam, pose, box, o)
    hit = status == 0
    g = rec[hit, 0] + F32(0.2)
    print("oracle 64x48: %d hits, %d passes, %d samples, max |g| %.2e" % (hit.sum(), st["passes"], st["samples"], np.abs(g).max()))
    assert hit.sum() > 60          # (the object covers about 3.5 % of the image: 121 hits measured)
    assert np.abs(g).max() < 1e-4    # (measured 9.2e-7)
    assert np.all(np.isnan(depth[~hit]))


def test_render_symbols_exported():
    L = C.CDLL(LIB)
    for name in ("gpis_render_create", "gpis_render_destroy", "gpis_render_set_chunk", "gpis_render_default_opts",
                 "gpis3_render_depth", "gpis2_render_scan", "gpis_render_get", "gpis_render_device", "gpis_render_info"):
        assert hasattr(L, name), name
