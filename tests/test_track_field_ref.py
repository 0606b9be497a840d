"""The field-tracking reference (tests/track_field_ref.py) on the CPU: fields built by dfield_ref from the f of the analytic scenes
of test_track_ref.py, pose recovery in 3-D and 2-D to within half a lattice step, the Jacobian of the field residual against
finite differences away from cell faces, and the C-ABI's two new symbols."""
import math
import os

import numpy as np

import dfield_ref
import mesh_ref
import track_field_ref
import track_ref
from test_track_ref import CAM, OFF2, depth_image, pose6, pose12, pose_error3, rot, scan, scene2, scene3

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lattices around what the scenes' sensors see (cubic cells, <= 2 M points)
LAT3 = dict(shape=(131, 101, 48), origin=(-1.3, -1.0, 0.8), step=0.02)      # 635 088 points
LAT2 = dict(shape=(396, 231), origin=(-3.2, -1.9), step=0.02)               # 91 476 points


def _field(scene, lat):
    x = mesh_ref.lattice(lat["shape"], lat["origin"], [lat["step"]] * len(lat["shape"]))
    f = scene(x.astype(np.float64))[0].astype(F32)
    dist, site = dfield_ref.distance_field(f, lat["shape"], lat["origin"], lat["step"], 0.0)
    assert np.count_nonzero(site == np.arange(site.size)) > 1000
    return dist


_CACHE = {}


def field3():
    if "3" not in _CACHE:
        _CACHE["3"] = _field(scene3, LAT3)
    return _CACHE["3"]


def field2():
    if "2" not in _CACHE:
        _CACHE["2"] = _field(scene2, LAT2)
    return _CACHE["2"]


def test_recovers_a_known_pose_3d():
    dist = field3()
    T_true = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
    depth = depth_image(scene3, CAM, T_true)
    start = pose12(rot([0.4, -1, 0.7], math.radians(2.0)) @ np.asarray(T_true[3:], np.float64).reshape(3, 3).T,
                   np.asarray(T_true[:3], np.float64) + np.array([0.0128, -0.0102, 0.0115]))
    out = track_field_ref.track_depth(dist, LAT3["shape"], LAT3["origin"], LAT3["step"], depth, CAM, start, stride=1)
    e0, e = pose_error3(start, T_true), pose_error3(out["pose"], T_true)
    print("3-D field: start %.4f m %.3f deg -> %.2e m %.3f deg, status %d, %d iterations, %d inliers of %d"
          % (e0[0], math.degrees(e0[1]), e[0], math.degrees(e[1]), out["status"], out["iterations"], out["inliers"], out["points"]))
    assert e0[0] > 0.019 and math.degrees(e0[1]) > 1.99
    assert out["status"] == 0 and out["passes"] == out["iterations"] + 1
    assert e[0] < 0.5 * LAT3["step"] and math.degrees(e[1]) < 0.5
    assert out["cost"] < out["cost0"]


def test_recovers_a_known_pose_2d():
    dist = field2()
    th = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)
    T_true = pose6(0.15, (0.3, -0.2))
    ranges = scan(scene2, th, T_true)
    start = pose6(0.15 + math.radians(2.0), (0.3 + 0.015, -0.2 - 0.013))
    out = track_field_ref.track_scan(dist, LAT2["shape"], LAT2["origin"], LAT2["step"], th, ranges, start, OFF2)
    P = out["pose"].astype(np.float64)
    et = float(np.hypot(P[0] - T_true[0], P[1] - T_true[1]))
    er = abs(math.atan2(P[3], P[2]) - 0.15)
    print("2-D field: status %d, %d iterations, error %.2e m %.3f deg" % (out["status"], out["iterations"], et, math.degrees(er)))
    assert out["status"] == 0
    assert et < 0.5 * LAT2["step"] and math.degrees(er) < 0.5


def test_field_residual_is_the_sampled_distance():
    """One evaluate-only call by hand: r = d, no variance test, points outside the lattice are no inliers."""
    dist = field3()
    depth = depth_image(scene3, CAM, pose12(np.eye(3), np.zeros(3)))
    T = pose12(rot([0, 1, 0], 0.01), np.array([0.0, 0.0, 0.01]))
    o = track_field_ref.opts(3, stride=2, max_iters=0)
    assert o.level == 0.0 and o.max_var == math.inf
    out = track_field_ref.track_depth(dist, LAT3["shape"], LAT3["origin"], LAT3["step"], depth, CAM, T, stride=2, max_iters=0)
    loc, pix = track_ref.points3(depth, CAM, 2)
    x = track_ref.world(loc, [float(v) for v in T], 3)
    s = dfield_ref.sample(dist, LAT3["shape"], LAT3["origin"], LAT3["step"], x)
    inl = np.all(np.isfinite(s), axis=1) & (np.abs(s[:, 0].astype(np.float64)) <= o.max_residual)
    assert out["inliers"] == inl.sum() > 1000
    assert np.array_equal(out["resid"][pix[inl]].view(np.uint32), s[inl, 0].view(np.uint32))
    assert np.count_nonzero(np.isfinite(out["resid"])) == inl.sum()


def test_jacobian_matches_finite_differences():
    """Away from cell faces (every u within [0.1, 0.9] of its cell, a step of 1e-4 m stays in the cell) the Jacobian from the
    sampled gradient is the derivative of the sampled distance under the pose update."""
    rng = np.random.default_rng(5)
    for dim, lat, dist in ((3, LAT3, field3()), (2, LAT2, field2())):
        if dim == 3:
            P = [float(v) for v in pose12(rot([0.3, -1, 0.2], 0.05), np.array([0.02, -0.01, 0.03]))]
            loc = np.stack([rng.uniform(-0.5, 0.5, 4000), rng.uniform(-0.4, 0.4, 4000), rng.uniform(0.9, 1.5, 4000)], 1).astype(F32)
        else:
            P = [float(v) for v in pose6(0.1, (0.2, -0.1))]
            loc = np.stack([rng.uniform(-2, 3, 4000), rng.uniform(-1, 1.5, 4000)], 1).astype(F32)
        nj = 6 if dim == 3 else 3
        shape, origin, step = lat["shape"], lat["origin"], lat["step"]
        x = track_ref.world(loc, P, dim)
        u = (x.astype(np.float64) - np.asarray(origin)) / step
        fr = u - np.floor(u)
        keep = np.all((fr > 0.1) & (fr < 0.9), axis=1)
        s = dfield_ref.sample(dist, shape, origin, step, x)
        keep &= np.all(np.isfinite(s), axis=1)
        loc, x, s = loc[keep], x[keep], s[keep]
        assert loc.shape[0] > 300
        _, t = track_ref.pass_pose(P, dim)
        J = track_ref.jacobian(x, s[:, 1:], t, dim)

        def r_at(xi):
            Q = track_ref.apply(P, list(xi), dim)
            Rq = np.asarray(Q[dim:]).reshape(dim, dim).T
            w = loc.astype(np.float64) @ Rq.T + np.asarray(Q[:dim])
            return dfield_ref.sample(dist, shape, origin, step, w.astype(F32))[:, 0].astype(np.float64)
        h = 1e-4
        for i in range(nj):
            e = np.zeros(nj)
            e[i] = h
            fd = (r_at(e) - r_at(-e)) / (2 * h)
            lever = 1.0 if i < dim else 3.0
            err = np.abs(J[:, i] - fd)
            print("dim %d column %d: |J - fd| median %.2e max %.2e" % (dim, i, float(np.median(err)), float(err.max())))
            assert np.median(err) < 2e-3 * lever and np.quantile(err, 0.99) < 2e-2 * lever, (dim, i)


def test_new_symbols_are_exported():
    import gpismap_amd
    L = gpismap_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    for name in ("gpis3_track_depth_field", "gpis2_track_scan_field"):
        assert hasattr(L, name), name
        assert "int   %s(" % name in hdr, name
    for cls, meth in ((gpismap_amd.DistanceField, "track_depth"), (gpismap_amd.DistanceField, "track_scan"),
                      (gpismap_amd.GPisMap3, "track_depth_field"), (gpismap_amd.GPisMap, "track_scan_field")):
        assert callable(getattr(cls, meth, None)), (cls, meth)
