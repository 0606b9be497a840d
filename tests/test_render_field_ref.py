"""The field-rendering reference (tests/render_field_ref.py) on the CPU: fields built by dfield_ref from the f of the analytic
scenes of test_track_ref.py, every hit depth against the analytic ray / surface intersection, the properties of the march that
need no tolerance (bracket, record, rays that start inside, a field without sites, the slack and its guarantee), and the C-ABI's
new symbols."""
import math
import os

import numpy as np

import dfield_ref
import mesh_ref
import render_field_ref
import render_ref
from test_track_field_ref import LAT2, LAT3, field2, field3
from test_track_ref import CAM, OFF2, depth_image, pose6, pose12, rot, scan, scene2, scene3

F32 = np.float32
U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T3 = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
T2 = pose6(0.15, (0.3, -0.2))
THETAS = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)

# The reference's own error on these scenes, in lattice steps along the analytic surface normal, over every hit ray (none left
# out: the silhouette of the sphere in front of the wall and the room's corners included), guarded with the usual 1.5x margin
# (DESIGN.md §7g).  Measured: 3-D median 0.00068, p99 0.0310, max 0.0590; 2-D median 0.000023 (the float32
# resolution of a range of a few metres), p99 0.0089, max 0.0136.
REF_ERR3 = {"median": 0.00102, "p99": 0.0465, "max": 0.0885}
REF_ERR2 = {"median": 0.000035, "p99": 0.0133, "max": 0.0203}


def _normal_error(depth, exact, dirs, grad, step):
    """|depth - exact| along the unit normal, in lattice steps (dirs: the world displacement per unit of the parameter)."""
    n = grad / np.linalg.norm(grad, axis=1)[:, None]
    return np.abs((depth.astype(np.float64) - exact) * np.sum(dirs * n, axis=1)) / step


def _errors3(depth, st, pose, scene=scene3):
    exact = depth_image(scene, CAM, pose).astype(np.float64)
    hit = st == 0
    assert np.array_equal(hit, np.isfinite(exact))
    idx = np.nonzero(hit)[0]
    u, v, il, o, d = render_ref.rays3(CAM, pose)
    x = render_ref.points3(u, v, pose, idx, exact[idx].astype(F32))
    dirs = np.stack([d[a][idx] for a in range(3)], axis=1).astype(np.float64)
    return _normal_error(depth[idx], exact[idx], dirs, scene(x)[1], LAT3["step"])


def _errors2(rng, st, pose):
    exact = scan(scene2, THETAS, pose).astype(np.float64)
    hit = st == 0
    assert np.array_equal(hit, np.isfinite(exact))
    idx = np.nonzero(hit)[0]
    c, s, o, d = render_ref.rays2(THETAS, pose, OFF2)
    x = render_ref.points2(c, s, OFF2, pose, idx, exact[idx].astype(F32))
    dirs = np.stack([d[a][idx] for a in range(2)], axis=1).astype(np.float64)
    return _normal_error(rng[idx], exact[idx], dirs, scene2(x)[1], LAT2["step"])


def _render3(dist=None, pose=T3, lat=LAT3, **kw):
    dist = field3() if dist is None else dist
    return render_field_ref.render_depth(dist, lat["shape"], lat["origin"], lat["step"], CAM, pose, **kw)


def _render2(pose=T2, **kw):
    return render_field_ref.render_scan(field2(), LAT2["shape"], LAT2["origin"], LAT2["step"], THETAS, pose, OFF2, **kw)


def test_depth_against_the_analytic_intersection_3d():
    depth, rec, st, stats = _render3()
    e = _errors3(depth, st, T3)
    print("3-D: %d rays, %d hits, %.2f samples per ray (max %d); error along the normal in steps: median %.4f p99 %.4f max %.4f"
          % (st.size, stats["hits"], stats["samples"] / st.size, stats["max_samples"], np.median(e), np.quantile(e, 0.99), e.max()))
    assert stats["hits"] == e.size > 4000
    assert np.median(e) <= REF_ERR3["median"] and np.quantile(e, 0.99) <= REF_ERR3["p99"] and e.max() <= REF_ERR3["max"]
    # the gradient at the reported point is the surface normal the field sees: within a few degrees of the analytic one
    idx = np.nonzero(st == 0)[0]
    u, v, il, o, d = render_ref.rays3(CAM, T3)
    g = scene3(render_ref.points3(u, v, T3, idx, depth[idx]))[1]
    cosang = np.sum(rec[idx, 1:] * g, axis=1) / (np.linalg.norm(rec[idx, 1:], axis=1) * np.linalg.norm(g, axis=1))
    assert np.median(cosang) > 0.999


def test_depth_against_the_analytic_intersection_2d():
    rng, rec, st, stats = _render2()
    e = _errors2(rng, st, T2)
    print("2-D: %d beams, %d hits, %.2f samples per beam (max %d); error along the normal in steps: median %.5f p99 %.4f max %.4f"
          % (st.size, stats["hits"], stats["samples"] / st.size, stats["max_samples"], np.median(e), np.quantile(e, 0.99), e.max()))
    assert stats["hits"] == e.size == 360
    assert np.median(e) <= REF_ERR2["median"] and np.quantile(e, 0.99) <= REF_ERR2["p99"] and e.max() <= REF_ERR2["max"]


def test_bracket_record_and_counters():
    for dim, out, lat, dist in ((3, _render3(refine=3), LAT3, field3()), (2, _render2(refine=0), LAT2, field2()),
                                (3, _render3(max_steps=6), LAT3, field3())):
        depth, rec, st, stats = out
        H, zlo, zhi, dlo, dhi = stats["bracket"]
        assert np.array_equal(H, np.nonzero(st == 0)[0]) and stats["hits"] == H.size
        assert np.all((dlo >= 0) | np.isnan(dlo)) and np.all(dhi < 0) and np.all(zlo < zhi)
        assert np.all((depth[H] >= zlo) & (depth[H] <= zhi))
        if dim == 3:
            u, v, il, o, d = render_ref.rays3(CAM, T3)
            x = render_ref.points3(u, v, T3, H, depth[H])
        else:
            c, s, o, d = render_ref.rays2(THETAS, T2, OFF2)
            x = render_ref.points2(c, s, OFF2, T2, H, depth[H])
        again = dfield_ref.sample(dist, lat["shape"], lat["origin"], lat["step"], x)
        assert np.array_equal(rec[H].view(U32), again.view(U32))
        miss = st != 0
        assert np.all(np.isnan(depth[miss])) and np.all(np.isnan(rec[miss]))
        assert stats["samples"] == stats["per_ray"].sum() and stats["max_samples"] == stats["per_ray"].max()
    assert np.count_nonzero(st == 2) > 1000 and stats["max_samples"] <= 6 + 8 + 1     # the third: a tiny max_steps


def test_a_ray_that_starts_inside_reports_nothing_before_it_has_been_outside():
    """A camera at the centre of the sphere: every ray starts inside (d < 0), leaves the sphere and hits the wall behind it."""
    P = pose12(np.eye(3), np.array([0.1, -0.05, 1.1]))
    first = {}

    def trace(idx, z, x, s, raw):
        for i, d in zip(idx, s[:, 0]):
            first.setdefault(int(i), float(d))
    depth, rec, st, stats = _render3(pose=P, tnear=0.01, trace=trace)
    assert np.all(np.array([first[i] for i in range(st.size)]) < 0)
    hit = st == 0
    assert hit.sum() > 2000
    u, v, il, o, d = render_ref.rays3(CAM, P)
    x = render_ref.points3(u, v, P, np.nonzero(hit)[0], depth[hit])
    r = np.linalg.norm(x.astype(np.float64) - np.array([0.1, -0.05, 1.1]), axis=1)
    assert r.min() > 0.25                      # nothing is reported on the sphere (radius 0.2) the rays leave from inside
    assert np.abs(x[:, 2] - 1.5).max() < 0.06  # the wall (z = 1.5 +- 0.05)


def test_a_field_without_sites_misses_everywhere():
    """Its lattice is all +inf or all -inf; the interpolant of equal infinities is NaN (inf - inf in the lerp), so every sample
    counts as unknown, the ray creeps by min_step and leaves its interval: status 1 (2 only where max_steps samples do not
    reach the end of the interval)."""
    shape, origin, step = (8, 8, 8), (-0.35, -0.35, 0.8), 0.1
    for sign in (1.0, -1.0):
        dist, site = dfield_ref.distance_field(np.full(512, sign, F32), shape, origin, step, 0.0)
        assert np.all(np.isinf(dist)) and np.all(site == -1)
        depth, rec, st, stats = render_field_ref.render_depth(dist, shape, origin, step, CAM, pose12(np.eye(3), np.zeros(3)))
        assert np.all(st == 1) and stats["hits"] == 0 and np.all(np.isnan(depth))
        assert stats["samples"] >= np.count_nonzero(stats["per_ray"]) > 0 and stats["max_samples"] < 512


# ---- the slack ------------------------------------------------------------------------------------------------------------
SPH = dict(shape=(61, 61, 51), origin=(-0.5, -0.65, 0.6), step=0.02)        # 189 771 points around the sphere of scene3
CENTRE, RADIUS = np.array([0.1, -0.05, 1.1]), 0.2


def sphere3(p):
    d = np.asarray(p, np.float64) - CENTRE
    n = np.linalg.norm(d, axis=1)
    return n - RADIUS, d / n[:, None]


_SPH = {}


def _sphere_field():
    if not _SPH:
        x = mesh_ref.lattice(SPH["shape"], SPH["origin"], [SPH["step"]] * 3)
        f = sphere3(x)[0].astype(F32)
        _SPH["f"] = f
        _SPH["dist"] = dfield_ref.distance_field(f, SPH["shape"], SPH["origin"], SPH["step"], 0.0)[0]
    return _SPH["f"], _SPH["dist"]


def test_slack_hits_the_same_surface_with_more_samples():
    f, dist = _sphere_field()
    out = {s: _render3(dist, lat=SPH, slack=s) for s in (0.0, 3.0)}
    for s, (depth, rec, st, stats) in out.items():
        e = _errors3(depth, st, T3, scene=sphere3)
        print("sphere, slack %.0f: %d hits, %d samples, error along the normal max %.4f steps" % (s, stats["hits"], stats["samples"], e.max()))
        assert stats["hits"] > 200 and e.max() <= REF_ERR3["max"]
    a, b = out[0.0], out[3.0]
    assert np.array_equal(a[2], b[2])
    hit = a[2] == 0
    u, v, il, o, d = render_ref.rays3(CAM, T3)
    dn = np.abs(a[0][hit].astype(np.float64) - b[0][hit]) / il[hit] / SPH["step"]      # arc length, in steps: >= along the normal
    assert np.quantile(dn, 0.98) <= 2 * REF_ERR3["max"]
    assert b[3]["samples"] > a[3]["samples"]


def test_an_unclamped_step_never_exceeds_the_distance_to_the_nearest_anchor():
    """The guarantee the default slack is derived from: |d| - 3 step <= the distance from the sample to the
    nearest anchor -- a statement about the anchors (the mesh vertices of this lattice), not about the continuous surface."""
    f, dist = _sphere_field()
    verts = mesh_ref.extract(f, SPH["shape"], SPH["origin"], [SPH["step"]] * 3, 0.0)[0].astype(np.float64)
    assert verts.shape[0] > 1000
    pts, raws = [], []

    def trace(idx, z, x, s, raw):
        keep = raw > 0
        pts.append(x[keep])
        raws.append(raw[keep])
    _render3(dist, lat=SPH, trace=trace)
    x, raw = np.concatenate(pts).astype(np.float64), np.concatenate(raws).astype(np.float64)
    assert raw.size > 5000
    near = np.full(raw.size, np.inf)
    for lo in range(0, raw.size, 2048):
        d2 = ((x[lo:lo + 2048, None, :] - verts[None, :, :]) ** 2).sum(axis=2)
        near[lo:lo + 2048] = np.sqrt(d2.min(axis=1))
    margin = (near - raw) / SPH["step"]
    print("%d unclamped steps against %d anchors: smallest margin %.3f steps" % (raw.size, verts.shape[0], margin.min()))
    assert margin.min() >= 0.0


def test_new_symbols_are_exported():
    import gpismap_amd
    L = gpismap_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    for name in ("gpis3_render_depth_field", "gpis2_render_scan_field", "gpis_render_field_default_opts", "gpis_render_set_field_tiles"):
        assert hasattr(L, name), name
        assert "int   %s(" % name in hdr, name
    assert "} gpis_render_field_opts;" in hdr
    for cls, meth in ((gpismap_amd.DistanceField, "render_depth"), (gpismap_amd.DistanceField, "render_scan"),
                      (gpismap_amd.GPisMap3, "render_depth_field"), (gpismap_amd.GPisMap, "render_scan_field")):
        assert callable(getattr(cls, meth, None)), (cls, meth)
    assert callable(gpismap_amd.render_field_opts)
