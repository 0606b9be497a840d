"""The pose-scoring reference (tests/locate_ref.py) on the CPU: the C-ABI's new symbols, the defective variants of the contract
the reference must tell apart on the GPU cases' inputs, the inlier count against the field tracker's on the same points, the
ranking of a pose grid on the analytic 2-D scene with locate-and-refine, and the 3-D cost at and off the true pose."""
import ctypes as C
import math
import os
import re

import numpy as np

import locate_ref
import track_field_ref
import track_ref
from test_gpu_track import _err2, _perturb2, _perturb3
from test_track_field_ref import LAT2, LAT3, field2, field3
from test_track_ref import CAM, OFF2, depth_image, pose6, pose12, rot, scan, scene2, scene3

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_locate_default_opts", "gpis_locate_create", "gpis_locate_destroy", "gpis3_locate_depth_field",
         "gpis2_locate_scan_field", "gpis_locate_get", "gpis_locate_info", "gpis_locate_device"}

# ---- the inputs shared with tests/test_gpu_locate.py ------------------------------------------------------------------------
TH2 = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)
TRUE2 = pose6(0.15, (0.3, -0.2))
TRUE3 = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
MAXR2 = 0.5
_CACHE = {}


def ranges2():
    if "r2" not in _CACHE:
        _CACHE["r2"] = scan(scene2, TH2, TRUE2)
    return _CACHE["r2"]


def depth3():
    if "d3" not in _CACHE:
        _CACHE["d3"] = depth_image(scene3, CAM, TRUE3)
    return _CACHE["d3"]


def grid2():
    """The 2-D pose grid: 13 x 11 positions every 0.25 m, every 10 degrees; it does not hold the true pose."""
    return locate_ref.pose_grid2(np.arange(-1, 2.01, 0.25), np.arange(-1, 1.51, 0.25), np.radians(np.arange(0, 360, 10)))


def grid3():
    """343 x 3 poses around the true one: offsets of +-6 cm in 2 cm steps on each axis, three rotation vectors (zero first)."""
    a = np.arange(-3, 4) * 0.02
    off = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    return locate_ref.pose_grid3(TRUE3, off, [(0.0, 0.0, 0.0), (0.0, 0.02, 0.0), (0.01, -0.01, 0.02)])


def _lat(lat):
    return lat["shape"], lat["origin"], lat["step"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis[0-9]?_locate[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_locate_default_opts.argtypes = [C.c_int, C.POINTER(gpismap_amd.gpis_locate_opts)]
    for dim in (3, 2):
        o = gpismap_amd.gpis_locate_opts()
        assert L.gpis_locate_default_opts(dim, C.byref(o)) == 0
        assert dict(max_residual=o.max_residual, stride=o.stride, top_k=o.top_k) == locate_ref.default_opts(dim)
    assert locate_ref.default_opts(3) == dict(max_residual=0.05, stride=8, top_k=16)
    assert locate_ref.default_opts(2)["max_residual"] == 0.5 and locate_ref.default_opts(2)["top_k"] == 16
    assert L.gpis_locate_default_opts(4, C.byref(o)) == -1 and L.gpis_locate_default_opts(2, None) == -1
    for cls, meths in ((gpismap_amd.DistanceField, ("score_scan", "score_depth", "locate_scan", "locate_depth")),
                       (gpismap_amd.GPisMap, ("score_scan_field", "locate_scan_field")),
                       (gpismap_amd.GPisMap3, ("score_depth_field", "locate_depth_field")),
                       (gpismap_amd.Locator, ("get", "info", "device_ptrs", "close"))):
        for m in meths:
            assert callable(getattr(cls, m, None)), (cls, m)
    for fn in ("locate_opts", "pose_grid2", "pose_grid3"):
        assert callable(getattr(gpismap_amd, fn, None)), fn


def test_pose_grids_match_the_package():
    import gpismap_amd
    xs, ys, th = np.arange(-1, 2.01, 0.25), np.arange(-1, 1.51, 0.25), np.radians(np.arange(0, 360, 10))
    g = gpismap_amd.pose_grid2(xs, ys, th)
    assert g.dtype == F32 and g.shape == (5148, 6) and np.array_equal(g.view(np.uint32), grid2().view(np.uint32))
    # the angle is the slowest axis, then y, then x
    assert tuple(g[1, :2]) == (F32(-0.75), F32(-1.0)) and tuple(g[13, :2]) == (F32(-1.0), F32(-0.75))
    assert g[13 * 11, 2] == F32(math.cos(math.radians(10))) and g[13 * 11, 3] == F32(math.sin(math.radians(10)))
    a = np.arange(-3, 4) * 0.02
    off = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    g3 = gpismap_amd.pose_grid3(TRUE3, off, [(0.0, 0.0, 0.0), (0.0, 0.02, 0.0), (0.01, -0.01, 0.02)])
    assert g3.shape == (1029, 12) and np.array_equal(g3.view(np.uint32), grid3().view(np.uint32))
    assert np.array_equal(g3[171].view(np.uint32), TRUE3.view(np.uint32))          # the zero offset, the zero rotation
    R = g3[343 + 171, 3:].astype(np.float64).reshape(3, 3).T
    assert np.allclose(R, rot([0, 1, 0], 0.02) @ TRUE3[3:].astype(np.float64).reshape(3, 3).T, atol=1e-7)


# ---- the defective variants -------------------------------------------------------------------------------------------------
VARIANTS = ("descending", "np_sum", "tree256", "min_after_square32", "outliers_zero", "pose64")


def test_reference_rejects_the_defective_variants():
    """On the GPU cases' inputs every variant changes the bits of at least one cost (asserted, not assumed)."""
    shape, origin, step = _lat(LAT2)
    loc2, _ = track_ref.points2(TH2, ranges2(), OFF2)
    poses2 = grid2()[:1031]
    good2 = locate_ref.score(field2(), shape, origin, step, loc2, poses2, MAXR2)[0]
    assert np.all(np.isfinite(good2))
    s3, o3, st3 = _lat(LAT3)
    loc3, _ = track_ref.points3(depth3(), CAM, 2)
    poses3 = grid3()[::21]
    good3 = locate_ref.score(field3(), s3, o3, st3, loc3, poses3, 0.05)[0]
    for v in VARIANTS:
        bad2 = locate_ref.score(field2(), shape, origin, step, loc2, poses2, MAXR2, variant=v)[0]
        bad3 = locate_ref.score(field3(), s3, o3, st3, loc3, poses3, 0.05, variant=v)[0]
        n2, n3 = int(np.count_nonzero(_bits(bad2) != _bits(good2))), int(np.count_nonzero(_bits(bad3) != _bits(good3)))
        print("variant %s: %d of %d 2-D costs and %d of %d 3-D costs differ" % (v, n2, good2.size, n3, good3.size))
        assert n2 > 0 and n3 > 0, v


def test_summation_order_by_hand():
    """65 points: slot 0 holds points 0 and 64, every other slot one point; then the tree."""
    T = np.arange(1.0, 66.0)[None, :] * 0.1
    v = list(T[0, :64])
    v[0] = v[0] + T[0, 64]
    h = 32
    while h >= 1:
        for k in range(h):
            v[k] = v[k] + v[k + h]
        h //= 2
    assert _bits(locate_ref.reduce_pose_terms(T))[0] == _bits(np.float64(v[0]))
    assert locate_ref.reduce_pose_terms(np.zeros((3, 0))).tolist() == [0.0, 0.0, 0.0]
    c = np.float64([3.0, 1.0, 2.0, 1.0])
    assert locate_ref.rank(c, 0).tolist() == [1, 3, 2, 0] and locate_ref.rank(c, 1).tolist() == [1]
    assert locate_ref.rank(c, 9).tolist() == [1, 3, 2, 0]


# ---- the tracker's points and test ------------------------------------------------------------------------------------------
def test_inlier_count_is_the_field_trackers():
    shape, origin, step = _lat(LAT2)
    P2 = _perturb2(TRUE2, 0.05, 3.0)
    for off2 in (OFF2, (0.0, 0.05)):
        t = track_field_ref.track_scan(field2(), shape, origin, step, TH2, ranges2(), P2, off2, max_iters=0, max_residual=0.07)
        c, n, _ = locate_ref.score_scan(field2(), shape, origin, step, TH2, ranges2(), P2[None, :], off2, max_residual=0.07)
        assert 0 < n[0] < t["points"] and n[0] == t["inliers"], (off2, n, t["inliers"], t["points"])
    s3, o3, st3 = _lat(LAT3)
    P3 = _perturb3(TRUE3, 0.02, 2.0)
    for stride in (1, 2, 7):
        t = track_field_ref.track_depth(field3(), s3, o3, st3, depth3(), CAM, P3, max_iters=0, max_residual=0.02, stride=stride)
        c, n, _ = locate_ref.score_depth(field3(), s3, o3, st3, depth3(), CAM, P3[None, :], max_residual=0.02, stride=stride)
        assert 0 < n[0] < t["points"] and n[0] == t["inliers"], (stride, n, t["inliers"], t["points"])


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_grid_ranking_and_locate_and_refine_2d():
    shape, origin, step = _lat(LAT2)
    dist = field2()
    poses = grid2()
    assert poses.shape == (5148, 6)
    loc, _ = track_ref.points2(TH2, ranges2(), OFF2)
    cost, inl, order = locate_ref.score(dist, shape, origin, step, loc, poses, MAXR2, top_k=16)
    best, second = poses[order[0]], order[1]
    print("best %s cost %.4f inliers %d; second cost %.4f" % (best, cost[order[0]], inl[order[0]], cost[second]))
    assert order.size == 16 and np.all(np.diff(cost[order]) >= 0)
    assert (best[0], best[1]) == (F32(0.25), F32(-0.25)) and best[2] == F32(math.cos(math.radians(10)))
    assert best[3] == F32(math.sin(math.radians(10)))
    assert inl[order[0]] == loc.shape[0] == 360 and cost[order[0]] < 0.5 * cost[second]

    def track_fn(p0):
        return track_field_ref.track_scan(dist, shape, origin, step, TH2, ranges2(), p0, OFF2)
    pose, info = locate_ref.locate(dist, shape, origin, step, loc, poses, track_fn, refine=8, max_residual=MAXR2, top_k=16)
    k = info["best"]
    near = track_fn(_perturb2(TRUE2, 0.05, 3.0))
    e, en = _err2(pose, TRUE2), _err2(near["pose"], TRUE2)
    print("locate-and-refine: candidate %d (pose index %d), status %d, cost %.4e, error %.2e m %.3f deg; the tracker from 5 cm / "
          "3 deg: status %d, error %.2e m %.3f deg" % (k, info["candidates"][k], info["tracks"][k]["status"],
                                                       info["refined_cost"][k], e[0], e[1], near["status"], en[0], en[1]))
    assert info["tracks"][k]["status"] == 0 and near["status"] == 0
    assert e[0] <= 1.5 * en[0] and e[1] <= 1.5 * en[1]
    # refine = 0: the best-ranked pose itself
    p0, i0 = locate_ref.locate(dist, shape, origin, step, loc, poses, track_fn, refine=0, max_residual=MAXR2, top_k=16)
    assert np.array_equal(p0, poses[order[0]]) and i0["tracks"] == []


def test_true_pose_costs_less_than_a_perturbed_one_3d():
    """No ranking claim in 3-D (DESIGN.md §7f documents the wall's flat valley): the true pose beats 2 cm / 2 degrees off."""
    s3, o3, st3 = _lat(LAT3)
    P = np.stack([TRUE3, _perturb3(TRUE3, 0.02, 2.0)])
    for stride in (1, 8):
        cost, inl, order = locate_ref.score_depth(field3(), s3, o3, st3, depth3(), CAM, P, stride=stride)
        print("3-D stride %d: true %.4e (%d inliers), perturbed %.4e (%d inliers)" % (stride, cost[0], inl[0], cost[1], inl[1]))
        assert cost[0] < cost[1] and order.tolist() == [0, 1]
