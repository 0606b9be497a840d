"""The coverage reference (tests/cover_ref.py) on the CPU: the C-ABI's new symbols, the 2-D scene's two frontier clusters at the
edges of the pillar's shadow and their disappearance after a second scan, exploration composed from the references, the 3-D rule
on the sphere-and-wall scene, and the corner cases the device tests rely on, asserted rather than assumed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cover_ref
import plan_ref
from test_locate_ref import TH2, TRUE2, TRUE3, depth3, ranges2
from test_track_field_ref import LAT2, LAT3, field2, field3
from test_track_ref import CAM, OFF2, pose6, pose12, scan, scene2

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_cover_default_opts", "gpis_cover_create", "gpis_cover_destroy", "gpis_cover_reset", "gpis_cover_set",
         "gpis_cover_get", "gpis_cover_device", "gpis3_cover_depth", "gpis2_cover_scan", "gpis_cover_frontiers",
         "gpis_cover_counts", "gpis_cover_get_frontiers", "gpis_cover_restrict", "gpis_cover_info"}
GAP = math.radians(2.0)
POSE2B = pose6(2.0, (3.6, 1.6))
_CACHE = {}


def _lat(lat):
    return lat["shape"], lat["origin"], lat["step"]


def seen2_first():
    if "a" not in _CACHE:
        shape, origin, step = _lat(LAT2)
        _CACHE["a"] = cover_ref.integrate_scan(np.zeros(int(np.prod(shape)), bool), shape, origin, step, TH2, ranges2(), TRUE2, OFF2,
                                               step, GAP)
    return _CACHE["a"]


def ranges2b():
    if "rb" not in _CACHE:
        _CACHE["rb"] = scan(scene2, TH2, POSE2B)
    return _CACHE["rb"]


def seen3_first():
    if "3" not in _CACHE:
        shape, origin, step = _lat(LAT3)
        _CACHE["3"] = cover_ref.integrate_depth(np.zeros(int(np.prod(shape)), bool), shape, origin, step, depth3(), CAM, TRUE3, step)
    return _CACHE["3"]


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis[23]?_cover[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_cover_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_cover_opts)]
    for dim, step in ((2, 0.02), (3, 0.05)):
        o = gpismap_amd.gpis_cover_opts()
        assert L.gpis_cover_default_opts(dim, step, C.byref(o)) == 0
        assert dict(back_off=o.back_off, max_gap=o.max_gap, clearance=o.clearance, min_size=o.min_size,
                    max_rounds=o.max_rounds) == cover_ref.default_opts(dim, float(F32(step)))
    d = cover_ref.default_opts(2, 0.5)
    assert d == dict(back_off=0.5, max_gap=float(F32(math.radians(2.0))), clearance=1.5, min_size=8, max_rounds=0)
    assert L.gpis_cover_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_cover_default_opts(2, 0.1, None) == -1
    assert L.gpis_cover_default_opts(2, 0.0, C.byref(o)) == -1
    for cls, meths in ((gpismap_amd.Coverage, ("reset", "integrate_depth", "integrate_scan", "set", "get", "device_ptr", "frontiers",
                                               "restrict", "info", "close")),
                       (gpismap_amd.GPisMap3, ("cover_depth",)), (gpismap_amd.GPisMap, ("cover_scan",)),
                       (gpismap_amd.DistanceField, ("explore",))):
        for m in meths:
            assert callable(getattr(cls, m, None)), (cls, m)
    assert callable(gpismap_amd.cover_opts)


# ---- the 2-D scene ----------------------------------------------------------------------------------------------------------
def test_pillar_shadow_raises_two_clusters_and_a_second_scan_closes_them():
    shape, origin, step = _lat(LAT2)
    dist, seen = field2(), seen2_first()
    fr = cover_ref.frontiers(seen, dist, shape, origin, step, 0.1, 8)
    print("first scan: %d seen, %d frontier points, %d components, clusters %s at %s" %
          (seen.sum(), fr["points"].size, fr["clusters"], fr["count"].tolist(), fr["rep_point"].tolist()))
    assert fr["label"].size == 2 and fr["clusters"] == 2 and np.all(fr["count"] >= 50)
    assert np.all(np.diff(fr["label"]) > 0) and fr["count"].sum() == fr["points"].size
    # the two edges of the pillar's shadow: both representatives lie beyond the pillar (centre (2.0, 0.6), radius 0.4) as seen
    # from the sensor, one on each side of the line through sensor and pillar
    s = np.asarray(TRUE2[:2], np.float64)
    axis = np.array([2.0, 0.6]) - s
    side = []
    for r in fr["rep_point"].astype(np.float64):
        v = r - s
        assert np.linalg.norm(v) > np.linalg.norm(axis)
        side.append(np.sign(axis[0] * v[1] - axis[1] * v[0]))
    assert sorted(side) == [-1.0, 1.0]
    # every member is seen and traversable, every representative is a member of its cluster, inside its box
    assert np.all(seen[fr["points"]]) and np.all(dist[fr["points"]] >= F32(0.1))
    for c in range(2):
        mem = fr["points"][fr["point_label"] == fr["label"][c]]
        assert fr["rep"][c] in mem and fr["label"][c] == mem.min() and mem.size == fr["count"][c]
        i, j = fr["rep"][c] % shape[0], fr["rep"][c] // shape[0]
        assert fr["box"][c, 0] <= i <= fr["box"][c, 3] and fr["box"][c, 1] <= j <= fr["box"][c, 4]
    # a lower clearance lets the scan's ragged rim through: small clusters, dropped by min_size
    lo = cover_ref.frontiers(seen, dist, shape, origin, step, 0.06, 1)
    print("clearance 0.06: clusters", lo["count"].tolist())
    assert lo["label"].size > 2 and cover_ref.frontiers(seen, dist, shape, origin, step, 0.06, 8)["label"].size == 2
    # the second scan looks behind the pillar
    both = cover_ref.integrate_scan(seen, shape, origin, step, TH2, ranges2b(), POSE2B, OFF2, step, GAP)
    fr2 = cover_ref.frontiers(both, dist, shape, origin, step, 0.1, 8)
    print("second scan: %d seen, %d frontier points" % (both.sum(), fr2["points"].size))
    assert np.all(both[seen]) and both.sum() > seen.sum() and fr2["label"].size == 0 and fr2["points"].size == 0


def test_explore_is_composed_from_the_references():
    shape, origin, step = _lat(LAT2)
    dist, seen = field2(), seen2_first()
    path, status, fr = cover_ref.explore(seen, dist, shape, origin, step, TRUE2[:2], 0.1)
    assert status == 0 and path.shape[0] > 10
    assert any(np.array_equal(path[-1].view(np.uint32), r.view(np.uint32)) for r in fr["rep_point"])
    ok, ijk = plan_ref.snap(path, shape, origin, step)
    assert ok.all() and np.all(seen[ijk[:, 1] * shape[0] + ijk[:, 0]])
    # without the restriction the planner also accepts unseen space: the restricted field blocks all of it
    rd = cover_ref.restrict(seen, dist, -step)
    assert np.all(rd[~seen] == F32(-step)) and np.array_equal(rd[seen].view(np.uint32), dist[seen].view(np.uint32))
    # nothing left to explore: status 4
    both = cover_ref.integrate_scan(seen, shape, origin, step, TH2, ranges2b(), POSE2B, OFF2, step, GAP)
    p2, st2, _ = cover_ref.explore(both, dist, shape, origin, step, TRUE2[:2], 0.1)
    assert st2 == 4 and p2.shape == (0, 2)


# ---- the 3-D scene ----------------------------------------------------------------------------------------------------------
def test_depth_rule_on_the_sphere_and_wall():
    """The nearest pixel's ray passes a seen point within half a pixel diagonal h = z sqrt(2) / (2 f), and that ray is free up to
    its depth, so a seen point lies at most h inside a surface; the field itself is exact to within a lattice step.  Bound:
    dist >= -(h(z_max) + step).  Measured here: min dist of a seen point -0.0105 (h + step = 0.0446), 204 857 points seen,
    clusters of 9978 and 917 points at clearance 3 steps."""
    shape, origin, step = _lat(LAT3)
    dist, seen = field3(), seen3_first()
    zmax = origin[2] + (shape[2] - 1) * step
    h = zmax * math.sqrt(2.0) / (2.0 * CAM[0])
    print("3-D: %d seen, min dist of a seen point %.4f, bound %.4f" % (seen.sum(), dist[seen].min(), -(h + step)))
    assert seen.sum() > 100000 and dist[seen].min() >= -(h + step)
    # almost all of what is seen is free space proper
    assert np.count_nonzero(dist[seen] < 0) < 0.001 * seen.sum()
    fr = cover_ref.frontiers(seen, dist, shape, origin, step, 3 * step, 8)
    print("3-D clusters:", fr["count"].tolist(), fr["box"].tolist())
    assert fr["label"].size >= 1
    # the sphere (centre (0.1, -0.05, 1.1), radius 0.2) casts a shadow: some cluster has a member behind it, inside its silhouette
    x = cover_ref.lattice_points(fr["points"], shape, origin, step).astype(np.float64)
    behind = (x[:, 2] > 1.3) & (np.hypot(x[:, 0] - 0.1, x[:, 1] + 0.05) < 0.3)
    assert behind.any() and np.isin(fr["point_label"][behind], fr["label"]).any()


# ---- corner cases -----------------------------------------------------------------------------------------------------------
def _tiny2():
    return (9, 7), (-0.4, -0.3), 0.1


def test_fewer_than_two_valid_beams_see_nothing():
    shape, origin, step = _tiny2()
    P = pose6(0.0, (0.0, 0.0))
    th = np.array([0.0, 0.01, 0.02], F32)
    for r in ([0.0, 0.0, 0.0], [1.0, 0.0, 40.0], [np.nan, 1.0, 0.1]):
        assert not cover_ref.scan_mask(shape, origin, step, th, np.array(r, F32), P, (0.0, 0.0), 0.01, GAP).any()
    two = cover_ref.scan_mask(shape, origin, step, th, np.array([1.0, 0.0, 1.0], F32), P, (0.0, 0.0), 0.01, GAP)
    assert two.any()


def test_duplicate_beams_change_nothing():
    shape, origin, step = _lat(LAT2)
    r = ranges2()
    idx = np.concatenate([np.arange(360), [17, 17, 200, 359, 0]])
    a = seen2_first()
    b = cover_ref.scan_mask(shape, origin, step, TH2[idx], r[idx], TRUE2, OFF2, step, GAP)
    assert np.array_equal(a, b)
    q, lim, narrow = cover_ref.sector_table(TH2[idx], r[idx], step, GAP)
    assert q.size == 365 and np.all(np.diff(q) >= 0) and np.count_nonzero(np.diff(q) == 0) == 5


def test_a_lattice_point_exactly_on_the_sensor_is_seen():
    shape, origin, step = _tiny2()
    on = cover_ref.lattice_points([3 * 9 + 4], shape, origin, step)[0]          # lattice point (4, 3)
    P = pose6(0.3, (float(on[0]), float(on[1])))
    th = np.array([0.0, 0.02], F32)
    m = cover_ref.scan_mask(shape, origin, step, th, np.array([0.5, 0.5], F32), P, (0.0, 0.0), 0.01, GAP)
    assert m[3 * 9 + 4]
    m1 = cover_ref.scan_mask(shape, origin, step, th, np.array([0.5, 0.0], F32), P, (0.0, 0.0), 0.01, GAP)
    assert not m1.any()


def test_wide_sectors_and_missing_returns_stay_unseen():
    shape, origin, step = _tiny2()
    P = pose6(0.0, (0.0, 0.0))
    th = np.radians(np.arange(0, 360, 1.0)).astype(F32)
    r = np.full(360, 2.0, F32)
    assert cover_ref.scan_mask(shape, origin, step, th, r, P, (0.0, 0.0), 0.01, GAP).all()
    r[90:181] = 0.0                                      # no return between 90 and 180 degrees: that quadrant stays unseen
    m = cover_ref.scan_mask(shape, origin, step, th, r, P, (0.0, 0.0), 0.01, GAP).reshape(7, 9)
    assert not m[4:, :4].any() and m[:3, :].all() and m[:, 5:].all()
    # two beams 359 degrees apart the long way round: the dot product alone would call the wide sector narrow
    th2 = np.radians([0.5, 359.5]).astype(F32)
    q, lim, narrow = cover_ref.sector_table(th2, np.array([2.0, 2.0], F32), 0.01, GAP)
    assert narrow.tolist() == [False, True]


def test_pixels_one_off_the_image_on_each_side():
    """An unrotated camera at the origin looking along z with fx = fy = 1, cx = cy = 0 and a 3 x 2 image: the lattice plane z = 1
    holds one point per integer pixel coordinate from -1 to 3 (x) and -1 to 2 (y)."""
    shape, origin, step = (5, 4, 1), (-1.0, -1.0, 1.0), 1.0
    cam = (1.0, 1.0, 0.0, 0.0, 3, 2)
    P = pose12(np.eye(3), np.zeros(3))
    m = cover_ref.depth_mask(shape, origin, step, np.full(6, 2.0, F32), cam, P, 0.5).reshape(4, 5)
    want = np.zeros((4, 5), bool)
    want[1:3, 1:4] = True
    assert np.array_equal(m, want)
    # column-major pixels: only pixel (2, 1) valid; a point at the depth less back_off exactly is not seen
    d = np.zeros(6, F32)
    d[2 * 2 + 1] = 2.0
    m = cover_ref.depth_mask(shape, origin, step, d, cam, P, 0.5).reshape(4, 5)
    assert m.sum() == 1 and m[2, 3]
    assert not cover_ref.depth_mask(shape, origin, step, d, cam, P, 1.0).any()
    # behind the camera
    assert not cover_ref.depth_mask(shape, (-1.0, -1.0, -1.0), step, np.full(6, 2.0, F32), cam, P, 0.5).any()


def test_option_checks():
    o = cover_ref.default_opts(2, 0.02)
    cover_ref.check_opts(o)
    for bad in (dict(clearance=o["back_off"]), dict(clearance=0.0), dict(back_off=-0.01), dict(max_gap=0.0),
                dict(max_gap=math.pi / 2), dict(min_size=0), dict(max_rounds=-1), dict(clearance=float("nan"))):
        with pytest.raises(ValueError):
            cover_ref.check_opts(dict(o, **bad))


def test_full_connectivity_joins_diagonal_touches_and_the_border_raises_nothing():
    shape = (6, 5)
    dist = np.ones(30, F32)
    # the lattice border alone raises nothing
    assert not cover_ref.frontier_flags(np.ones(30, bool), dist, shape, 0.5).any()
    # two unseen points that touch at a corner: their rims join into one component
    seen = np.ones((5, 6), bool)
    seen[1, 1] = seen[2, 2] = False
    fr = cover_ref.frontiers(seen.ravel(), dist, shape, (0.0, 0.0), 1.0, 0.5, 1)
    assert fr["clusters"] == 1 and fr["count"].tolist() == [6]
    # two frontier points that touch only diagonally are one component; two apart are two
    pts = np.array([0 * 6 + 0, 1 * 6 + 1, 3 * 6 + 3, 3 * 6 + 5])
    assert cover_ref.components(pts, shape).tolist() == [0, 0, 21, 23]
    # NaN and low distances are neither frontier nor neighbour
    d2 = dist.copy()
    d2[1 * 6 + 1] = np.nan
    d2[2 * 6 + 2] = 0.4
    assert not cover_ref.frontier_flags(seen.ravel(), d2, shape, 0.5).any()
    # the representative: ties go to the smallest index (a 2 x 2 block: all four are equally far from the centroid)
    s2 = np.zeros((5, 6), bool)
    s2[1:3, 1:3] = True
    fr = cover_ref.frontiers(s2.ravel(), dist, shape, (0.0, 0.0), 1.0, 0.5, 1)
    assert fr["count"].tolist() == [4] and fr["rep"].tolist() == [7] and fr["sums"].tolist() == [[6, 6, 0]]
    assert fr["box"].tolist() == [[1, 1, 0, 2, 2, 0]] and fr["centroid"].tolist() == [[1.5, 1.5]]


# ---- the host code on its own -----------------------------------------------------------------------------------------------
def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/cover_host_check.cpp: the pseudo-angle, the sector table and the option checks of csrc/cover_host.h, compiled
    with the sanitizers and run directly; its table is compared with the reference's, bit for bit."""
    exe = tmp_path / "cover_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpismap_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "cover_host_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "0", lines[-5:]
    # the program's table of its own 365-beam scan (angles and ranges as below): q, lim, narrow per line
    k = np.arange(365)
    th = (-3.1 + 6.2 * (k * 37 % 365) / 364.0).astype(F32)
    rg = (1.0 + 0.5 * (k * 53 % 101) / 100.0).astype(F32)
    rg[k % 11 == 3] = 0.0
    rg[100] = 40.0
    th[200] = th[17]
    q, lim, narrow = cover_ref.sector_table(th, rg, 0.02, F32(GAP))
    rows = [l.split() for l in lines if l.startswith("T ")]
    assert len(rows) == q.size > 300
    got_q = np.array([int(r[1], 16) for r in rows], np.uint64)
    got_lim = np.array([int(r[2], 16) for r in rows], np.uint64)
    got_n = np.array([int(r[3]) for r in rows])
    assert np.array_equal(got_q, q.view(np.uint64)) and np.array_equal(got_lim, lim.view(np.uint64))
    assert np.array_equal(got_n, narrow.astype(int))
