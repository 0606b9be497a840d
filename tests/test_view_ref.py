"""The view-scoring reference (tests/view_ref.py) on the CPU: the C-ABI's new symbols and defaults, the recorded gains of the 2-D
pillar scene's frontier representatives and of the 3-D scene's own view, the identity with integration that defines the gain, and
the corner cases the device tests rely on, asserted rather than assumed."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cover_ref
import view_ref
from test_cover_ref import seen2_first, seen3_first
from test_locate_ref import TH2, TRUE2, TRUE3
from test_track_field_ref import LAT2, LAT3, field2, field3
from test_track_ref import CAM, OFF2, pose6, pose12, rot

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_view_default_opts", "gpis_view_create", "gpis_view_destroy", "gpis3_view_gain_depth", "gpis2_view_gain_scan",
         "gpis_view_get", "gpis_view_get_predicted", "gpis_view_info"}
YAWS8 = np.arange(8) * (2.0 * math.pi / 8.0)
WALL2 = pose6(0.0, (4.32, 1.0))            # the sensor (offset 0.08 along x) stands 0.1 m in front of the wall x = 4.5
OUTSIDE2 = pose6(1.0, (9.0, 9.0))
OUTSIDE3 = pose12(np.eye(3), np.array([0.0, 0.0, 9.0]))
_CACHE = {}


def _lat(lat):
    return lat["shape"], lat["origin"], lat["step"]


def pose_grid2(xs, ys, thetas):
    """gpismap_amd.pose_grid2 (its agreement with the package is tests/test_locate_ref.py's)."""
    xs, ys, th = (np.asarray(v, np.float64).ravel() for v in (xs, ys, thetas))
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    c, s = np.cos(T), np.sin(T)
    return np.stack([X, Y, c, s, -s, c], axis=-1).reshape(-1, 6).astype(F32)


def candidates2():
    """The 16 poses of the 2-D scene: the two frontier cluster representatives after the first scan x 8 yaws."""
    if "c2" not in _CACHE:
        shape, origin, step = _lat(LAT2)
        fr = cover_ref.frontiers(seen2_first(), field2(), shape, origin, step, 0.1, 8)
        _CACHE["c2"] = np.concatenate([pose_grid2([r[0]], [r[1]], YAWS8) for r in fr["rep_point"]])
    return _CACHE["c2"]


def free_field(shape):
    return np.ones(int(np.prod(shape)), F32)


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis[23]?_view[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_view_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_view_opts)]
    for dim, step in ((2, 0.02), (3, 0.05)):
        o = gpismap_amd.gpis_view_opts()
        assert L.gpis_view_default_opts(dim, step, C.byref(o)) == 0
        d = view_ref.default_opts(dim, float(F32(step)))
        assert dict(back_off=o.back_off, max_gap=o.max_gap, miss=o.miss, min_dist=o.min_dist) == {k: d[k] for k in ("back_off", "max_gap", "miss", "min_dist")}
        for k in ("tnear", "tfar", "min_step", "max_step", "slack", "refine", "max_steps"):
            assert getattr(o.march, k) == F32(getattr(d["march"], k)), k
    d = view_ref.default_opts(3, 0.5)
    assert (d["back_off"], d["miss"], d["min_dist"], d["max_gap"]) == (0.5, 3.5, -math.inf, float(F32(math.radians(2.0))))
    assert view_ref.default_opts(2, 0.5)["miss"] == 29.5
    assert L.gpis_view_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_view_default_opts(2, 0.1, None) == -1
    assert L.gpis_view_default_opts(2, 0.0, C.byref(o)) == -1
    for cls, meths in ((gpismap_amd.ViewScorer, ("gain", "hits", "predicted", "info", "close")),
                       (gpismap_amd.GPisMap3, ("view_gain_depth_field",)), (gpismap_amd.GPisMap, ("view_gain_scan_field",)),
                       (gpismap_amd.DistanceField, ("view_gain_depth", "view_gain_scan", "next_view", "explore"))):
        for m in meths:
            assert callable(getattr(cls, m, None)), (cls, m)
    assert callable(gpismap_amd.view_opts)


# ---- the recorded scenes ------------------------------------------------------------------------------------------------------
def test_gains_at_the_pillar_scenes_frontier_representatives():
    shape, origin, step = _lat(LAT2)
    dist, seen = field2(), seen2_first()
    assert seen.sum() == 62434
    P = candidates2()
    gain, hits, pred = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, P)
    print("2-D gains", gain.tolist(), "hits", hits.tolist())
    assert gain.dtype == np.int64 and hits.dtype == np.int32 and pred.shape == (16, 360) and pred.dtype == F32
    assert np.all(hits == 360)
    assert gain[:8].min() == 9373 and gain[:8].max() == 9416 and gain[8:].min() == 9461 and gain[8:].max() == 9505
    # the identity that defines the gain: the bytes integrating the predicted scan would turn from 0 to 1
    for k in (0, 5, 11):
        after = cover_ref.integrate_scan(seen, shape, origin, step, TH2, pred[k], P[k], OFF2, step, math.radians(2.0))
        assert int(after.sum()) - int(seen.sum()) == gain[k]
    # a pose alone and in the batch
    g1, h1, p1 = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, P[11])
    assert g1[0] == gain[11] and h1[0] == hits[11] and np.array_equal(p1[0].view(np.uint32), pred[11].view(np.uint32))
    # the view that was integrated gains next to nothing of its own mask
    g0, _, p0 = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, TRUE2)
    mask = cover_ref.scan_mask(shape, origin, step, TH2, p0[0], TRUE2, OFF2, step, math.radians(2.0))
    print("2-D own view: gain %d of a mask of %d" % (g0[0], mask.sum()))
    assert mask.sum() > 50000 and g0[0] < 0.001 * mask.sum()


def test_gain_of_the_3d_scenes_own_view():
    shape, origin, step = _lat(LAT3)
    dist, seen = field3(), seen3_first()
    gain, hits, pred = view_ref.gain_depth(dist, seen, shape, origin, step, CAM, TRUE3)
    mask = cover_ref.depth_mask(shape, origin, step, pred[0], CAM, TRUE3, step)
    print("3-D own view: %d hits, gain %d of a mask of %d" % (hits[0], gain[0], mask.sum()))
    assert hits[0] == 4800 and gain[0] == 14
    assert mask.sum() > 100000 and gain[0] < 0.001 * mask.sum()
    after = cover_ref.integrate_depth(seen, shape, origin, step, pred[0], CAM, TRUE3, step)
    assert int(after.sum()) - int(seen.sum()) == gain[0]
    # turned away from what was seen, the same camera reveals more; min_dist only ever removes targets
    P2 = pose12(rot([0.2, 1.0, 0.1], math.radians(25.0)), np.array([-0.3, 0.1, 0.05]))
    g2, h2, p2 = view_ref.gain_depth(dist, seen, shape, origin, step, CAM, P2)
    g3, _, _ = view_ref.gain_depth(dist, seen, shape, origin, step, CAM, P2, min_dist=0.1)
    print("3-D turned view: gain %d (%d with min_dist 0.1), %d hits" % (g2[0], g3[0], h2[0]))
    assert g2[0] > 1000 and 0 < g3[0] < g2[0]
    after = cover_ref.integrate_depth(seen, shape, origin, step, p2[0], CAM, P2, step)
    assert int(after.sum()) - int(seen.sum()) == g2[0]


# ---- corner cases -----------------------------------------------------------------------------------------------------------
def test_a_nan_miss_reveals_nothing_and_the_default_miss_reveals_the_range():
    shape, origin, step = (60, 40), (-0.6, -0.4), 0.02
    dist, seen = free_field(shape), np.zeros(2400, bool)
    P = np.stack([pose6(0.3, (0.0, 0.0)), pose6(2.0, (0.2, -0.1))])
    th = TH2[::4]
    gain, hits, pred = view_ref.gain_scan(dist, seen, shape, origin, step, th, (0.0, 0.0), P, miss=float("nan"), max_gap=math.radians(5.0))
    assert np.all(hits == 0) and np.all(gain == 0) and np.isnan(pred).all()
    for miss in (0.0, 0.1, 30.0, -1.0, float("inf")):
        g, _, _ = view_ref.gain_scan(dist, seen, shape, origin, step, th, (0.0, 0.0), P, miss=miss, max_gap=math.radians(5.0))
        assert np.all(g == 0), miss
    g, h, _ = view_ref.gain_scan(dist, seen, shape, origin, step, th, (0.0, 0.0), P, max_gap=math.radians(5.0))
    assert np.all(h == 0) and np.all(g == 2400)                    # every ray misses and is given the range: all is revealed
    cam = (20.0, 20.0, 6.0, 3.0, 13, 7)
    shape3, origin3 = (20, 12, 10), (-0.2, -0.12, 0.5)
    P3 = pose12(np.eye(3), np.zeros(3))[None]
    g, h, _ = view_ref.gain_depth(free_field(shape3), np.zeros(2400, bool), shape3, origin3, step, cam, P3, miss=float("nan"))
    assert h[0] == 0 and g[0] == 0
    g, h, _ = view_ref.gain_depth(free_field(shape3), np.zeros(2400, bool), shape3, origin3, step, cam, P3)
    assert h[0] == 0 and 0 < g[0] < 2400


def test_ranges_below_the_window_change_a_poses_sector_table():
    """From 0.1 m in front of the wall the march (tnear 0.05) predicts ranges below 0.2: those beams are not valid, the pose's
    table is shorter than the other pose's, and the gain is still the integration identity's."""
    shape, origin, step = _lat(LAT2)
    dist, seen = field2(), seen2_first()
    P = np.stack([WALL2, candidates2()[3]])
    gain, hits, pred = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, P, tnear=0.05)
    valid = ((pred.astype(np.float64) > 0.2) & (pred.astype(np.float64) < 30.0)).sum(axis=1)
    print("near the wall: %d of 360 beams valid, %d below 0.2; gains %s" % (valid[0], (pred[0] < 0.2).sum(), gain.tolist()))
    assert hits[0] == 360 and 0 < (pred[0] < F32(0.2)).sum() < 360 and valid[0] < valid[1] == 360
    for k in range(2):
        after = cover_ref.integrate_scan(seen, shape, origin, step, TH2, pred[k], P[k], OFF2, step, math.radians(2.0))
        assert int(after.sum()) - int(seen.sum()) == gain[k]
    assert gain[0] > 0


def test_a_pose_outside_the_lattice():
    """The 2-D laser looks all round: from outside, the beams that cross the lattice box are marched through it (they start inside
    a wall, so only a later free-to-wall crossing is a hit), the others miss without a sample.  The 3-D camera looks away."""
    shape, origin, step = _lat(LAT2)
    dist, seen = field2(), seen2_first()
    gain, hits, pred = view_ref.gain_scan(dist, seen, shape, origin, step, TH2, OFF2, OUTSIDE2)
    miss = F32(30.0) - F32(step)
    print("outside: %d hits, gain %d" % (hits[0], gain[0]))
    assert 0 < hits[0] < 90 and np.count_nonzero(pred[0] == miss) == 360 - hits[0]
    after = cover_ref.integrate_scan(seen, shape, origin, step, TH2, pred[0], OUTSIDE2, OFF2, step, math.radians(2.0))
    assert int(after.sum()) - int(seen.sum()) == gain[0]
    shape, origin, step = _lat(LAT3)
    gain, hits, _ = view_ref.gain_depth(field3(), seen3_first(), shape, origin, step, CAM, OUTSIDE3)
    assert hits[0] == 0 and gain[0] == 0


def test_targets_and_option_checks():
    dist = np.array([1.0, np.nan, -np.inf, 0.05, 0.2, 1.0], F32)
    seen = np.array([0, 0, 0, 0, 0, 1], np.uint8)
    assert view_ref.targets(seen, dist, -math.inf).tolist() == [True, True, True, True, True, False]
    assert view_ref.targets(seen, dist, 0.1).tolist() == [True, True, False, False, True, False]
    assert view_ref.targets(seen, dist, math.inf).tolist() == [False, True, False, False, False, False]
    o = view_ref.default_opts(2, 0.02)
    view_ref.check_opts(o)
    for bad in (dict(min_dist=float("nan")), dict(back_off=-0.01), dict(back_off=float("inf")), dict(max_gap=0.0),
                dict(max_gap=math.pi / 2)):
        with pytest.raises(ValueError):
            view_ref.check_opts(dict(o, **bad))
    with pytest.raises(TypeError):
        view_ref.gain_scan(free_field((4, 4)), np.zeros(16), (4, 4), (0.0, 0.0), 0.1, TH2, OFF2, TRUE2, nonsense=1)


# ---- the host code on its own -----------------------------------------------------------------------------------------------
def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/view_host_check.cpp: the option tail, the batch limits and the order table of csrc/view_host.h, compiled with the
    sanitizers and run directly; the tables built from the order table are compared with cover_host.h's inside the program."""
    exe = tmp_path / "view_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpismap_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "view_host_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().splitlines()[-1] == "0", r.stdout[-2000:]
