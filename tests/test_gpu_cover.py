"""Coverage of the sensor's view, its frontiers and the field restricted to seen space on the GPU (csrc/cover.hip, gpis_cover_*)
against the numpy reference (tests/cover_ref.py): every result is an integer or a double computed in one fixed order, so every
comparison is for equal bytes.  Fields come from from_grid on analytic grids; the frontier cases upload their masks."""
import ctypes as C
import math

import numpy as np
import pytest

import cover_ref
import plan_ref
import replay
from test_cover_ref import GAP, POSE2B, ranges2b
from test_gpu_dfield import SYN
from test_gpu_locate import _masked
from test_gpu_plan import _balls, _bits_equal, _field
from test_gpu_track import _gazebo_map, _synthetic_map
from test_gpu_track_field import LAT2, LAT3, _grid_field, _lat
from test_locate_ref import TH2, TRUE2, TRUE3, depth3, ranges2
from test_track_ref import CAM, OFF2, depth_image, pose6, pose12, rot, scene2, scene3

pytestmark = pytest.mark.gpu
F32 = np.float32
BLOCK, CHUNK = 256, 2048                                 # csrc/cover.h: threads of a workgroup (both scans), points of a chunk
_CACHE = {}


def df2():
    if "df2" not in _CACHE:
        _CACHE["df2"] = _grid_field(scene2, LAT2)
        _CACHE["dist2"] = _CACHE["df2"].get()[0].ravel()
    return _CACHE["df2"], _CACHE["dist2"]


def df3():
    if "df3" not in _CACHE:
        _CACHE["df3"] = _grid_field(scene3, LAT3)
        _CACHE["dist3"] = _CACHE["df3"].get()[0].ravel()
    return _CACHE["df3"], _CACHE["dist3"]


def _free(shape, origin=None, step=0.02):
    """(field, dist) without a surface: every point is traversable."""
    origin = origin if origin is not None else (0.0,) * len(shape)
    return _field(np.ones(int(np.prod(shape)), F32), shape, origin, step)


def _cover(df):
    import gpismap_amd
    return gpismap_amd.Coverage().reset(df)


def _seen2_first():
    """Coverage of LAT2 after the scan from TRUE2 (device), checked against the reference once."""
    if "cv2" not in _CACHE:
        df, _ = df2()
        shape, origin, step = _lat(df)
        cv = _cover(df).integrate_scan(TH2, ranges2(), TRUE2, OFF2)
        ref = cover_ref.integrate_scan(np.zeros(int(np.prod(shape)), bool), shape, origin, step, TH2, ranges2(), TRUE2, OFF2, step, GAP)
        got = cv.get()
        assert got.dtype == np.uint8 and got.shape == tuple(shape)[::-1] and np.array_equal(got.ravel(), ref.astype(np.uint8))
        _CACHE["cv2"] = (cv, ref)
    return _CACHE["cv2"]


def _check_frontiers(cv, df, dist, seen, stream=None, **opts):
    """frontiers() on the device against the reference on the same mask and the device's own dist: every array, every bit."""
    import gpismap_amd
    shape, origin, step = _lat(df)
    dim = len(shape)
    o = gpismap_amd.cover_opts(dim, step, **opts)
    out = cv.frontiers(df, points=True, stream=stream, **opts)
    ref = cover_ref.frontiers(seen, dist, shape, origin, step, o.clearance, o.min_size)
    assert out["npoints"] == ref["points"].size and out["ncomponents"] == ref["clusters"]
    for k, r in (("points", "points"), ("point_label", "point_label"), ("label", "label"), ("count", "count"), ("sums", "sums"),
                 ("box", "box"), ("rep_index", "rep")):
        assert out[k].dtype == ref[r].dtype and np.array_equal(out[k], ref[r]), (k, out[k][:8], ref[r][:8])
    assert out["rep"].dtype == F32 and out["rep"].shape == (ref["label"].size, dim) and _bits_equal(out["rep"], ref["rep_point"])
    assert out["centroid"].dtype == np.float64 and np.array_equal(out["centroid"].view(np.uint64), ref["centroid"].view(np.uint64))
    inf = cv.info()
    assert inf["frontiers"] == 1 and inf["points"] == out["npoints"] and inf["clusters"] == ref["label"].size
    assert inf["components"] == ref["clusters"] and (inf["rounds"] >= 1) == (out["npoints"] > 0)
    return out, ref


# ---- seen -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off2", [OFF2, (0.0, 0.05)])
def test_seen_bytes_2d_after_one_and_two_scans(off2):
    df, _ = df2()
    shape, origin, step = _lat(df)
    cv = _cover(df)
    assert cv.get().sum() == 0 and cv.info()["frames"] == 0
    ref = np.zeros(int(np.prod(shape)), bool)
    for k, (r, P) in enumerate(((ranges2(), TRUE2), (_masked(ranges2b(), 200), POSE2B))):
        assert cv.integrate_scan(TH2, r, P, off2) is cv
        ref = cover_ref.integrate_scan(ref, shape, origin, step, TH2, r, P, off2, step, GAP)
        got = cv.get().ravel()
        print("2-D off %s frame %d: %d seen" % (off2, k, ref.sum()))
        assert np.array_equal(got, ref.astype(np.uint8)), np.flatnonzero(got != ref)[:8]
        assert ref.sum() > 30000 and cv.info()["frames"] == k + 1
    # the options reach the rule: a larger back-off and a gap below the beam spacing (1 degree) see less / nothing
    cv.reset(df).integrate_scan(TH2, ranges2(), TRUE2, off2, back_off=0.2, clearance=0.5, max_gap=math.radians(1.5))
    r2 = cover_ref.integrate_scan(np.zeros(ref.size, bool), shape, origin, step, TH2, ranges2(), TRUE2, off2, 0.2, math.radians(1.5))
    assert np.array_equal(cv.get().ravel(), r2.astype(np.uint8)) and 0 < r2.sum() < ref.sum()
    cv.reset(df).integrate_scan(TH2, ranges2(), TRUE2, off2, max_gap=math.radians(0.5))
    assert cv.get().sum() == 0


def test_seen_bytes_3d_after_one_and_two_frames():
    df, _ = df3()
    shape, origin, step = _lat(df)
    cv = _cover(df)
    ref = np.zeros(int(np.prod(shape)), bool)
    P2 = pose12(rot([0.2, 1.0, 0.1], math.radians(12.0)), np.array([-0.3, 0.1, 0.05]))
    for k, (d, P) in enumerate(((depth3(), TRUE3), (depth_image(scene3, CAM, P2), P2))):
        cv.integrate_depth(d, P, CAM)
        before = ref.sum()
        ref = cover_ref.integrate_depth(ref, shape, origin, step, d, CAM, P, step)
        got = cv.get().ravel()
        print("3-D frame %d: %d seen" % (k, ref.sum()))
        assert np.array_equal(got, ref.astype(np.uint8)), np.flatnonzero(got != ref)[:8]
        assert ref.sum() > before + 10000


def test_seen_bytes_small_and_odd_lattices():
    th = np.radians(np.arange(0.0, 360.0, 1.0)).astype(F32)
    r = (1.0 + 0.5 * np.cos(3 * th.astype(np.float64))).astype(F32)
    r[20:140] = 0.0
    for shape in ((5, 3), (27, 19), (2, 2)):                       # 27 x 19 = 2 * 256 + 1 points
        origin, step = (-0.35, -0.2), 0.11
        df, _ = _free(shape, origin, step)
        P = pose6(0.4, (0.02 + 0.11 * (shape[0] // 2) - 0.35, 0.01))
        cv = _cover(df).integrate_scan(th, r, P, (0.03, -0.02), back_off=0.05)
        ref = cover_ref.scan_mask(shape, origin, step, th, r, P, (0.03, -0.02), 0.05, GAP)
        assert np.array_equal(cv.get().ravel(), ref.astype(np.uint8)) and ref.sum() > 0, (shape, ref.sum())
        assert ref.size < 20 or ref.sum() < ref.size
    cam = (40.0, 40.0, 15.5, 11.5, 32, 24)
    rng = np.random.default_rng(5)
    d = rng.uniform(0.5, 1.6, 32 * 24).astype(F32)
    d[::7] = 0.0
    d[3::11] = np.nan
    for shape in ((3, 3, 2), (19, 9, 3)):                           # 19 x 9 x 3 = 2 * 256 + 1 points
        origin, step = (-0.4, -0.2, 0.6), 0.09
        df, _ = _free(shape, origin, step)
        P = pose12(rot([1, -0.5, 0.2], 0.15), np.array([0.05, -0.02, -0.1]))
        cv = _cover(df).integrate_depth(d, P, cam, back_off=0.03)
        ref = cover_ref.depth_mask(shape, origin, step, d, cam, P, 0.03)
        assert np.array_equal(cv.get().ravel(), ref.astype(np.uint8)) and 0 < ref.sum() < ref.size, (shape, ref.sum())


def test_a_lattice_point_on_the_sensor_and_too_few_beams():
    shape, origin, step = (9, 7), (-0.4, -0.3), 0.1
    df, _ = _free(shape, origin, step)
    on = cover_ref.lattice_points([3 * 9 + 4], shape, origin, step)[0]
    P = pose6(0.3, (float(on[0]), float(on[1])))
    th = np.array([0.0, 0.02, 0.04], F32)
    for r in ([0.5, 0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]):
        r = np.array(r, F32)
        cv = _cover(df).integrate_scan(th, r, P, (0.0, 0.0), back_off=0.01)
        ref = cover_ref.scan_mask(shape, origin, step, th, r, P, (0.0, 0.0), 0.01, GAP)
        assert np.array_equal(cv.get().ravel(), ref.astype(np.uint8)) and bool(ref[3 * 9 + 4]) == (np.count_nonzero(r) >= 2)


def test_set_get_and_device_ptr():
    df, _ = _free((7, 5))
    cv = _cover(df)
    m = (np.arange(35) % 3 == 0)
    assert cv.set(m * 7) is cv                                      # any non-zero value is "seen"
    assert np.array_equal(cv.get().ravel(), m.astype(np.uint8)) and cv.get().shape == (5, 7)
    ptr = cv.device_ptr()
    cv.reset(df)
    assert cv.get().sum() == 0 and ptr != 0 and cv.device_ptr() == ptr          # (grow-only: the same lattice keeps its buffer)


# ---- frontiers --------------------------------------------------------------------------------------------------------------
def test_frontiers_of_the_pillar_scene():
    df, dist = df2()
    cv, seen = _seen2_first()
    out, ref = _check_frontiers(cv, df, dist, seen, clearance=0.1)
    assert out["label"].size == 2 and np.all(out["count"] >= 50)
    out, _ = _check_frontiers(cv, df, dist, seen, clearance=0.06, min_size=1)
    assert out["label"].size > 2 and out["ncomponents"] == out["label"].size
    out, _ = _check_frontiers(cv, df, dist, seen, clearance=0.06)
    assert out["label"].size == 2 and out["ncomponents"] > 2
    # after the second scan nothing is left
    cvb = _cover(df).set(seen).integrate_scan(TH2, ranges2b(), POSE2B, OFF2)
    both = cover_ref.integrate_scan(seen, *_lat(df), TH2, ranges2b(), POSE2B, OFF2, LAT2["step"], GAP)
    out, _ = _check_frontiers(cvb, df, dist, both, clearance=0.1)
    assert out["npoints"] == 0 and out["label"].size == 0


def test_frontiers_3d_scene():
    df, dist = df3()
    shape, origin, step = _lat(df)
    seen = cover_ref.integrate_depth(np.zeros(dist.size, bool), shape, origin, step, depth3(), CAM, TRUE3, step)
    cv = _cover(df).set(seen)
    out, _ = _check_frontiers(cv, df, dist, seen)
    assert out["label"].size >= 1 and out["npoints"] > 5000


def test_zero_and_one_frontier_point_and_corner_touch():
    df, dist = _free((6, 5))
    cv = _cover(df)
    for m in (np.zeros(30, bool), np.ones(30, bool)):              # nothing seen; everything seen (the border raises nothing)
        out, _ = _check_frontiers(cv.set(m), df, dist, m, clearance=0.5, min_size=1)
        assert out["npoints"] == 0 and out["ncomponents"] == 0 and out["points"].size == 0
    one = np.zeros(30, bool)
    one[2 * 6 + 3] = True
    out, _ = _check_frontiers(cv.set(one), df, dist, one, clearance=0.5, min_size=1)
    assert out["npoints"] == 1 and out["label"].tolist() == [15] and out["rep_index"].tolist() == [15]
    out, _ = _check_frontiers(cv, df, dist, one, clearance=0.5)         # below min_size: labelled, not in the table
    assert out["npoints"] == 1 and out["ncomponents"] == 1 and out["label"].size == 0
    m = np.ones((5, 6), bool)
    m[1, 1] = m[2, 2] = False                                       # two holes touching at a corner: one component
    out, _ = _check_frontiers(cv.set(m), df, dist, m.ravel(), clearance=0.5, min_size=1)
    assert out["ncomponents"] == 1 and out["count"].tolist() == [6]
    m = np.zeros((5, 6), bool)
    m[0, 0] = m[1, 1] = m[3, 3] = m[3, 5] = True                    # frontier points touching diagonally / two apart
    out, _ = _check_frontiers(cv.set(m), df, dist, m.ravel(), clearance=0.5, min_size=1)
    assert out["point_label"].tolist() == [0, 0, 21, 23]
    # 3-D: diagonal touch through a cube's corner
    df3_, dist3_ = _free((4, 4, 3))
    m = np.zeros((3, 4, 4), bool)
    m[0, 0, 0] = m[1, 1, 1] = m[2, 3, 3] = True
    out, _ = _check_frontiers(_cover(df3_).set(m), df3_, dist3_, m.ravel(), clearance=0.5, min_size=1)
    assert out["ncomponents"] == 2 and out["count"].tolist() == [2, 1]


@pytest.mark.parametrize("count", [BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_frontier_counts_around_the_scan_sizes(count):
    """`count` isolated columns' worth of seen points on even columns (each has an unseen neighbour): the list is exactly that long."""
    shape = (600, 20)
    df, dist = _free(shape)
    cand = np.flatnonzero((np.arange(12000) % 600) % 2 == 0)
    m = np.zeros(12000, bool)
    m[cand[np.sort(np.random.default_rng(count).permutation(cand.size)[:count])]] = True
    out, _ = _check_frontiers(_cover(df).set(m), df, dist, m, clearance=0.1, min_size=1)
    assert out["npoints"] == count


@pytest.mark.parametrize("shape", [(CHUNK, BLOCK - 1), (CHUNK, BLOCK), (CHUNK + 1, BLOCK)])
def test_chunk_counts_around_the_offset_scan_width(shape):
    """255, 256 and 257 chunks of 2048 points: the single-workgroup scan of the chunk counts at, and one pass beyond, its width.
    Seen rows (each point of which has an unseen neighbour above or below) at the first, a middle and the last row, and the last
    lattice point's neighbour."""
    df, dist = _free(shape)
    m = np.zeros(shape[::-1], bool)
    m[0, :] = m[shape[1] // 2, : shape[0] // 2] = m[-1, ::3] = True
    m[-2, -1] = True
    out, _ = _check_frontiers(_cover(df).set(m), df, dist, m.ravel(), clearance=0.1, min_size=4)
    assert out["npoints"] > shape[0] and out["points"][-1] >= (shape[1] - 1) * shape[0]


def _spiral(n):
    """A one-point-wide square spiral of seen points on an n x n lattice, its arms one unseen point apart: one long component."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def test_spiral_many_rounds_and_the_round_limit():
    import gpismap_amd
    n = 95
    df, dist = _free((n, n))
    m = _spiral(n)
    cv = _cover(df).set(m)
    out, ref = _check_frontiers(cv, df, dist, m.ravel(), clearance=0.1)
    assert out["ncomponents"] == 1 and out["count"].tolist() == [out["npoints"]] and out["npoints"] > 4000 and cv.info()["rounds"] > 1
    print("spiral of %d points: %d rounds" % (m.sum(), cv.info()["rounds"]))
    # the limit: GPIS_ERR_LIMIT, and the holder is left without frontiers
    o = gpismap_amd.cover_opts(2, 0.02, clearance=0.1, max_rounds=1)
    L = gpismap_amd.lib()
    assert L.gpis_cover_frontiers(cv.h, df.h, C.byref(o), None) == -4
    assert cv.info()["frontiers"] == 0 and L.gpis_cover_counts(cv.h, None, None, None) == -3
    assert L.gpis_cover_get_frontiers(cv.h, None, None, None, None, None, None, None) == -3
    # enough rounds: the same result as without a limit
    out2 = cv.frontiers(df, points=True, clearance=0.1, max_rounds=10000)
    assert np.array_equal(out2["point_label"], ref["point_label"])


def test_components_across_every_chunk_and_block_border():
    """Stripes: every second row seen, so each seen row is one dense component running through the 256-point and 2048-point borders of
    the flat index; in 3-D a seen plane does the same."""
    df, dist = _free((600, 21))
    m = np.zeros((21, 600), bool)
    m[::2, :] = True
    m[3, 100] = True                                               # joins rows 2 and 4
    out, _ = _check_frontiers(_cover(df).set(m), df, dist, m.ravel(), clearance=0.1)
    assert out["ncomponents"] == 10 and out["count"].max() == 1201
    df3_, dist3_ = _free((40, 30, 5))
    m = np.zeros((5, 30, 40), bool)
    m[2] = True
    m[0, ::2, ::2] = True
    out, _ = _check_frontiers(_cover(df3_).set(m), df3_, dist3_, m.ravel(), clearance=0.1, min_size=1)
    assert out["count"].max() == 1200 and out["ncomponents"] == 1 + 15 * 20


def test_clearance_and_nan_distances_gate_the_flags():
    shape, origin, step = (40, 33), (0.0, 0.0), 0.1
    f = _balls(shape, origin, step, [((12.0, 15.0), 5.5), ((30.0, 8.0), 3.0)])
    df, dist = _field(f, shape, origin, step)
    rng = np.random.default_rng(2)
    m = rng.random(40 * 33) < 0.6
    cv = _cover(df).set(m)
    for cl in (0.05, 0.2, 0.45):
        out, _ = _check_frontiers(cv, df, dist, m, clearance=cl, back_off=0.01, min_size=1)
        assert out["npoints"] > 0


# ---- the restricted field -----------------------------------------------------------------------------------------------------
def test_restrict_and_plan_through_seen_space_only():
    import gpismap_amd
    df, dist = df2()
    shape, origin, step = _lat(df)
    cv, seen = _seen2_first()
    r = cv.restrict(df)
    assert r is not df and r.info() == df.info()
    rd, rsite, rf = r.get()
    assert rf is None and _bits_equal(rd.ravel(), cover_ref.restrict(seen, dist, -float(F32(step))))
    assert np.array_equal(rsite, df.get()[1])
    mine = gpismap_amd.DistanceField()
    assert cv.restrict(df, out=mine, unseen_dist=-1.5) is mine
    assert _bits_equal(mine.get()[0].ravel(), cover_ref.restrict(seen, dist, -1.5))
    # the planner on the restricted field: plan_ref's bits, and no path point is unseen
    fr = cover_ref.frontiers(seen, dist, shape, origin, step, 0.1, 8)
    pl = r.plan(fr["rep_point"], clearance=0.1)
    o = gpismap_amd.plan_opts(2, F32(step), clearance=0.1)
    pb = plan_ref.Problem(rd.ravel(), shape, origin, step, fr["rep_point"], clearance=o.clearance, margin=o.margin, gain=o.gain,
                          connectivity=o.connectivity)
    rc = plan_ref.solve_dijkstra(pb)
    rp = plan_ref.policy(pb, rc)
    cost, pol = pl.get()
    assert _bits_equal(cost.ravel(), rc) and np.array_equal(pol.ravel(), rp)
    assert not np.isfinite(rc[~seen]).any() and np.isfinite(rc[seen]).sum() > 30000
    starts = np.array([TRUE2[:2], [1.0, 1.5], [-2.0, 0.0]], F32)
    paths, sc, st = pl.paths(starts)
    off, pts, rsc, rst = plan_ref.paths(pb, rc, rp, starts, int(np.prod(shape)))
    assert np.array_equal(st, rst) and st[0] == 0 and _bits_equal(np.concatenate(paths), pts)
    ok, ijk = plan_ref.snap(pts, shape, origin, step)
    assert ok.all() and seen[ijk[:, 1] * shape[0] + ijk[:, 0]].all()
    # the sampler runs on it unchanged
    assert np.isfinite(r.sample(starts)).all()


def test_explore_is_the_composition_of_the_references():
    df, dist = df2()
    shape, origin, step = _lat(df)
    cv, seen = _seen2_first()
    path, status, clusters = df.explore(cv, TRUE2[:2], clearance=0.1)
    rpath, rstatus, rfr = cover_ref.explore(seen, dist, shape, origin, step, TRUE2[:2], 0.1, margin=4 * float(F32(step)))
    assert status == rstatus == 0 and _bits_equal(path, rpath) and path.shape[0] > 10
    assert np.array_equal(clusters["label"], rfr["label"]) and _bits_equal(clusters["rep"], rfr["rep_point"])
    assert any(_bits_equal(path[-1], r) for r in rfr["rep_point"])
    # everything seen: nothing to explore
    cvb = _cover(df).set(seen).integrate_scan(TH2, ranges2b(), POSE2B, OFF2)
    p2, st2, c2 = df.explore(cvb, TRUE2[:2], clearance=0.1)
    assert st2 == 4 and p2.shape == (0, 2) and c2["label"].size == 0


# ---- streams, maps, errors --------------------------------------------------------------------------------------------------
def test_same_bits_on_a_callers_stream():
    import torch
    df, dist = df2()
    cv, seen = _seen2_first()
    st = torch.cuda.Stream()
    cvs = _cover(df).integrate_scan(TH2, ranges2(), TRUE2, OFF2, stream=st.cuda_stream)
    assert np.array_equal(cvs.get().ravel(), seen.astype(np.uint8))
    _check_frontiers(cvs, df, dist, seen, stream=st.cuda_stream, clearance=0.1)
    r = cvs.restrict(df, stream=st.cuda_stream)
    assert _bits_equal(r.get()[0].ravel(), cover_ref.restrict(seen, dist, -float(F32(LAT2["step"]))))
    df_, _ = df3()
    shape, origin, step = _lat(df_)
    cv3 = _cover(df_).integrate_depth(depth3(), TRUE3, CAM, stream=st.cuda_stream)
    ref = cover_ref.depth_mask(shape, origin, step, depth3(), CAM, TRUE3, step)
    assert np.array_equal(cv3.get().ravel(), ref.astype(np.uint8))


def test_map_level_calls_use_the_maps_camera_and_offset():
    g2, f2 = _gazebo_map(ids=range(1))
    shape, origin, step = (120, 90), (-6.0, -4.5), 0.1
    df, _ = _free(shape, origin, step)
    fr = f2[0]
    P = pose6(0.3, (0.2, -0.1))
    cv = _cover(df)
    assert g2.cover_scan(cv, fr["thetas"], fr["ranges"], P) is cv
    ref = cover_ref.scan_mask(shape, origin, step, fr["thetas"], fr["ranges"], P, OFF2, step, GAP)
    assert np.array_equal(cv.get().ravel(), ref.astype(np.uint8)) and ref.sum() > 100
    gm = _synthetic_map(frames=1)
    df3_, _ = _free(SYN["shape"], SYN["origin"], SYN["step"])
    shape, origin, step = _lat(df3_)
    cv3 = _cover(df3_)
    d = replay.synthetic_depth(1)
    assert gm.cover_depth(cv3, d, replay.IDENTITY_POSE) is cv3
    ref = cover_ref.depth_mask(shape, origin, step, d, (568.0, 568.0, 310.0, 224.0, 640, 480), replay.IDENTITY_POSE, step)
    assert np.array_equal(cv3.get().ravel(), ref.astype(np.uint8)) and ref.sum() > 10000


def test_error_paths():
    import gpismap_amd
    L = gpismap_amd.lib()
    ARG, STATE = -1, -3
    df, _ = _free((7, 5), step=0.5)
    other, _ = _free((7, 6), step=0.5)
    shifted, _ = _free((7, 5), origin=(0.5, 0.0), step=0.5)
    df3_, _ = _free((4, 3, 2), step=0.5)
    empty = gpismap_amd.DistanceField()
    fp = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    th, r, P6, off = np.array([0.0, 0.1], F32), np.array([1.0, 1.0], F32), pose6(0.0, (1.0, 1.0)), np.zeros(2, F32)
    P12 = pose12(np.eye(3), np.zeros(3))
    cam = gpismap_amd.gpis_cam(10.0, 10.0, 1.5, 1.5, 4, 4)
    d16 = np.ones(16, F32)
    buf = np.zeros(64, np.uint8)
    ub = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    o = gpismap_amd.cover_opts(2, 0.5)

    # a holder that was never reset
    cv = gpismap_amd.Coverage()
    assert cv.info()["valid"] == 0 and cv.device_ptr() == 0
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, fp(P6), fp(off), C.byref(o), None) == STATE
    assert L.gpis3_cover_depth(None, cv.h, C.byref(cam), fp(d16), fp(P12), C.byref(o), None) == STATE
    assert L.gpis_cover_frontiers(cv.h, df.h, C.byref(o), None) == STATE and L.gpis_cover_frontiers(cv.h, df.h, None, None) == STATE
    assert L.gpis_cover_set(cv.h, ub(buf), 35) == STATE and L.gpis_cover_get(cv.h, ub(buf), 35) == STATE
    assert L.gpis_cover_restrict(cv.h, df.h, other.h, -1.0, None) == STATE
    with pytest.raises(gpismap_amd.GpisError):
        cv.get()
    # a field without a result
    assert L.gpis_cover_reset(cv.h, empty.h) == STATE and L.gpis_cover_reset(cv.h, None) == ARG and L.gpis_cover_reset(None, df.h) == ARG
    cv.reset(df)
    assert L.gpis_cover_frontiers(cv.h, empty.h, C.byref(o), None) == STATE
    assert L.gpis_cover_restrict(cv.h, empty.h, other.h, -1.0, None) == STATE
    # counts before any frontiers
    assert L.gpis_cover_counts(cv.h, None, None, None) == STATE
    # another lattice: size, origin, dim
    for wrong in (other, shifted, df3_):
        assert L.gpis_cover_frontiers(cv.h, wrong.h, C.byref(o), None) == ARG
        assert L.gpis_cover_restrict(cv.h, wrong.h, empty.h, -1.0, None) == ARG
    assert L.gpis3_cover_depth(None, cv.h, C.byref(cam), fp(d16), fp(P12), None, None) == ARG          # a depth frame on a 2-D lattice
    cv3 = gpismap_amd.Coverage().reset(df3_)
    assert L.gpis2_cover_scan(None, cv3.h, fp(th), fp(r), 2, fp(P6), fp(off), None, None) == ARG
    # restricting in place, a non-finite fill
    assert L.gpis_cover_restrict(cv.h, df.h, df.h, -1.0, None) == ARG
    assert L.gpis_cover_restrict(cv.h, df.h, other.h, float("nan"), None) == ARG
    assert L.gpis_cover_restrict(cv.h, df.h, other.h, float("inf"), None) == ARG and other.info()["shape"] == (7, 6)
    with pytest.raises(gpismap_amd.GpisError):
        cv.restrict(df, out=df)
    # bad options
    for bad in (dict(clearance=0.5), dict(clearance=0.1), dict(back_off=-0.1), dict(max_gap=0.0), dict(max_gap=1.6), dict(min_size=0),
                dict(max_rounds=-1), dict(clearance=float("nan"))):
        b = gpismap_amd.cover_opts(2, 0.5, **bad)
        assert L.gpis_cover_frontiers(cv.h, df.h, C.byref(b), None) == ARG, bad
        assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, fp(P6), fp(off), C.byref(b), None) == ARG, bad
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.cover_opts(2, 0.5, nonsense=1)
    # wrong array sizes, missing arguments, bad frames and poses
    assert L.gpis_cover_set(cv.h, ub(buf), 34) == ARG and L.gpis_cover_get(cv.h, ub(buf), 36) == ARG
    assert L.gpis_cover_set(cv.h, None, 35) == ARG and L.gpis_cover_get(cv.h, None, 35) == ARG
    with pytest.raises(gpismap_amd.GpisError):
        cv.set(np.zeros(34))
    with pytest.raises(gpismap_amd.GpisError):
        cv3.integrate_depth(np.ones(15, F32), P12, (10.0, 10.0, 1.5, 1.5, 4, 4))
    with pytest.raises(gpismap_amd.GpisError):
        cv.integrate_scan(th, r[:1], P6, (0.0, 0.0))
    with pytest.raises(gpismap_amd.GpisError):
        cv.integrate_scan(th, r, P6[:5], (0.0, 0.0))
    with pytest.raises(gpismap_amd.GpisError):
        cv.integrate_scan(th, r, P6, None)                           # no offset and no map
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 0, fp(P6), fp(off), None, None) == ARG
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, fp(P6), None, None, None) == ARG
    assert L.gpis2_cover_scan(None, cv.h, None, fp(r), 2, fp(P6), fp(off), None, None) == ARG
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, None, fp(off), None, None) == ARG
    bad6 = P6.copy()
    bad6[1] = np.nan
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, fp(bad6), fp(off), None, None) == ARG
    assert L.gpis2_cover_scan(None, cv.h, fp(np.array([0.0, np.inf], F32)), fp(r), 2, fp(P6), fp(off), None, None) == ARG
    assert L.gpis3_cover_depth(None, cv3.h, None, fp(d16), fp(P12), None, None) == ARG
    zero_fx = gpismap_amd.gpis_cam(0.0, 10.0, 1.5, 1.5, 4, 4)
    assert L.gpis3_cover_depth(None, cv3.h, C.byref(zero_fx), fp(d16), fp(P12), None, None) == ARG
    # none of this touched the mask or the lattice
    assert cv.get().sum() == 0 and cv.info()["frames"] == 0 and cv3.info()["dim"] == 3
    assert L.gpis2_cover_scan(None, cv.h, fp(th), fp(r), 2, fp(P6), fp(off), None, None) == 0 and cv.info()["frames"] == 1
