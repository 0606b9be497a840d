"""The trajectory optimiser's host side and its reference (tests/traj_ref.py): the exported C entries that need no device, the
closed form of inverse(tridiag(-1, 2, -1)) against a float64 solve, the resampling, the defective variants on the inputs the
GPU cases use (tests/traj_cases.py), and the geometry the default options reach on two ball scenes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import plan_ref
import traj_cases
import traj_ref

F32 = np.float32
U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x", "status", "iterations", "length", "smooth", "obstacle", "min_dist", "nonfinite", "collides")


def _same(a, b):
    for k in KEYS:
        u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if u.dtype == F32:
            u, v = u.view(U32), v.view(U32)
        if not np.array_equal(u, v):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _scene(dim):
    sc = traj_cases.scene(dim)
    dist = traj_cases.ref_dist(sc)
    return sc, dist, traj_cases.plan(sc, dist)


# ---- exported symbols and host-only entries ------------------------------------------------------------------------------------
def test_exports_and_default_opts():
    import gpismap_amd
    L = C.CDLL(gpismap_amd.LIB_PATH)                     # loads without a GPU
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpismap_amd.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(gpis_traj_[0-9a-z_]*)\s*\(", hdr))
    assert names == {"gpis_traj_default_opts", "gpis_traj_create", "gpis_traj_destroy", "gpis_traj_from_paths", "gpis_traj_set",
                     "gpis_traj_optimize", "gpis_traj_info", "gpis_traj_get", "gpis_traj_device"}
    for n in sorted(names):
        assert hasattr(L, n), "missing symbol " + n
    o = gpismap_amd.gpis_traj_opts()
    f = L.gpis_traj_default_opts
    f.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_traj_opts)]
    for dim, step in [(2, 0.25), (3, 0.1)]:
        assert f(dim, step, C.byref(o)) == 0
        want = traj_ref.default_opts(dim, step)
        got = {k: getattr(o, k) for k in traj_ref.OPT_NAMES}
        for k in traj_ref.OPT_NAMES:
            assert F32(got[k]).view(U32) == F32(want[k]).view(U32) if k not in ("iters", "sub") else got[k] == want[k], k
    assert (o.iters, o.sub) == (100, 3)
    assert f(2, 0.25, C.byref(o)) == 0 and (o.clearance, o.margin, o.w_smooth, o.max_move) == (0.0, 0.75, 1.0, 0.125)
    assert f(2, 0.25, None) == -1 and f(1, 0.25, C.byref(o)) == -1 and f(4, 0.25, C.byref(o)) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert f(3, bad, C.byref(o)) == -1
    # NULL handles never reach a device
    L.gpis_traj_set.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int]
    L.gpis_traj_from_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.gpis_traj_optimize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gpismap_amd.gpis_traj_opts), C.c_void_p]
    L.gpis_traj_info.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.gpis_traj_get.argtypes = [C.c_void_p] * 10
    L.gpis_traj_device.argtypes = [C.c_void_p] * 4
    assert L.gpis_traj_set(None, None, 1, 8, 2) == -1 and L.gpis_traj_from_paths(None, None, 8) == -1
    assert L.gpis_traj_optimize(None, None, None, None) == -1 and L.gpis_traj_info(None, None, 0) == -1
    assert L.gpis_traj_get(*[None] * 10) == -1 and L.gpis_traj_device(*[None] * 4) == -1
    assert gpismap_amd.traj_opts(2, 0.25, iters=7).iters == 7
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.traj_opts(2, 0.25, speed=1)


# ---- closed form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 62, 63, 254])
def test_closed_form_against_float64_solve(n):
    """delta_i is a sum of n products of an exact coefficient c_ij <= (n + 1)^2 / 4 with g_j, then one division.  Each product and
    each of the n - 1 additions rounds once (relative 2^-24 of a partial sum bounded by S_i = sum_j c_ij |g_j|), the division once
    more: |delta_i - exact| <= (n + 1) 2^-24 S_i / (n + 1) (1 + small), taken as (n + 2) 2^-24 S_i / (n + 1)."""
    rng = np.random.default_rng(n)
    g = rng.normal(0, 1, (5, n, 3)).astype(F32)
    d = traj_ref.metric(g).astype(np.float64)
    A = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    exact = np.linalg.solve(A, g.astype(np.float64).transpose(1, 0, 2).reshape(n, -1)).reshape(n, 5, 3).transpose(1, 0, 2)
    i = np.arange(1, n + 1)
    c = np.minimum.outer(i, i) * (n + 1 - np.maximum.outer(i, i))
    S = np.einsum("ij,mja->mia", c.astype(np.float64), np.abs(g.astype(np.float64))) / (n + 1)
    bound = (n + 2) * 2.0 ** -24 * S + 1e-300
    assert np.all(np.abs(d - exact) <= bound), float(np.max(np.abs(d - exact) / bound))
    assert np.array_equal(c, np.round(np.linalg.inv(A) * (n + 1)).astype(np.int64))


# ---- resampling ----------------------------------------------------------------------------------------------------------------
def test_resampling():
    q = np.array([[0, 0], [1, 0], [2, 0], [2, 1], [3, 2]], F32) * F32(0.25)
    for N in (3, 5, 9, 64):
        x = traj_ref.resample_one(q, N)
        assert np.array_equal(x[0], q[0]) and np.array_equal(x[-1], q[-1]) and x.dtype == F32
    # L = 1: N copies; L = 2: equal steps along the one segment
    assert np.array_equal(traj_ref.resample_one(q[:1], 4), np.repeat(q[:1], 4, axis=0))
    x = traj_ref.resample_one(q[:2], 5)
    assert np.array_equal(x[:, 0], np.array([0, 0.0625, 0.125, 0.1875, 0.25], F32)) and np.all(x[:, 1] == 0)
    # waypoints that land exactly on path points: 4 unit segments of 0.25 resampled to 5 and to 9 points
    r = np.array([[0, 0], [1, 0], [2, 0], [2, 1], [2, 2]], F32) * F32(0.25)
    assert np.array_equal(traj_ref.resample_one(r, 5), r)
    x9 = traj_ref.resample_one(r, 9)
    assert np.array_equal(x9[::2], r) and np.array_equal(x9[1], F32([0.125, 0])) and np.array_equal(x9[5], F32([0.5, 0.125]))
    # equidistant along the polyline: the arc position of waypoint i is i S / (N - 1) up to the rounding of s (L serial additions,
    # each within 2^-24 S), of t_i and of the interpolation (a few 2^-24 S more): 2^-24 S (L + 8)
    sc, dist, (pb, rc, pol, off, pts, scost, st) = _scene(2)
    for p in np.flatnonzero(st == 0)[:12]:
        qq = pts[off[p]:off[p + 1]]
        L = qq.shape[0]
        if L < 2:
            continue
        s64 = np.concatenate([[0], np.cumsum(np.sqrt((np.diff(qq.astype(np.float64), axis=0) ** 2).sum(1)))])
        for N in (4, 64, 255):
            x = traj_ref.resample_one(qq, N).astype(np.float64)
            # arc position of x_i: project onto its segment
            t = np.arange(N) * s64[-1] / (N - 1)
            k = np.clip(np.searchsorted(s64, t, side="right") - 1, 0, L - 2)
            pos = s64[k] + np.sqrt(((x - qq[k]) ** 2).sum(1))
            assert np.max(np.abs(pos - t)) <= 2.0 ** -24 * s64[-1] * (L + 8), (p, N)
    x, ist = traj_ref.resample(off, pts, st, 16)
    assert np.all(ist[st != 0] == 2) and np.all(np.isnan(x[st != 0])) and np.all(np.isfinite(x[st == 0]))
    one = np.flatnonzero((off[1:] - off[:-1]) == 1)
    assert one.size >= 1 and np.all(x[one[0]] == x[one[0], 0])


# ---- the defective variants on the GPU cases' inputs ---------------------------------------------------------------------------
def test_populations_and_defective_variants():
    sc, dist, (pb, rc, pol, off, pts, scost, st) = _scene(2)
    shape, origin, step = sc["shape"], sc["origin"], sc["step"]
    assert set(np.unique(st)) >= {0, 1, 2} and (st == 0).sum() >= 30
    # every planner status: 3 from a start enclosed by a shell, 4 from paths cut at max_points, whose points are kept but give
    # no input (NaN waypoints, input status 2, every result column NaN or 0)
    for dm in (2, 3):
        ssc = traj_cases.status_scene(dm)
        sdist = traj_cases.ref_dist(ssc)
        batches = traj_cases.status_paths(ssc, sdist)
        traj_cases.check_status_paths(batches)
        for o4, p4, s4 in batches:
            x4, i4 = traj_ref.resample(o4, p4, s4, 17)
            assert np.array_equal(i4 == 0, s4 == 0) and np.all(np.isnan(x4[s4 != 0])) and np.all(np.isfinite(x4[s4 == 0]))
            r4 = traj_ref.optimize(sdist, ssc["shape"], ssc["origin"], ssc["step"], x4, i4, dict(iters=2))
            bad = s4 != 0
            assert np.all(r4["status"][bad] == 2) and np.all(np.isnan(r4["length"][bad])) and np.all(np.isnan(r4["min_dist"][bad]))
            assert not r4["iterations"][bad].any() and not r4["nonfinite"][bad].any() and not r4["collides"][bad].any()
            assert np.all(r4["status"][~bad] <= 1)
    # planner paths, default options: the trust region, early stops and capped trajectories in one batch
    x, ist = traj_ref.resample(off, pts, st, 64)
    tr = {}
    ref = traj_ref.optimize(dist, shape, origin, step, x, ist, None, trace=tr)
    ok = ist == 0
    assert (ref["status"][ok] == 0).sum() >= 3 and (ref["status"][ok] == 1).sum() >= 3 and np.all(ref["status"][~ok] == 2)
    early = ref["iterations"][ok & (ref["status"] == 0)]
    assert early.min() >= 1 and early.max() < 100 and len(set(early.tolist())) >= 2
    # hand-made waypoints: every branch of step 1
    hx, hopts, names = traj_cases.hand_made(sc, dist, 64)
    ht = {}
    href = traj_ref.optimize(dist, shape, origin, step, hx, None, dict(hopts, iters=5), trace=ht)
    k = {n: i for i, n in enumerate(names)}
    assert ht["trust"][k["zigzag"]] and ht["inside"][k["through"]] and ht["nonfinite"][k["leaves"]]
    assert ht["e_zero"][k["exact"]] and ht["e_margin"][k["exact"]]
    assert href["status"][k["nan"]] == 2 and href["status"][k["free"]] == 0 and href["iterations"][k["free"]] == 1
    assert href["collides"][k["through"]] == 1 and href["nonfinite"][k["leaves"]] > 0 and href["nonfinite"][k["last"]] == 0
    assert np.array_equal(href["x"][k["nan"]].view(U32), hx[k["nan"]].view(U32))
    # every defective variant changes at least one bit of what the GPU cases compare
    for v in traj_ref.VARIANTS:
        if v == "search_lt":
            # On the two ball scenes this variant does not show, which is asserted here and holds for those scenes only: where a
            # waypoint lands exactly on Q_k the variant computes Q_{k-1} + 1 (Q_k - Q_{k-1}), and on their lattices (step 0.25:
            # exact floats; origin 0 and step 0.2) that difference does not round at the landing points.  On a lattice with
            # origin -0.05 and step 0.1 it does round, and the variant changes bits on real planner paths;
            # tests/test_gpu_traj.py runs the device on exactly these paths, which pins its search.
            for dm in (2, 3):
                _, _, (_, _, _, o2, p2, _, s2) = _scene(dm)
                for N in traj_cases.NS:
                    a, b = traj_ref.resample(o2, p2, s2, N), traj_ref.resample(o2, p2, s2, N, variant=v)
                    assert np.array_equal(a[0].view(U32), b[0].view(U32))
            osc = traj_cases.offgrid_scene()
            ost = np.stack([traj_cases.world(osc, c) for c in traj_cases.OFFGRID_STARTS])
            _, _, _, o2, p2, _, s2 = traj_cases.plan(osc, traj_cases.ref_dist(osc), ost)
            assert np.all(s2 == 0)
            for N in traj_cases.OFFGRID_NS:
                a, b = traj_ref.resample(o2, p2, s2, N), traj_ref.resample(o2, p2, s2, N, variant=v)
                differ = (a[0].view(U32) != b[0].view(U32)).any(axis=(1, 2))
                assert differ.any() and not differ.all(), (v, N)
            continue
        a = traj_ref.optimize(dist, shape, origin, step, x, ist, None, variant=v)
        b = traj_ref.optimize(dist, shape, origin, step, hx, None, dict(hopts, iters=5), variant=v)
        assert not (_same(a, ref) and _same(b, href)), v


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 32), (2, 64), (3, 32), (3, 64)])
def test_geometry_with_default_options(dim, N):
    """With the defaults: no trajectory collides whose lattice path kept dist >= clearance + margin / 2, every trajectory is
    shorter than its lattice path and its largest |a_i| is below that of the resampled input."""
    sc, dist, (pb, rc, pol, off, pts, scost, st) = _scene(dim)
    shape, origin, step = sc["shape"], sc["origin"], sc["step"]
    o = traj_ref.default_opts(dim, step)
    x, ist = traj_ref.resample(off, pts, st, N)
    r = traj_ref.optimize(dist, shape, origin, step, x, ist)
    ok = (ist == 0) & ((off[1:] - off[:-1]) > 1)
    assert ok.sum() >= 30
    okp, ijk = plan_ref.snap(pts, shape, origin, step)
    pd = dist[(ijk[:, 2] * shape[1] + ijk[:, 1]) * shape[0] + ijk[:, 0]]
    m = len(st)
    pmin = np.array([pd[off[k]:off[k + 1]].min() if off[k + 1] > off[k] else np.nan for k in range(m)])
    plen = np.array([np.sqrt((np.diff(pts[off[k]:off[k + 1]].astype(np.float64), axis=0) ** 2).sum(1)).sum() for k in range(m)])
    need = ok & (pmin >= o["clearance"] + o["margin"] / 2)
    assert need.sum() >= 20 and np.all(r["collides"][need] == 0)
    assert np.all(r["length"][ok] < plen[ok])
    assert np.all(traj_ref.max_bend(r["x"][ok]) < traj_ref.max_bend(x[ok]))
    print("dim %d N %d: %d trajectories, %d with a clear lattice path, collide after %d, mean length %.4f of the path's, mean max|a| "
          "%.4f of the input's, min_dist >= %.3f steps" % (dim, N, ok.sum(), need.sum(), r["collides"][ok].sum(),
          float(np.mean(r["length"][ok] / plen[ok])), float(np.mean(traj_ref.max_bend(r["x"][ok]) / traj_ref.max_bend(x[ok]))),
          float(r["min_dist"][ok].min() / step)))
