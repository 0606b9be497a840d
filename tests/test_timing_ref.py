"""The time parametrisation's host side and its reference (tests/timing_ref.py) on the CPU: the exported C entries that need no
device, hand-computed cases, the populations the shared cases (tests/timing_cases.py) must reach, the limits the speed profile
keeps, the defective variants on the inputs the GPU cases use, and the closure with the controller's model (tests/mppi_ref.py)
on the two ball scenes: the control sequences drive the model through the timed positions."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import mppi_ref
import timing_cases as tc
import timing_ref as tr
import traj_cases
import traj_ref

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_timing_default_opts", "gpis_timing_time", "gpis_timing_info", "gpis_timing_get", "gpis_timing_controls",
         "gpis_timing_follow"}
TKEYS = ("v", "t", "limiter", "status", "duration", "max_speed", "max_curvature", "limiter_counts")
CKEYS = ("U", "heading0", "p0", "clamped")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a.view(np.uint64) if a.dtype == F64 else a


def _same(a, b, keys):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


@functools.lru_cache(maxsize=None)
def _scene(dim):
    sc = traj_cases.scene(dim)
    dist = traj_cases.ref_dist(sc)
    return sc, dist, (dist, sc["shape"], sc["origin"], sc["step"])


def _status(x):
    return np.where(np.isfinite(x).all(axis=(1, 2)), 0, 2).astype(np.uint8)


# ---- exported symbols and host-only entries ------------------------------------------------------------------------------------
def test_exports_and_default_opts():
    import gpismap_amd
    L = C.CDLL(gpismap_amd.LIB_PATH)                     # loads without a GPU
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpismap_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gpis_timing_[0-9a-z_]*)\s*\(", hdr)) == NAMES
    for n in sorted(NAMES):
        assert hasattr(L, n), "missing symbol " + n
    o = gpismap_amd.gpis_traj_timing_opts()
    f = L.gpis_timing_default_opts
    f.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_traj_timing_opts)]
    for dim, step in [(2, 0.25), (3, 0.1)]:
        assert f(dim, step, C.byref(o)) == 0
        want = tr.default_opts(dim, step)
        for k in tr.OPT_NAMES:
            assert F32(getattr(o, k)).view(np.uint32) == F32(want[k]).view(np.uint32), k
    assert tuple(f[0] for f in gpismap_amd.gpis_traj_timing_opts._fields_) == tr.OPT_NAMES
    assert f(2, 0.25, C.byref(o)) == 0 and (o.v_max, o.a_max, o.d_max, o.a_lat, o.w_max, o.clearance, o.slow_dist) == (1.0, 0.5, 0.5, 0.5, 1.0, 0.25, 1.0)
    assert f(2, 0.25, None) == -1 and f(1, 0.25, C.byref(o)) == -1 and f(4, 0.25, C.byref(o)) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert f(3, bad, C.byref(o)) == -1
    # NULL handles never reach a device
    d = C.c_double
    L.gpis_timing_time.argtypes = [C.c_void_p] * 4
    L.gpis_timing_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.gpis_timing_get.argtypes = [C.c_void_p] * 9
    L.gpis_timing_controls.argtypes = [C.c_void_p, d, C.c_int, d, d, d] + [C.c_void_p] * 4
    L.gpis_timing_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, d, d, d, d, C.c_void_p, C.c_void_p]
    assert L.gpis_timing_time(None, None, C.byref(o), None) == -1 and L.gpis_timing_info(None, None, 0) == -1
    assert L.gpis_timing_get(*[None] * 9) == -1 and L.gpis_timing_controls(None, 0.1, 4, 0.0, 0.0, 0.0, None, None, None, None) == -1
    assert L.gpis_timing_follow(None, None, 0, 0.1, 0.0, 0.0, 0.0, None, None) == -1
    assert gpismap_amd.timing_opts(2, 0.25, v_max=2.0).v_max == 2.0
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.timing_opts(2, 0.25, jerk=1)
    for meth in ("time", "timing", "timing_info", "controls"):
        assert callable(getattr(gpismap_amd.Trajectories, meth)), meth
    assert callable(gpismap_amd.Controller.follow)


def test_the_reference_rejects_bad_options():
    sc = traj_cases.scene(2)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(v_max=0.0), dict(v_max=nan), dict(v_min=0.0), dict(v_min=2.0), dict(a_max=0.0), dict(d_max=-1.0), dict(a_lat=-0.1),
               dict(w_max=-1.0), dict(v_start=-0.1), dict(v_end=inf), dict(clearance=nan), dict(slow_dist=-1.0)):
        with pytest.raises(ValueError):
            tr.check_opts(tc.opts(sc, **kw))
    tr.check_opts(tc.opts(sc, a_lat=0.0, w_max=0.0, slow_dist=0.0, clearance=-1.0, v_min=1.0))
    x = np.zeros((1, 3, 2), F32)
    for a in (dict(dt=0.0), dict(dt=nan), dict(T=0), dict(T=257), dict(t0=-1.0), dict(w_limit=-1.0), dict(min_move=-1.0)):
        kw = dict(dt=0.1, T=4, t0=0.0, w_limit=0.0, min_move=0.0)
        kw.update(a)
        with pytest.raises(ValueError):
            tr.controls(x, np.zeros((1, 3), F32), np.zeros((1, 3), F32), [0], **kw)


# ---- hand-computed -------------------------------------------------------------------------------------------------------------
def test_hand_computed_line_and_status3():
    """(0,0) (1,0) (2,0), a_max = d_max = 0.5, rest to rest: L = (0, 1, 0), both cones reach exactly 1 at the middle, where the tie
    goes to v_max: v = (0, 1, 0), dt = 2 / 1, t = (0, 2, 4).  Then the position at tau: s = 0.25 tau^2 up to t = 2."""
    x = np.array([[[0, 0], [1, 0], [2, 0]]], F32)
    o = dict(tr.default_opts(2, 0.25), a_lat=F32(0), w_max=F32(0))
    r = tr.time(x, [0], o)
    assert r["v"].tolist() == [[0.0, 1.0, 0.0]] and r["t"].tolist() == [[0.0, 2.0, 4.0]] and r["limiter"].tolist() == [[5, 0, 5]]
    assert (r["status"][0], r["duration"][0], r["max_speed"][0], r["max_curvature"][0]) == (0, 4.0, 1.0, 0.0)
    assert r["limiter_counts"].tolist() == [[1, 0, 0, 0, 0, 2, 0, 0]]
    c = tr.controls(x, r["v"], r["t"], r["status"], 1.0, 5)
    assert c["p"][0, :, 0].tolist() == [0.0, 0.25, 1.0, 1.75, 2.0, 2.0] and not c["p"][0, :, 1].any()
    assert c["U"][0].tolist() == [[0.25, 0.0], [0.75, 0.0], [0.75, 0.0], [0.25, 0.0], [0.0, 0.0]]
    assert c["heading0"].tolist() == [[1.0, 0.0]] and c["p0"].tolist() == [[0.0, 0.0]] and c["clamped"][0] == 0
    # a right angle: Menger's curvature of (0,0) (1,0) (1,1) is 2 * 1 / (1 * 1 * sqrt(2))
    k = tr.curvature(np.array([[[0, 0], [1, 0], [1, 1]]], F32), np.ones((1, 2), F32))
    assert k[0, 0] == 0 and k[0, 2] == 0 and k[0, 1] == F32(2) / np.sqrt(F32(2))
    k3 = tr.curvature(np.array([[[0, 0, 1], [1, 0, 1], [1, 0, 2]]], F32), np.ones((1, 2), F32))
    assert k3[0, 1] == k[0, 1]
    x3, kw = tc.status3()
    r = tr.time(x3, [0], dict(tr.default_opts(2, 0.25), **{k: F32(v) for k, v in kw.items()}))
    assert r["status"][0] == 3 and r["t"][0, 0] == 0 and r["t"][0, 1] == 0 and np.isinf(r["t"][0, 2]) and r["limiter"][0, 1] == 6
    c = tr.controls(x3, r["v"], r["t"], r["status"], 0.5, 3)
    assert not c["U"].any() and c["heading0"].tolist() == [[1.0, 0.0]] and c["p0"].tolist() == [[0.5, 2.0]]


# ---- what the shared cases reach -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_cases_reach_every_code_status_and_branch(dim):
    sc, dist, field = _scene(dim)
    codes, stats, trace = set(), set(), {}
    for N in (3, 4, 64):
        x = tc.curves(sc, N)
        for kw in tc.OPT_SETS:
            r = tr.time(x, _status(x), tc.opts(sc, **kw), field)
            codes |= set(int(c) for c in np.unique(r["limiter"][r["status"] != 2]))
            stats |= set(int(s) for s in r["status"])
            assert np.array_equal(r["limiter_counts"].sum(axis=1), np.where(r["status"] == 2, 0, N))
        r = tr.time(x, _status(x), tc.opts(sc), field)
        for wl, mm in ((0.0, 1e-9), (0.5, 0.05)):      # (from rest the first step is shorter than 0.05: it does not count as moving)
            c = tr.controls(x, r["v"], r["t"], r["status"], 0.25, 64, 0.0, wl, mm, trace=trace)
            assert np.isfinite(c["U"]).all() and np.isfinite(c["heading0"]).all()
            k = tc.NAMES.index("reversal")
            assert c["clamped"][k] >= 1 and (wl == 0.0 or c["clamped"].sum() > c["clamped"][k])
            assert np.abs(c["U"][..., -1]).max() <= (wl if wl > 0 else np.inf)
        still = tc.NAMES.index("point")
        assert r["duration"][still] == 0 and not c["U"][still].any() and c["heading0"][still].tolist() == [1.0, 0.0]
    assert codes == set(range(8)) and stats == {0, 2, 3}
    assert trace["past"] > 0 and trace["reversal"] > 0 and trace["still"] > 0 and trace["before_first"] > 0
    assert dim == 2 or trace["vertical"] > 0


# ---- the limits hold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_profile_keeps_its_limits(dim):
    """u_i <= L_i exactly (L_i is a member of the minimum).  Slopes: u_{i+1} is at most the cone of the j that attains u_i taken
    one segment further; the two cone values differ by the roundings of S_{i+1} = S_i + ds_i, of the difference, the product and
    the sum on each side, each at most half an ulp of the largest value involved, which is at most max(u_i, u_{i+1}, 2 a S_{i+1}):
    8 ulp of that operand."""
    sc, dist, field = _scene(dim)
    worst = 0.0
    for N in (4, 64, 256):
        x = tc.curves(sc, N)
        for kw in tc.OPT_SETS:
            o = tc.opts(sc, **kw)
            parts = {}
            r = tr.time(x, _status(x), o, field, parts=parts)
            u, L, ds, S = (parts[k].astype(F64) for k in ("u", "L", "ds", "S"))
            assert np.all(u <= L)
            assert np.all(parts["L"][:, 1:-1] >= o["v_min"] * o["v_min"]) and np.all(parts["L"] <= o["v_max"] * o["v_max"])
            for lim, sign in ((F32(2) * o["a_max"], 1.0), (F32(2) * o["d_max"], -1.0)):
                rise = sign * (u[:, 1:] - u[:, :-1]) - float(lim) * ds
                big = np.maximum(np.maximum(u[:, 1:], u[:, :-1]), float(lim) * S[:, 1:]).astype(F32)
                tol = 8.0 * np.spacing(big).astype(F64)
                assert np.all(rise <= tol), (N, kw, float((rise - tol).max()))
                worst = max(worst, float((rise / np.spacing(big)).max()))
    print("largest slope excess: %.2f ulp of the larger operand (8 allowed)" % worst)


# ---- defective variants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", tr.VARIANTS)
def test_variants_differ_on_the_gpu_cases(variant):
    """Every defective variant changes bits on the inputs tests/test_gpu_timing.py uses, so a device that equals the reference
    there implements none of them."""
    differs = 0
    for dim in (2, 3):
        sc, dist, field = _scene(dim)
        for N in (64, 65, 256):
            x = tc.curves(sc, N)
            o = tc.opts(sc)
            ref = tr.time(x, _status(x), o, field)
            if variant in ("sweeps", "npsum"):
                differs += not _same(tr.time(x, _status(x), o, field, variant=variant), ref, ("v", "t"))
                continue
            # tau_k on a knot: dt from the reference's own times (the GPU test takes the device's, which are the same bits)
            hit = False
            for dt in tc.knot_dts(ref["t"], ref["status"]):
                a = tr.controls(x, ref["v"], ref["t"], ref["status"], dt, 64, 0.0, 0.0, 1e-9)
                b = tr.controls(x, ref["v"], ref["t"], ref["status"], dt, 64, 0.0, 0.0, 1e-9, variant=variant)
                hit = hit or not _same(a, b, CKEYS)
            differs += hit
    assert differs == 6, (variant, differs)


# ---- closure with the controller's model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_controls_drive_the_model_through_the_timed_positions(dim):
    """Planner paths -> traj_ref.optimize -> time -> controls (no clamp engaged), then mppi_ref's model from (p_0, heading0) with
    zero noise visits p_k.  Allowed: 64 T 2^-53 max(1, max |coordinate|), accumulated double rounding over T steps."""
    sc, dist, field = _scene(dim)
    _, _, _, off, pts, _, st = traj_cases.plan(sc, dist)
    x, ist = traj_ref.resample(off, pts, st, 64)
    opt = traj_ref.optimize(dist, sc["shape"], sc["origin"], sc["step"], x, ist)
    tm = tr.time(opt["x"], opt["status"], tc.opts(sc), field)
    ok = np.flatnonzero((tm["status"] == 0) & (tm["duration"] > 0))
    assert ok.size >= 30 and np.all(tm["status"][opt["status"] == 2] == 2)
    dt, T = (0.2 if dim == 2 else 0.1), 140              # a horizon of 28 s / 14 s: some trajectories end inside it, some do not
    assert (tm["duration"][ok] < dt * T).any() and (tm["duration"][ok] > dt * T).any()
    c = tr.controls(opt["x"], tm["v"], tm["t"], tm["status"], dt, T, 0.0, 0.0, 0.0)
    assert not c["clamped"].any()
    nu = mppi_ref.ncontrols(dim)
    mo = dict(dt=dt, gamma=0.0, sigma=(0.0,) * 4, umin=(-np.inf,) * 4, umax=(np.inf,) * 4, clearance=0.0, margin=0.0, w_obs=0.0,
              w_col=0.0, w_off=0.0, w_goal=0.0)
    bound = 64 * T * 2.0 ** -53 * max(1.0, float(np.abs(opt["x"][ok]).max()))
    worst = 0.0
    for r in ok:
        start = np.concatenate([c["p0"][r], c["heading0"][r]])
        ro = mppi_ref.rollouts(dist, sc["shape"], sc["origin"], sc["step"], start, c["U"][r], np.zeros((1, T, nu)), mo,
                               goal=np.zeros(dim), states=True)
        err = np.sqrt(((ro["states"][0, :, :dim] - c["p"][r]) ** 2).sum(axis=1)).max()
        worst = max(worst, float(err))
    length = opt["length"][ok].astype(F64)
    share = tm["limiter_counts"][ok].sum(axis=0) / float(tm["limiter_counts"][ok].sum())
    print("dim %d: %d trajectories, closure error %.3g (allowed %.3g); duration / (length / v_max) median %.2f, range %.2f .. %.2f; "
          "limiter shares %s; max speed %.2f" % (dim, ok.size, worst, bound, np.median(tm["duration"][ok] / length),
                                                (tm["duration"][ok] / length).min(), (tm["duration"][ok] / length).max(),
                                                " ".join("%s %.0f%%" % (n, 100 * s) for n, s in zip(tr.CODES, share)),
                                                tm["max_speed"][ok].max()))
    assert worst <= bound, (worst, bound)
