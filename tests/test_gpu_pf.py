"""The particle filter on the GPU (csrc/pf.hip, gpis_pf_* / gpis2_pf_update_scan / gpis3_pf_update_depth) against the numpy
reference (tests/pf_ref.py), stage by stage: after every call the reference is fed the device's state from before that call.
Everything is compared as bits except the weights q, where the one inexact step (exp, within 1 ulp on either side;
2^32 * 2^-51 < 1) allows a difference of 1; every later stage is computed from the device's own q and compared exactly.  Batch
sizes cover the last workgroup, the segment tree and both levels of the scan; then the point counts, 3-D with the quaternion
sign alignment and ties, reproducibility, the CPU scenario end to end, the map level, the neighbours and the error paths."""
import ctypes as C
import math

import numpy as np
import pytest

import locate_ref
import pf_ref
import track_ref
from test_gpu_locate import _gz, _masked, df2, df3
from test_gpu_track import _bits_equal, _perturb2, _same
from test_gpu_track_field import _lat
from test_locate_ref import MAXR2, TH2, TRUE3, depth3, grid2, grid3, ranges2
from test_pf_ref import IDENT2, IDENT3, M_R0, MOTION2, SEED_R0, STEPS2, err2, motion2, motion3, path2, scans2
from test_track_ref import CAM, OFF2, rot

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U64 = np.uint64
MOTION3 = motion3((0.002, -0.001, 0.003), (1, 2, 3), 0.004)


def _b64(a):
    return np.ascontiguousarray(a, F64).view(U64)


def _b32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    va, vb = (a.view(U64), b.view(U64)) if a.dtype == F64 else (a.view(np.uint32), b.view(np.uint32)) if a.dtype == F32 else (a, b)
    bad = np.flatnonzero((va != vb).reshape(va.shape[0], -1).any(axis=1)) if va.ndim else np.flatnonzero(va != vb)
    assert bad.size == 0, (what, "%d differ, first at %s" % (bad.size, bad[:8]))


class Frame:
    """One frame and its field: the local points for the reference, the arguments for the device."""

    def __init__(self, dim, df, dist, **kw):
        self.dim, self.df, self.dist = dim, df, dist
        self.shape, self.origin, self.step = _lat(df)
        self.kw = kw
        if dim == 2:
            self.loc, _ = track_ref.points2(kw["thetas"], kw["ranges"], kw["off2"])
        else:
            self.loc, _ = track_ref.points3(kw["depth"], kw["cam6"], kw["stride"])

    def update(self, pf, **opts):
        if self.dim == 2:
            return pf.update_scan(self.df, self.kw["thetas"], self.kw["ranges"], self.kw["off2"], **opts)
        return pf.update_depth(self.df, self.kw["depth"], self.kw["cam6"], stride=self.kw["stride"], **opts)

    def score(self, poses, max_residual):
        if self.dim == 2:
            return self.df.score_scan(self.kw["thetas"], self.kw["ranges"], poses, self.kw["off2"], max_residual=max_residual, top_k=1)
        return self.df.score_depth(self.kw["depth"], poses, self.kw["cam6"], stride=self.kw["stride"], max_residual=max_residual, top_k=1)


class Checked:
    """A ParticleFilter (a new one, or `pf`: one that has served other calls and is initialised again here) whose every call is
    checked against the reference fed with the device's state from before the call."""

    def __init__(self, poses, seed, dim, pf=None):
        import gpismap_amd
        self.pf = pf if pf is not None else gpismap_amd.ParticleFilter()
        self.dim, self.seed, self.tick = dim, seed, 0
        self.opts = pf_ref.default_opts(dim)
        self.pf.init(poses, seed=seed)
        g = self.pf.get()
        ref = pf_ref.init_state(poses, dim)
        self.m = ref.shape[0]
        _same_bits(g["state"], ref, "init state")
        _same_bits(g["poses"], pf_ref.pose32(ref, dim), "init poses")
        assert not g["L"].any() and np.all(g["q"] == U64(1 << 32)) and np.array_equal(g["ancestors"], np.arange(self.m))
        i = self.pf.info()
        assert (i["inited"], i["dim"], i["particles"], i["tick"], i["updates"]) == (1, dim, self.m, 0, 0)
        self.resampled_steps = self.kept_steps = self.q_off = 0

    def predict(self, motion, **kw):
        o = dict(self.opts, **kw)
        before = self.pf.get()
        self.pf.predict(motion, **kw)
        self.tick += 1
        g = self.pf.get()
        ref = pf_ref.predict(before["state"], self.dim, self.seed, self.tick, pf_ref.motion_from_pose(motion, self.dim),
                             o["sigma_t"], o["sigma_r"])
        _same_bits(g["state"], ref, "predict state, tick %d" % self.tick)
        _same_bits(g["poses"], pf_ref.pose32(ref, self.dim), "predict poses, tick %d" % self.tick)
        _same_bits(g["L"], before["L"], "predict leaves L")
        assert self.pf.info()["tick"] == self.tick
        return g

    def update(self, fr, locate_too=True, **kw):
        o = dict(self.opts, **kw)
        m, dim = self.m, self.dim
        before = self.pf.get()
        est = fr.update(self.pf, **kw)
        g = self.pf.get()
        what = "m %d p %d tick %d" % (m, fr.loc.shape[0], self.tick)
        # cost: the scorer's reference, and the scorer itself on the same poses
        rc, rn, _ = locate_ref.score(fr.dist, fr.shape, fr.origin, fr.step, fr.loc, before["poses"], o["max_residual"])
        _same_bits(g["cost"], rc, "cost, " + what)
        assert np.array_equal(g["inliers"], rn), what
        if locate_too:
            sc = fr.score(before["poses"], o["max_residual"])
            _same_bits(sc[0], g["cost"], "cost against score_*, " + what)
            assert np.array_equal(sc[1], g["inliers"]), what
        assert self.pf.info()["points"] == fr.loc.shape[0]
        # weights: the one inexact step
        Lref = pf_ref.accumulate(before["L"], rc, o["beta"])
        qref = pf_ref.weights(Lref)
        q = g["q"]
        dq = np.abs(q.astype(np.int64) - qref.astype(np.int64))
        self.q_off += int(np.count_nonzero(dq))
        assert dq.max() <= 1, "%s: q differs from the reference's at %d of %d particles, by up to %d" % (what, np.count_nonzero(dq), m, dq.max())
        assert q.max() == U64(1 << 32)
        # everything after q: from the device's q, exactly
        T, Th, S2 = pf_ref.totals(q)
        assert (est["T"], est["Th"], est["S2"]) == (T, Th, S2), what
        ne = pf_ref.neff(Th, S2)
        assert _b64(est["neff"]) == _b64(ne), (what, est["neff"], ne)
        e = pf_ref.pose64(pf_ref.estimate(q, before["state"], dim), dim)
        _same_bits(est["pose"], e, "estimate, " + what)
        want = ne < o["resample_below"] * m
        assert est["resampled"] == want and self.pf.info()["resampled"] == int(want), (what, ne)
        if want:
            self.tick += 1
            self.resampled_steps += 1
            a = pf_ref.ancestors(q, self.seed, self.tick)
            assert np.array_equal(g["ancestors"], a), (what, np.flatnonzero(g["ancestors"] != a)[:8])
            _same_bits(g["state"], before["state"][a], "gathered state, " + what)
            _same_bits(g["poses"], before["poses"][a], "gathered poses, " + what)
            assert not g["L"].any(), what
        else:
            self.kept_steps += 1
            _same_bits(g["L"], Lref, "L, " + what)
            _same_bits(g["state"], before["state"], "state kept, " + what)
            _same_bits(g["poses"], before["poses"], "poses kept, " + what)
            assert np.array_equal(g["ancestors"], before["ancestors"]), what
        assert self.pf.info()["tick"] == self.tick
        return est, g

    def resample(self):
        before = self.pf.get()
        self.pf.resample()
        self.tick += 1
        g = self.pf.get()
        a = pf_ref.ancestors(before["q"], self.seed, self.tick)
        assert np.array_equal(g["ancestors"], a)
        _same_bits(g["state"], before["state"][a], "explicit resample, state")
        _same_bits(g["poses"], before["poses"][a], "explicit resample, poses")
        assert not g["L"].any() and np.array_equal(g["q"], before["q"]) and self.pf.info()["tick"] == self.tick
        return g


def frame2(ranges=None, off2=OFF2):
    df, dist = df2()
    return Frame(2, df, dist, thetas=TH2, ranges=ranges2() if ranges is None else ranges, off2=off2)


def frame3(stride):
    df, dist = df3()
    return Frame(3, df, dist, depth=depth3(), cam6=CAM, stride=stride)


# ---- stage by stage, 2-D ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097))
def test_stages_2d_every_batch_size(m):
    """Three steps: the first update collapses the set and resamples (m > 1); the second predicts the duplicates apart and keeps
    them (resample_below 0: L accumulates from the resampling's zero and is compared as bits); the third accumulates again."""
    fr = frame2()
    c = Checked(grid2()[:m], 1, 2)
    mo = motion2(*MOTION2)
    for k, kw in enumerate((dict(), dict(resample_below=0.0), dict())):
        c.predict(mo)
        est, g = c.update(fr, **kw)
        if k == 0 and m > 2:        # (m = 2: N_eff >= 1 = resample_below * m, never below)
            assert est["resampled"] and np.unique(g["ancestors"]).size < m
        if k == 1:
            assert not est["resampled"]
            if m > 2:           # the duplicates of the first resampling have been moved apart by their own noise
                assert np.unique(_b64(g["state"]), axis=0).shape[0] == m
    assert c.kept_steps >= 1 and (m <= 2 or c.resampled_steps >= 1)
    print("m %d: q off by one at %d particle-updates of %d" % (m, c.q_off, 3 * m))


def test_stages_2d_two_scan_levels_and_a_position_on_a_prefix_sum():
    """65 537 particles: 257 blocks, so the scan of the block sums has two blocks; 37 beams keep the reference at 2.4 M samples
    per update.  The first update runs with a beta that leaves one dominant particle (T = 2^32, qs = 65535, rem = 1) and a seed
    whose resampling offset is 0: p_0 = 0 equals the prefix sums of every particle before the dominant one, and the ancestor
    is the first C_i > p, not the first C_i >= p."""
    poses = locate_ref.pose_grid2(np.linspace(-1, 3, 41), np.linspace(-1.5, 1.5, 41), np.linspace(0, 2 * math.pi, 39, endpoint=False))[:M_R0]
    fr = frame2(_masked(ranges2(), 37))
    assert fr.loc.shape[0] == 37 and poses.shape[0] == M_R0
    c = Checked(poses, SEED_R0, 2)
    est, g = c.update(fr, beta=1e6)
    assert est["T"] == 1 << 32 and est["resampled"] and c.tick == 1
    p, Cs, _ = pf_ref.positions(g["q"], SEED_R0, 1)
    assert int(p[0]) == 0 == int(Cs[0]) and np.all(g["ancestors"] == int(np.argmax(g["q"]))) and g["ancestors"][0] > 0
    c.predict(motion2(*MOTION2))
    est, g = c.update(fr, locate_too=False)
    if not est["resampled"]:
        g = c.resample()
    assert np.unique(g["ancestors"]).size > 100      # a spread set: the prefix sums cross both levels of the scan


def test_L_accumulates_without_resampling():
    fr = frame2()
    c = Checked(grid2()[:257], 3, 2)
    for k in range(3):
        c.predict(motion2(*MOTION2))
        est, g = c.update(fr, locate_too=False, resample_below=0.0, beta=0.01)
        assert not est["resampled"]
    assert c.kept_steps == 3 and np.all(g["L"] > 0)


# ---- point counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (0, 1, 63, 64, 65, 360))
def test_point_counts_2d(p):
    fr = frame2(_masked(ranges2(), p))
    assert fr.loc.shape[0] == p
    c = Checked(grid2()[:257], 1, 2)
    c.predict(motion2(*MOTION2))
    est, g = c.update(fr)
    if p == 0:                  # no point: the weights stay as they were
        assert not g["cost"].any() and not g["L"].any() and np.all(g["q"] == U64(1 << 32)) and est["neff"] == 257.0 and not est["resampled"]
    c.predict(motion2(*MOTION2))
    c.update(fr, locate_too=False)


def test_off_lattice_uniform_weights_and_the_identity_gather():
    fr = frame2()
    poses = grid2()[:257].copy()
    poses[:, :2] += F32(100.0)
    c = Checked(poses, 1, 2)
    est, g = c.update(fr)
    assert np.all(g["cost"] == 360 * MAXR2 * MAXR2) and not g["inliers"].any()
    assert np.all(g["q"] == U64(1 << 32)) and est["neff"] == 257.0 and est["T"] == 257 << 32 and not est["resampled"]
    before = g
    g = c.resample()
    assert np.array_equal(g["ancestors"], np.arange(257))
    _same_bits(g["state"], before["state"], "the identity gather")
    # resample_below = 0 never resamples, whatever the weights
    c2 = Checked(grid2()[:257], 1, 2)
    est, g = c2.update(fr, resample_below=0.0)
    assert est["neff"] < 2.0 and not est["resampled"] and c2.tick == 0


# ---- 3-D ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", (2, 8))
@pytest.mark.parametrize("m", (1, 64, 257, 1029))
def test_stages_3d(m, stride):
    fr = frame3(stride)
    sel = np.arange(1029) if m == 1029 else (171 + 37 * np.arange(m)) % 1029
    c = Checked(grid3()[sel], 1, 3)
    for k, kw in enumerate((dict(), dict(resample_below=0.0), dict())):
        c.predict(MOTION3 if k else IDENT3)
        c.update(fr, **kw)
    assert c.kept_steps >= 1 and (m == 1 or c.resampled_steps >= 1)


def hemisphere_poses(n=64, far=False):
    """Poses around a rotation of about 120 degrees about (-1, 0.1, 0.05): alternately 118 degrees (trace > 0: w > 0) and 122
    degrees (the largest-diagonal branch: x > 0, so w < 0): neighbouring rotations whose quaternions lie in opposite hemispheres."""
    rng = np.random.default_rng(6)
    R0 = TRUE3[3:].astype(F64).reshape(3, 3).T
    out = []
    for k in range(n):
        R = rot(rng.standard_normal(3), 0.01) @ rot([-1, 0.1, 0.05], math.radians(118.0 if k % 2 == 0 else 122.0)) @ R0
        t = TRUE3[:3].astype(F64) + rng.uniform(-0.02, 0.02, 3) + (100.0 if far else 0.0)
        out.append(np.concatenate([t, R.T.ravel()]))
    return np.array(out, F32)


def test_quaternion_sign_alignment_3d():
    poses = hemisphere_poses()
    Q = pf_ref.init_state(poses, 3)[:, 3:]
    assert np.all(Q[0::2, 0] > 0) and np.all(Q[1::2, 0] < 0) and np.all(Q[0::2] @ Q[1] < -0.9)
    fr = frame3(8)
    c = Checked(poses, 1, 3)
    for k in range(2):
        est, g = c.update(fr, beta=10.0)
        assert est["neff"] > 8.0                   # many particles carry weight: without the alignment the sum would cancel
        R = est["pose"][3:].reshape(3, 3).T
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-12)
        best = poses[int(np.argmax(g["q"]))] if k == 0 else None
        if best is not None:                       # the mean rotation is near every particle's: within 5 degrees of the best's
            Rb = best[3:].astype(F64).reshape(3, 3).T
            assert math.degrees(math.acos(min(1.0, (np.trace(Rb.T @ R) - 1.0) / 2.0))) < 5.0
        c.predict(IDENT3)


def test_tie_for_the_best_particle_3d():
    """Every point off the lattice: every q is 2^32, and the lowest index decides the hemisphere.  Swapping the first two
    particles (opposite hemispheres) leaves the estimated rotation where it was; the reference's argmax states the rule."""
    fr = frame3(8)
    poses = hemisphere_poses(far=True)
    c = Checked(poses, 1, 3)
    est, g = c.update(fr)
    assert np.all(g["q"] == U64(1 << 32)) and pf_ref.best_index(g["q"]) == 0 and not est["resampled"]
    swapped = poses.copy()
    swapped[[0, 1]] = poses[[1, 0]]
    c2 = Checked(swapped, 1, 3)
    est2, _ = c2.update(fr)
    assert np.allclose(est2["pose"], est["pose"], atol=1e-9)
    # duplicates of the best pose: the tie goes to the lowest index
    d = grid3()[[3, 171, 9, 171, 171, 40]]
    c3 = Checked(d, 1, 3)
    est3, g3 = c3.update(frame3(2), resample_below=0.0)
    assert g3["q"][1] == g3["q"][3] == g3["q"][4] == U64(1 << 32) and pf_ref.best_index(g3["q"]) == 1


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
def _run(poses, seed, steps, stream=None):
    import gpismap_amd
    df, _ = df2()
    pf = gpismap_amd.ParticleFilter()
    pf.init(poses, seed=seed)
    out = []
    for _ in range(steps):
        pf.predict(MOTION2, stream=stream)         # (the (dx, dy, dtheta) form)
        out.append(pf.get())
        est = pf.update_scan(df, TH2, ranges2(), OFF2, stream=stream)
        out.append(dict(pf.get(), pose=est["pose"], neff=np.float64(est["neff"])))
    return out


def _equal_runs(a, b):
    return all(np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)) for x, y in zip(a, b) for k in x)


def test_same_seed_same_bits_and_the_stream_does_not_matter():
    import torch
    poses = grid2()[:1000]
    a = _run(poses, 7, 2)
    assert _equal_runs(a, _run(poses, 7, 2))
    s = torch.cuda.Stream(device=0)
    assert _equal_runs(a, _run(poses, 7, 2, stream=C.c_void_p(s.cuda_stream)))
    b = _run(poses, 8, 1)
    assert np.count_nonzero(_b64(b[0]["state"]) != _b64(a[0]["state"])) > 3000
    # the (dx, dy, dtheta) form of the motion is the pose form
    import gpismap_amd
    pf = gpismap_amd.ParticleFilter()
    pf.init(poses, seed=7)
    pf.predict(motion2(*MOTION2))
    _same_bits(pf.get()["state"], a[0]["state"], "motion forms")


def test_predict_depends_on_seed_tick_and_slot_alone():
    import gpismap_amd
    out = []
    for m in (257, 1000):
        pf = gpismap_amd.ParticleFilter()
        pf.init(grid2()[:m], seed=5)
        pf.predict(motion2(*MOTION2))
        out.append(pf.get())
    _same_bits(out[0]["state"], out[1]["state"][:257], "the first 257 of 1000")
    _same_bits(out[0]["poses"], out[1]["poses"][:257], "the first 257 of 1000")


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_global_localisation_2d_on_the_device():
    """The CPU scenario of tests/test_pf_ref.py through ParticleFilter, with its acceptance: behaviour, not bits (a q may
    differ by one from the reference's own run)."""
    import gpismap_amd
    df, _ = df2()
    pf = gpismap_amd.ParticleFilter()
    pf.init(grid2(), seed=1)
    hist = []
    for k, (truth, rg) in enumerate(zip(path2(), scans2())):
        if k:
            pf.predict(MOTION2)
        est = pf.update_scan(df, TH2, rg, OFF2)
        hist.append((est["neff"], est["resampled"]) + err2(est["pose"], truth))
        print("update %d: N_eff %.1f, resampled %d, error %.4f m %.3f deg" % ((k,) + hist[-1]))
    assert len(hist) == STEPS2 + 1 and hist[0][0] < 2.0 and hist[0][1]
    assert all(h[0] > 500.0 for h in hist[2:])
    assert hist[-1][2] <= 0.02 and hist[-1][3] <= 0.5
    i = pf.info()
    assert i["updates"] == STEPS2 + 1 and i["tick"] == STEPS2 + i["resamplings"] and i["particles"] == 5148 and i["points"] == 360


def test_device_pointers():
    """The addresses of the set: all there, state and poses change halves with a resampling, the rest stay."""
    import gpismap_amd
    pf = gpismap_amd.ParticleFilter()
    pf.init(grid2()[:300], seed=1)
    p = pf.device_ptrs()
    assert all(p[k] for k in gpismap_amd.ParticleFilter.PTR_KEYS) and len(set(p.values())) == 7
    pf.resample()
    q = pf.device_ptrs()
    assert q["state"] != p["state"] and q["poses"] != p["poses"] and all(q[k] == p[k] for k in ("L", "q", "cost", "inliers", "ancestors"))
    pf.resample()
    assert pf.device_ptrs() == p


# ---- map level ------------------------------------------------------------------------------------------------------------------
def test_map_level_update_matches_score_scan_field():
    import gpismap_amd
    g2, f2, dfg = _gz()
    fr = f2[len(f2) // 2]
    x, y, th = float(fr["pose"][0]), float(fr["pose"][1]), math.atan2(float(fr["pose"][3]), float(fr["pose"][2]))
    d = np.array([-0.3, -0.1, 0.1, 0.3])
    poses = gpismap_amd.pose_grid2(x + d, y + d, th + np.radians([-6.0, -2.0, 2.0, 6.0]))
    pf = gpismap_amd.ParticleFilter()
    pf.init(poses, seed=2)
    pf.predict((0.0, 0.0, 0.0))
    before = pf.poses()
    est = g2.pf_update_scan_field(dfg, pf, fr["thetas"], fr["ranges"])
    g = pf.get()
    sc = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], before, top_k=0)
    _same_bits(g["cost"], sc[0], "gazebo field")
    assert np.array_equal(g["inliers"], sc[1]) and g["inliers"].max() > 20
    assert math.hypot(est["pose"][0] - x, est["pose"][1] - y) < 0.45


# ---- neighbours -----------------------------------------------------------------------------------------------------------------
def test_scorer_and_field_tracker_unchanged_by_a_filter_step():
    import gpismap_amd
    g2, f2, dfg = _gz()
    fr = f2[5]
    start = _perturb2(fr["pose"], 0.05, 1.0)
    t = gpismap_amd.Tracker()
    poses = np.stack([start, fr["pose"], _perturb2(fr["pose"], 0.2, 4.0)])
    track0 = g2.track_scan_field(dfg, fr["thetas"], fr["ranges"], start, tracker=t)
    score0 = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], poses)
    pf = gpismap_amd.ParticleFilter()
    pf.init(np.tile(poses, (100, 1)), seed=1)
    pf.predict((0.01, 0.0, 0.001))
    g2.pf_update_scan_field(dfg, pf, fr["thetas"], fr["ranges"])
    track1 = g2.track_scan_field(dfg, fr["thetas"], fr["ranges"], start, tracker=t)
    score1 = g2.score_scan_field(dfg, fr["thetas"], fr["ranges"], poses)
    assert track0[1]["inliers"] > 20 and _same(track0, track1)
    assert _bits_equal(score0[0], score1[0]) and np.array_equal(score0[1], score1[1]) and np.array_equal(score0[2], score1[2])


# ---- errors ---------------------------------------------------------------------------------------------------------------------
_SCAN = object()


def _upd2(L, pf, df, thetas=TH2, ranges=_SCAN, off2=OFF2, n=None, map_h=None, **kw):
    import gpismap_amd
    P = lambda a: None if a is None else np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    o = gpismap_amd.pf_opts(2, **kw)
    ranges = ranges2() if ranges is _SCAN else ranges
    return L.gpis2_pf_update_scan(map_h, df.h if df is not None else None, pf.h if pf is not None else None, P(thetas), P(ranges),
                                  len(TH2) if n is None else n, P(off2), C.byref(o), None)


def test_errors_leave_the_state():
    import gpismap_amd
    L = gpismap_amd.lib()
    df, _ = df2()
    d3, _ = df3()
    nores = gpismap_amd.DistanceField()
    dp = lambda a: np.ascontiguousarray(a, F64).ctypes.data_as(C.POINTER(C.c_double))
    fp = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(C.POINTER(C.c_float))
    pf = gpismap_amd.ParticleFilter()
    # before init
    assert L.gpis_pf_predict(pf.h, dp(IDENT2), None, None) == -3 and _upd2(L, pf, df) == -3 and L.gpis_pf_resample(pf.h, None) == -3
    assert L.gpis_pf_get(pf.h, None, None, None, None, None, None, None) == -3 and L.gpis_pf_estimate(pf.h, None, None, None, None) == -3
    assert L.gpis_pf_device(pf.h, (C.c_void_p * 7)(), 7) == -3 and pf.info()["inited"] == 0
    with pytest.raises(gpismap_amd.GpisError):
        pf.get()
    with pytest.raises(gpismap_amd.GpisError):
        pf.predict((0.0, 0.0, 0.0))
    poses = grid2()[:300]
    bad = poses.copy(); bad[7, 2] = np.nan
    assert L.gpis_pf_init(pf.h, 2, fp(bad), 300, 1) == -1 and L.gpis_pf_init(pf.h, 4, fp(poses), 300, 1) == -1
    assert L.gpis_pf_init(pf.h, 2, fp(poses), 0, 1) == -1 and L.gpis_pf_init(pf.h, 2, None, 300, 1) == -1
    assert L.gpis_pf_init(pf.h, 2, fp(poses), (1 << 24) + 1, 1) == -4 and pf.info()["inited"] == 0
    pf.init(poses, seed=1)
    assert L.gpis_pf_estimate(pf.h, None, None, None, None) == -3          # no update yet
    pf.predict(MOTION2)
    pf.update_scan(df, TH2, ranges2(), OFF2, resample_below=0.0)
    a, ia, ea, pa = pf.get(), pf.info(), pf.estimate(), pf.device_ptrs()

    def still_there(what):
        b, eb = pf.get(), pf.estimate()
        assert pf.info() == ia and pf.device_ptrs() == pa, what
        for k in a:
            _same_bits(b[k], a[k], what + ": " + k)
        _same_bits(eb["pose"], ea["pose"], what)
        assert (eb["neff"], eb["T"], eb["resampled"]) == (ea["neff"], ea["T"], ea["resampled"]), what

    bad_th = TH2.copy(); bad_th[2] = np.nan
    arg = dict(no_field=dict(df=None), no_thetas=dict(thetas=None), no_ranges=dict(ranges=None), no_offset=dict(off2=None), n0=dict(n=0),
               stride0=dict(stride=0), r_neg=dict(max_residual=-1.0), r_nan=dict(max_residual=np.nan), r_inf=dict(max_residual=np.inf),
               beta_neg=dict(beta=-1.0), beta_nan=dict(beta=np.nan), beta_inf=dict(beta=np.inf), st_neg=dict(sigma_t=(-0.1, 0.0)),
               st_nan=dict(sigma_t=(0.0, np.nan)), sr_neg=dict(sigma_r=-0.01), sr_inf=dict(sigma_r=np.inf), rb_nan=dict(resample_below=np.nan),
               theta=dict(thetas=bad_th), off_nan=dict(off2=np.array([np.nan, 0.0], F32)), dim=dict(df=d3))
    for name, kw in arg.items():
        args = dict(df=df)
        args.update(kw)
        assert _upd2(L, pf, args.pop("df"), **args) == -1, name
        still_there(name)
    assert _upd2(L, None, df) == -1
    assert _upd2(L, pf, nores) == -3
    still_there("no result in the field")
    assert _upd2(L, pf, df, n=(1 << 26) + 1) == -4
    still_there("beams")
    # a 3-D update on the 2-D set
    assert L.gpis3_pf_update_depth(None, d3.h, pf.h, C.byref(gpismap_amd._cam(CAM)), fp(depth3()), None, None) == -1
    still_there("a depth image for a 2-D set")
    # predict
    for name, (mo, kw) in dict(no_motion=(None, {}), nan=(np.array([0.0, np.nan, 1.0, 0.0, 0.0, 1.0]), {}), st=(IDENT2, dict(sigma_t=(-1.0, 0.0))),
                               sr=(IDENT2, dict(sigma_r=np.nan))).items():
        o = gpismap_amd.pf_opts(2, **kw)
        assert L.gpis_pf_predict(pf.h, None if mo is None else dp(mo), C.byref(o), None) == -1, name
        still_there("predict " + name)
    with pytest.raises(gpismap_amd.GpisError):
        pf.predict((0.0, 0.0))
    with pytest.raises(gpismap_amd.GpisError):
        pf.update_scan(df, TH2, ranges2()[:-1], OFF2)
    with pytest.raises(gpismap_amd.GpisError):
        pf.update_scan(df, TH2, ranges2(), OFF2, top_k=3)
    still_there("python checks")
    # 3-D: the camera and the field
    p3 = gpismap_amd.ParticleFilter()
    p3.init(grid3()[:64], seed=1)
    p3.update_depth(d3, depth3(), CAM, resample_below=0.0)
    a3, i3 = p3.get(), p3.info()
    cam = lambda c: C.byref(gpismap_amd._cam(c))
    for name, (f, c, dep, kw) in dict(no_cam=(d3, None, depth3(), {}), bad_cam=(d3, (0.0, 50.0, 39.5, 29.5, 80, 60), depth3(), {}),
                                      no_depth=(d3, CAM, None, {}), stride0=(d3, CAM, depth3(), dict(stride=0)),
                                      dim=(df, CAM, depth3(), {}), beta=(d3, CAM, depth3(), dict(beta=-1.0))).items():
        o = gpismap_amd.pf_opts(3, **kw)
        rc = L.gpis3_pf_update_depth(None, f.h, p3.h, None if c is None else cam(c), None if dep is None else fp(dep), C.byref(o), None)
        assert rc == -1, name
        b3 = p3.get()
        assert p3.info() == i3 and all(np.array_equal(np.ascontiguousarray(b3[k]).view(np.uint8), np.ascontiguousarray(a3[k]).view(np.uint8)) for k in a3), name
    assert L.gpis3_pf_update_depth(None, nores.h, p3.h, cam(CAM), fp(depth3()), None, None) == -3
    assert L.gpis3_pf_update_depth(None, d3.h, p3.h, cam((50.0, 50.0, 39.5, 29.5, 8193, 8192)), fp(depth3()), None, None) == -4
    assert p3.info() == i3
    # after the errors the filters work again; init replaces a set, also by one of the other dimension
    pf.predict(MOTION2)
    pf.update_scan(df, TH2, ranges2(), OFF2)
    pf.init(grid3()[:10], seed=2)
    est = pf.update_depth(d3, depth3(), CAM)
    assert pf.info()["dim"] == 3 and est["pose"].shape == (12,)
