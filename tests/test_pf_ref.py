"""The particle-filter reference (tests/pf_ref.py) on the CPU: the C-ABI's new symbols and defaults, the generator's known
answers and statistics, the invariants of the motion update and of the resampling, the defective variants of the contract the
reference must tell apart on the GPU cases' inputs, and the behaviour of the whole filter on the analytic scenes: global
localisation from a pose grid in 2-D while the sensor moves, a static camera in 3-D."""
import ctypes as C
import math
import os
import re

import numpy as np

import locate_ref
import pf_ref
import track_ref
from test_locate_ref import MAXR2, TH2, TRUE2, TRUE3, _lat, depth3, grid2, grid3, ranges2
from test_track_field_ref import LAT2, LAT3, field2, field3
from test_track_ref import CAM, OFF2, pose6, pose_error3, scan, scene2

F32 = np.float32
F64 = np.float64
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_pf_default_opts", "gpis_pf_create", "gpis_pf_destroy", "gpis_pf_init", "gpis_pf_predict", "gpis2_pf_update_scan",
         "gpis3_pf_update_depth", "gpis_pf_resample", "gpis_pf_estimate", "gpis_pf_get", "gpis_pf_device", "gpis_pf_info"}

# ---- the inputs shared with tests/test_gpu_pf.py ----------------------------------------------------------------------------
MOTION2 = (0.10, 0.0, 0.06)            # per step: 0.10 m forward, 0.06 rad
STEPS2 = 7
SEED_R0 = 74744                        # with this seed the resampling offset of tick 1 is 0 mod 65535 (asserted below)
M_R0 = 65537                           # one dominant particle of 65537: qs = 65535, rem = 1
IDENT2 = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 1.0])
IDENT3 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
_CACHE = {}


def motion2(dx, dy, dth):
    c, s = math.cos(dth), math.sin(dth)
    return np.array([dx, dy, c, s, -s, c], F64)


def motion3(d, axis, ang):
    from test_track_ref import rot
    return np.concatenate([np.asarray(d, F64), rot(axis, ang).T.ravel()])


def path2():
    """The sensor's true poses (x, y, theta) of the 2-D scenario: TRUE2, then STEPS2 steps of MOTION2 in its own frame."""
    x, y, th = 0.3, -0.2, 0.15
    out = [(x, y, th)]
    for _ in range(STEPS2):
        x, y, th = x + MOTION2[0] * math.cos(th), y + MOTION2[0] * math.sin(th), th + MOTION2[2]
        out.append((x, y, th))
    return out


def scans2():
    """The scans of the scenario, one per pose of path2()."""
    if "scans2" not in _CACHE:
        _CACHE["scans2"] = [scan(scene2, TH2, pose6(th, (x, y))) for x, y, th in path2()]
    return _CACHE["scans2"]


def err2(est, truth):
    """(metres, degrees) between an estimated pose [x, y, c, s, ...] and (x, y, theta)."""
    d = math.atan2(float(est[3]), float(est[2])) - truth[2]
    d = (d + math.pi) % (2 * math.pi) - math.pi
    return math.hypot(float(est[0]) - truth[0], float(est[1]) - truth[1]), abs(math.degrees(d))


def _bits(a):
    return np.ascontiguousarray(a, F64).view(U64)


ULP1 = 2.0 ** -52                      # the spacing of doubles at 1


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis[0-9]?_pf[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_pf_default_opts.argtypes = [C.c_int, C.POINTER(gpismap_amd.gpis_pf_opts)]
    for dim in (3, 2):
        o = gpismap_amd.gpis_pf_opts()
        assert L.gpis_pf_default_opts(dim, C.byref(o)) == 0
        got = dict(max_residual=o.max_residual, beta=o.beta, sigma_t=tuple(o.sigma_t), sigma_r=o.sigma_r,
                   resample_below=o.resample_below, stride=o.stride)
        assert got == pf_ref.default_opts(dim)
        p = gpismap_amd.pf_opts(dim, sigma_t=0.25, beta=3.0)
        assert tuple(p.sigma_t) == ((0.25,) * 3 if dim == 3 else (0.25, 0.25, 0.0)) and p.beta == 3.0 and p.stride == o.stride
    assert pf_ref.default_opts(2) == dict(max_residual=0.5, beta=2.0, sigma_t=(0.03, 0.03, 0.0), sigma_r=0.03, resample_below=0.5, stride=1)
    assert pf_ref.default_opts(3) == dict(max_residual=0.05, beta=100.0, sigma_t=(0.003, 0.003, 0.003), sigma_r=0.003,
                                          resample_below=0.5, stride=8)
    # max_residual and stride are the locator's
    for dim in (2, 3):
        assert all(pf_ref.default_opts(dim)[k] == locate_ref.default_opts(dim)[k] for k in ("max_residual", "stride"))
    assert L.gpis_pf_default_opts(4, C.byref(o)) == -1 and L.gpis_pf_default_opts(2, None) == -1
    for cls, meths in ((gpismap_amd.ParticleFilter, ("init", "predict", "update_scan", "update_depth", "resample", "estimate", "get",
                                                     "poses", "device_ptrs", "info", "close")),
                       (gpismap_amd.GPisMap, ("pf_update_scan_field",)), (gpismap_amd.GPisMap3, ("pf_update_depth_field",))):
        for m in meths:
            assert callable(getattr(cls, m, None)), (cls, m)
    assert callable(getattr(gpismap_amd, "pf_opts", None))
    with np.testing.assert_raises(gpismap_amd.GpisError):
        gpismap_amd.pf_opts(2, top_k=1)


# ---- the generator ----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The three known answers of Random123's kat_vectors for philox4x32-10."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        got = tuple(int(v[0]) for v in pf_ref.philox(*ctr, *key))
        assert got == want, (ctr, [hex(v) for v in got])
    # vectorised over the first counter word: the same blocks as one at a time
    w = pf_ref.philox(np.arange(5), 7, 2, 0, 11, 13)
    for i in range(5):
        assert tuple(int(v[i]) for v in w) == tuple(int(v[0]) for v in pf_ref.philox(i, 7, 2, 0, 11, 13))
    assert pf_ref.key(0x123456789abcdef0) == (0x9abcdef0, 0x12345678)


def test_deviate_statistics():
    assert pf_ref.KZ == 1.0 / math.sqrt(8.0 * (65536.0 ** 2 - 1.0) / 3.0) and pf_ref.KZ.hex() == "0x1.3988e1412ed76p-17"
    z = pf_ref.deviates(1, np.arange(10 ** 6), 1, 0)
    mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
    frac = [float(np.mean(np.abs(z) < k)) for k in (1, 2, 3)]
    print("10^6 deviates: mean %.2e, variance %.4f, max |z| %.3f, P(|z| < 1, 2, 3) = %.3f %.3f %.4f" % (mean, var, top, *frac))
    assert abs(mean) < 0.01 and abs(var - 1.0) < 0.01 and top <= 4.9
    assert abs(frac[0] - 0.6827) < 0.01 and abs(frac[1] - 0.9545) < 0.005 and abs(frac[2] - 0.9973) < 0.002
    # the bound: all halves 0 / all 65535
    assert (2 * 0 - 8 * 65535) * pf_ref.KZ > -4.899 and (2 * 8 * 65535 - 8 * 65535) * pf_ref.KZ < 4.899
    # a deviate depends on (seed, slot, tick, k, tag) alone
    a = pf_ref.deviates(5, np.arange(1000), 3, 1)
    assert np.array_equal(a[:257], pf_ref.deviates(5, np.arange(257), 3, 1))
    for other in (pf_ref.deviates(6, np.arange(1000), 3, 1), pf_ref.deviates(5, np.arange(1000), 4, 1),
                  pf_ref.deviates(5, np.arange(1000), 3, 2), pf_ref.deviates(5, np.arange(1000), 3, 1, tag=1)):
        assert np.count_nonzero(other != a) > 990


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_rotation_conversions():
    from test_track_ref import rot
    rng = np.random.default_rng(2)
    hemis = 0
    for k in range(200):
        ax, ang = rng.standard_normal(3), rng.uniform(-math.pi, math.pi)
        R = rot(ax, ang)
        q = np.array(pf_ref.mat_to_quat(R.T.ravel()))
        assert abs(float(q @ q) - 1.0) < 4e-16
        assert np.allclose(pf_ref.quat_to_mat(q[None, :])[0].reshape(3, 3).T, R, atol=1e-14)
        hemis += q[0] < 0
    assert hemis > 10                      # the branches do return quaternions of either hemisphere
    # every branch
    for R in (np.eye(3), rot([1, 0, 0], 3.0), rot([0, 1, 0], 3.0), rot([0, 0, 1], 3.0)):
        q = np.array(pf_ref.mat_to_quat(R.T.ravel()))
        assert np.allclose(pf_ref.quat_to_mat(q[None, :])[0].reshape(3, 3).T, R, atol=1e-14)
    # the float32 pose of the initial 2-D state is the input; 3-D: within float32 rounding of it
    g2, g3 = grid2()[:300], grid3()[:300]
    assert np.array_equal(pf_ref.pose32(pf_ref.init_state(g2, 2), 2).view(np.uint32), g2.view(np.uint32))
    assert np.allclose(pf_ref.pose32(pf_ref.init_state(g3, 3), 3), g3, atol=2e-7)
    with np.testing.assert_raises(ValueError):
        pf_ref.init_state(np.array([[0, 0, np.nan, 0, 0, 1]], F32), 2)


def test_predict_keeps_the_norm_and_zero_noise_identity_motion_keeps_the_bits():
    o2, o3 = pf_ref.default_opts(2), pf_ref.default_opts(3)
    s2 = pf_ref.init_state(grid2(), 2)
    s3 = pf_ref.init_state(grid3(), 3)
    m2 = pf_ref.motion_from_pose(motion2(*MOTION2), 2)
    m3 = pf_ref.motion_from_pose(motion3((0.01, -0.02, 0.03), (1, 2, 3), 0.05), 3)
    a2, a3 = s2, s3
    for tick in (1, 2, 3):
        a2 = pf_ref.predict(a2, 2, 1, tick, m2, o2["sigma_t"], o2["sigma_r"])
        a3 = pf_ref.predict(a3, 3, 1, tick, m3, o3["sigma_t"], o3["sigma_r"])
        n2 = a2[:, 2] * a2[:, 2] + a2[:, 3] * a2[:, 3]
        n3 = a3[:, 3] * a3[:, 3] + a3[:, 4] * a3[:, 4] + a3[:, 5] * a3[:, 5] + a3[:, 6] * a3[:, 6]
        d2, d3 = np.abs(n2 - 1.0).max() / ULP1, np.abs(np.sqrt(n3) - 1.0).max() / ULP1
        print("tick %d: c^2 + s^2 within %.1f ulp of 1, |Q| within %.1f" % (tick, d2, d3))
        assert d2 <= 2 and d3 <= 2
    # the particles spread: the noise is there, and it differs per particle
    assert np.unique(_bits(a2[:, 0] - s2[:, 0])).size > 5000
    # zero noise, identity motion.  The translation never changes.  The heading (quaternion) is divided by n = sqrt(its squared
    # norm); n is 1 when the squared norm is 1 or 1 + 2^-52 (sqrt(1 + 2^-52) = 1 + 2^-53 - ... rounds to 1; sqrt(1 - 2^-53) =
    # 1 - 2^-54 - ... lies below the midpoint and rounds to 1 - 2^-53), so such a particle keeps its bits: about half of the
    # predicted particles are of that kind.  The n of the rest is within the bound above, and they move by at most one ulp per
    # component.
    i2 = pf_ref.predict(a2, 2, 1, 4, pf_ref.motion_from_pose(IDENT2, 2), (0.0, 0.0, 0.0), 0.0)
    i3 = pf_ref.predict(a3, 3, 1, 4, pf_ref.motion_from_pose(IDENT3, 3), (0.0, 0.0, 0.0), 0.0)
    assert np.array_equal(_bits(i2[:, :2]), _bits(a2[:, :2])) and np.array_equal(_bits(i3[:, :3]), _bits(a3[:, :3]))
    fix2, fix3 = (n2 == 1.0) | (n2 == 1.0 + ULP1), (n3 == 1.0) | (n3 == 1.0 + ULP1)
    print("squared norm 1 or 1 + 2^-52: %.2f of the 2-D particles, %.2f of the 3-D" % (fix2.mean(), fix3.mean()))
    assert fix2.mean() > 0.3 and fix3.mean() > 0.3
    assert np.array_equal(_bits(i2[fix2]), _bits(a2[fix2])) and np.array_equal(_bits(i3[fix3]), _bits(a3[fix3]))
    assert np.abs(i2 - a2).max() <= 2.0 ** -52 and np.abs(i3 - a3).max() <= 2.0 ** -52
    # an exactly normalised heading from init (theta = 0: c = 1, s = 0) keeps its bits too
    z = s2[:143]
    assert np.all(z[:, 2] == 1.0) and np.all(z[:, 3] == 0.0)
    assert np.array_equal(_bits(pf_ref.predict(z, 2, 1, 1, pf_ref.motion_from_pose(IDENT2, 2), (0.0, 0.0, 0.0), 0.0)), _bits(z))


# ---- resampling ---------------------------------------------------------------------------------------------------------------
def test_resampling_invariants():
    rng = np.random.default_rng(4)
    for m in (1, 2, 257, 1 << 16):
        # equal weights: the identity
        q = np.full(m, 1 << 32, U64)
        assert np.array_equal(pf_ref.ancestors(q, 3, 1), np.arange(m))
        # one dominant particle: every ancestor is that particle
        k = m // 3
        q = np.zeros(m, U64)
        q[k] = 1 << 32
        assert np.all(pf_ref.ancestors(q, 3, 1) == k)
        # random weights (the best at 2^32, many zeros): positions below T, ancestors in range, non-decreasing, and a
        # particle's count of children within one of its share m q / T
        for seed in (1, 2, 3):
            w = np.exp(-rng.exponential(8.0, m))
            w[rng.integers(m)] = 1.0
            q = np.floor(w * pf_ref.TWO32).astype(U64)
            p, Cs, T = pf_ref.positions(q, seed, 5)
            assert int(p[-1]) < T == int(Cs[-1]) and np.all(np.diff(p.astype(np.int64)) >= 0)
            a = pf_ref.ancestors(q, seed, 5)
            assert a.min() >= 0 and a.max() <= m - 1 and np.all(np.diff(a) >= 0)
            assert np.all(q[a] > 0)
            share = q.astype(F64) * m / float(T)
            assert np.abs(np.bincount(a, minlength=m) - share).max() < 1.0 + 1e-6
    # the offset differs with the tick and the seed
    q = np.floor(np.exp(-rng.exponential(2.0, 1000)) * pf_ref.TWO32).astype(U64)
    q[0] = 1 << 32
    p = [pf_ref.positions(q, s, t)[0][0] for s, t in ((1, 1), (1, 2), (2, 1))]
    assert len(set(int(v) for v in p)) == 3


def dominant_q():
    """One dominant particle of M_R0: T = 2^32, qs = 65535, rem = 1; with SEED_R0 the offset of tick 1 is 0, so p_0 = 0 equals
    the prefix sums of every particle before the dominant one."""
    q = np.zeros(M_R0, U64)
    q[40000] = 1 << 32
    return q


def test_a_position_equal_to_a_prefix_sum():
    q = dominant_q()
    p, Cs, T = pf_ref.positions(q, SEED_R0, 1)
    assert divmod(T, M_R0) == (65535, 1) and int(p[0]) == 0 == int(Cs[0])
    assert np.all(pf_ref.ancestors(q, SEED_R0, 1) == 40000)                # the first C_i > 0, not the first C_i >= 0
    assert pf_ref.ancestors(q, SEED_R0, 1, variant="left")[0] == 0


# ---- the defective variants ---------------------------------------------------------------------------------------------------
def update_inputs2(m=1000):
    """(state, cost) of the GPU cases' 2-D set after their first predict: grid2()[:m], seed 1, the scenario's motion."""
    key = ("upd2", m)
    if key not in _CACHE:
        o = pf_ref.default_opts(2)
        shape, origin, step = _lat(LAT2)
        st = pf_ref.predict(pf_ref.init_state(grid2()[:m], 2), 2, 1, 1, pf_ref.motion_from_pose(motion2(*MOTION2), 2), o["sigma_t"], o["sigma_r"])
        loc, _ = track_ref.points2(TH2, ranges2(), OFF2)
        cost = locate_ref.score(field2(), shape, origin, step, loc, pf_ref.pose32(st, 2), MAXR2)[0]
        _CACHE[key] = (st, cost)
    return _CACHE[key]


def test_reference_rejects_the_defective_variants():
    """On the GPU cases' inputs every variant changes at least one bit or one index (asserted, not assumed)."""
    o2, o3 = pf_ref.default_opts(2), pf_ref.default_opts(3)
    s2, s3 = pf_ref.init_state(grid2()[:1000], 2), pf_ref.init_state(grid3(), 3)
    m2 = pf_ref.motion_from_pose(motion2(*MOTION2), 2)
    m3 = pf_ref.motion_from_pose(motion3((0.01, -0.02, 0.03), (1, 2, 3), 0.05), 3)
    good2 = pf_ref.predict(s2, 2, 1, 1, m2, o2["sigma_t"], o2["sigma_r"])
    good3 = pf_ref.predict(s3, 3, 1, 1, m3, o3["sigma_t"], o3["sigma_r"])
    for v in ("world_noise", "float32", "no_renorm"):
        bad2 = pf_ref.predict(s2, 2, 1, 1, m2, o2["sigma_t"], o2["sigma_r"], variant=v)
        bad3 = pf_ref.predict(s3, 3, 1, 1, m3, o3["sigma_t"], o3["sigma_r"], variant=v)
        n2 = int(np.count_nonzero(np.any(_bits(bad2) != _bits(good2), axis=1)))
        n3 = int(np.count_nonzero(np.any(_bits(bad3) != _bits(good3), axis=1)))
        print("variant %s: %d of %d 2-D states and %d of %d 3-D states differ" % (v, n2, len(s2), n3, len(s3)))
        assert n2 > 0 and n3 > 0, v
    st, cost = update_inputs2()
    # a mild beta keeps many weights between 0 and 2^32, where floor and round part
    L = pf_ref.accumulate(np.zeros(len(cost)), cost, 0.05)
    q = pf_ref.weights(L)
    nr = int(np.count_nonzero(pf_ref.weights(L, variant="round") != q))
    print("variant round: %d of %d weights differ" % (nr, q.size))
    assert nr > 0 and np.abs(pf_ref.weights(L, variant="round").astype(np.int64) - q.astype(np.int64)).max() == 1
    e, eb = pf_ref.estimate(q, st, 2), pf_ref.estimate(q, st, 2, variant="np_sum")
    print("variant np_sum (2-D): %d of 4 estimate components differ" % np.count_nonzero(_bits(e) != _bits(eb)))
    assert np.any(_bits(e) != _bits(eb))
    q3 = pf_ref.weights(np.random.default_rng(8).uniform(0.0, 3.0, len(good3)))
    assert np.any(_bits(pf_ref.estimate(q3, good3, 3)) != _bits(pf_ref.estimate(q3, good3, 3, variant="np_sum")))
    # side='left' parts from the contract only where a position equals a prefix sum: the dominant-particle input of the GPU case
    qd = dominant_q()
    assert np.any(pf_ref.ancestors(qd, SEED_R0, 1, variant="left") != pf_ref.ancestors(qd, SEED_R0, 1))


def test_estimate_by_hand():
    """Three particles: the weighted mean in the tree's order, the sign alignment towards the best particle's quaternion, the
    lowest index on a tie."""
    q = np.array([1 << 31, 1 << 32, 1 << 32], U64)
    st = np.array([[1.0, 2.0, 1.0, 0.0], [3.0, 1.0, 0.0, 1.0], [5.0, 0.0, 0.6, 0.8]])
    e = pf_ref.estimate(q, st, 2)
    T = float((1 << 31) + 2 * (1 << 32))
    sx = ((2.0 ** 31 * 1.0 + 2.0 ** 32 * 3.0) + 2.0 ** 32 * 5.0) / T          # (256-point segment: pairs (i, i + 128) first; three points
    assert e[0] == sx                                                         #  reach slot 0 in index order through the zeros)
    assert abs(e[2] * e[2] + e[3] * e[3] - 1.0) < 4e-16
    assert pf_ref.totals(q) == (int(T), (1 << 15) + 2 * (1 << 16), (1 << 30) + 2 * (1 << 32))
    assert pf_ref.neff(*pf_ref.totals(q)[1:]) == float((1 << 15) + 2 * (1 << 16)) ** 2 / float((1 << 30) + 2 * (1 << 32))
    assert pf_ref.best_index(q) == 1
    Q = np.array([0.5, 0.5, 0.5, 0.5])
    s3 = np.concatenate([np.zeros((3, 3)), np.stack([-Q, Q, -Q])], axis=1)
    e3 = pf_ref.estimate(q, s3, 3)
    assert np.array_equal(e3[3:], Q)                                          # aligned to particle 1: all three agree
    s3b = np.concatenate([np.zeros((3, 3)), np.stack([-Q, -Q, Q])], axis=1)
    assert np.array_equal(pf_ref.estimate(q, s3b, 3)[3:], -Q)                 # the tie between 1 and 2: index 1 decides the sign
    assert np.array_equal(pf_ref.pose64(np.array([1.0, 2.0, 0.6, 0.8]), 2), np.array([1.0, 2.0, 0.6, 0.8, -0.8, 0.6]))


# ---- behaviour ----------------------------------------------------------------------------------------------------------------
def test_global_localisation_2d():
    """5148 particles on a 0.25 m / 10 degree grid that does not hold the true pose; the sensor moves 0.10 m and 0.06 rad per
    step.  The first update collapses the set onto the best grid pose (N_eff about 1); the noise of the motion update and the
    resampling recover: after the last update the estimate is within one lattice step and half a degree."""
    o = pf_ref.default_opts(2)
    shape, origin, step = _lat(LAT2)
    f = pf_ref.Filter(grid2(), 2, seed=1)
    assert f.m == 5148
    mo = motion2(*MOTION2)
    hist = []
    for k, (truth, rg) in enumerate(zip(path2(), scans2())):
        if k:
            f.predict(mo, o["sigma_t"], o["sigma_r"])
        loc, _ = track_ref.points2(TH2, rg, OFF2)
        e = f.update(field2(), shape, origin, step, loc, o["max_residual"], o["beta"], o["resample_below"])
        hist.append((f.neff, f.resampled) + err2(pf_ref.pose64(e, 2), truth))
        print("update %d: N_eff %.1f, resampled %d, error %.4f m %.3f deg" % ((k,) + hist[-1]))
    assert len(hist) == STEPS2 + 1
    assert hist[0][0] < 2.0 and hist[0][1]                     # the collapse
    assert all(h[0] > 500.0 for h in hist[2:])                 # the recovery
    assert hist[-1][2] <= LAT2["step"] and hist[-1][3] <= 0.5
    assert f.tick == STEPS2 + sum(h[1] for h in hist)


def test_static_camera_3d():
    """1029 particles around the true pose, a static camera, stride 2, six updates: the estimate within 5 mm / 0.5 degrees, and
    cheaper than every initial grid pose but the true one.  (No claim about the wall's valley)"""
    o = pf_ref.default_opts(3)
    s3, o3, st3 = _lat(LAT3)
    loc, _ = track_ref.points3(depth3(), CAM, 2)
    g = grid3()
    f = pf_ref.Filter(g, 3, seed=1)
    assert f.m == 1029
    for k in range(6):
        if k:
            f.predict(IDENT3, o["sigma_t"], o["sigma_r"])
        e = f.update(field3(), s3, o3, st3, loc, o["max_residual"], o["beta"], o["resample_below"])
    P = pf_ref.pose64(e, 3)
    et, er = pose_error3(P, TRUE3)
    c0 = locate_ref.score(field3(), s3, o3, st3, loc, g, o["max_residual"])[0]
    ce = locate_ref.score(field3(), s3, o3, st3, loc, P.astype(F32)[None, :], o["max_residual"])[0][0]
    others = np.delete(c0, 171)
    print("3-D: error %.2e m %.3f deg, cost %.2e (true pose %.2e, the best other grid pose %.2e)" % (et, math.degrees(er), ce, c0[171], others.min()))
    assert et <= 0.005 and math.degrees(er) <= 0.5
    assert ce < others.min()
