"""The tracking reference (tests/track_ref.py) checked against itself on analytic scenes with exact f and gradient: the Jacobian
against finite differences, pose recovery in 3-D and 2-D, the degenerate plane, the evaluate-only call, and the reduction tree
against an exactly rounded sum.  CPU only."""
import math

import numpy as np

import track_ref

F32 = np.float32
CAM = (50.0, 50.0, 39.5, 29.5, 80, 60)
OFF2 = (0.08, 0.0)


# ---- analytic scenes ------------------------------------------------------------------------------------------------------
def scene3(p):
    """A sphere in front of a wavy wall facing the camera: (f, grad) in double; f > 0 in free space."""
    p = np.asarray(p, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    fp = (1.5 + 0.05 * np.sin(4 * x) * np.cos(3 * y)) - z
    gp = np.stack([0.2 * np.cos(4 * x) * np.cos(3 * y), -0.15 * np.sin(4 * x) * np.sin(3 * y), -np.ones_like(x)], axis=1)
    d = p - np.array([0.1, -0.05, 1.1])
    n = np.linalg.norm(d, axis=1)
    fs = n - 0.2
    gs = d / n[:, None]
    s = fs < fp
    return np.where(s, fs, fp), np.where(s[:, None], gs, gp)


def scene2(p):
    """A room with a wavy floor and a round pillar."""
    p = np.asarray(p, np.float64)
    x, y = p[:, 0], p[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    d = p - np.array([2.0, 0.6])
    n = np.linalg.norm(d, axis=1)
    cands = [(n - 0.4, d[:, 0] / n, d[:, 1] / n),
             (y - (-1.5 + 0.1 * np.sin(2 * x)), -0.2 * np.cos(2 * x), one),
             (4.5 - x, -one, zero), (2.5 - y, zero, -one), (x + 3.0, one, zero)]
    f = np.min(np.stack([c[0] for c in cands]), axis=0)
    g = np.zeros((x.size, 2))
    for c in reversed(cands):
        m = c[0] == f
        g[m, 0], g[m, 1] = c[1][m], c[2][m]
    return f, g


def plane3(p):
    p = np.asarray(p, np.float64)
    return 1.5 - p[:, 2], np.tile([0.0, 0.0, -1.0], (p.shape[0], 1))


def analytic_fn(scene, dim):
    def fn(x, res):
        f, g = scene(x)
        res[:, 0] = f
        res[:, 1:1 + dim] = g
        res[:, 1 + dim] = 1e-3
        return res
    return fn


def cast(scene, o, d, lo, hi, step):
    """First crossing of f = 0 along o + s d, s in [lo, hi]: sampled, then bisected in double.  NaN where none."""
    ss = np.arange(lo, hi, step)
    n = d.shape[0]
    prev = scene(o + lo * d)[0]
    a = np.full(n, np.nan)
    for s in ss[1:]:
        cur = scene(o + s * d)[0]
        hit = np.isnan(a) & (prev > 0) & (cur <= 0)
        a[hit] = s - step
        prev = cur
    ok = ~np.isnan(a)
    l, h = a[ok], a[ok] + step
    for _ in range(60):
        mid = 0.5 * (l + h)
        inside = scene(o[ok] + mid[:, None] * d[ok])[0] <= 0
        h = np.where(inside, mid, h)
        l = np.where(inside, l, mid)
    out = np.full(n, np.nan)
    out[ok] = 0.5 * (l + h)
    return out


def pose12(R, t):
    return np.concatenate([t, R.T.ravel()]).astype(F32)       # [t(3), R column-major]


def rot(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def depth_image(scene, cam, P):
    """Depth along the camera z of the scene from pose P (12 floats), update()'s column-major layout."""
    fx, fy, cx, cy, W, H = cam
    k = np.arange(W * H)
    u = ((k // H) - cx) / fx
    v = ((k % H) - cy) / fy
    R = np.asarray(P[3:], np.float64).reshape(3, 3).T
    d = (R @ np.stack([u, v, np.ones_like(u)])).T                 # a unit step in z
    z = cast(scene, np.tile(np.asarray(P[:3], np.float64), (k.size, 1)), d, 0.45, 3.5, 0.004)
    return z.astype(F32)


def scan(scene, thetas, P6):
    R = np.array([[P6[2], P6[4]], [P6[3], P6[5]]], np.float64)
    o = R @ np.array(OFF2) + np.asarray(P6[:2], np.float64)
    d = (R @ np.stack([np.cos(thetas.astype(np.float64)), np.sin(thetas.astype(np.float64))])).T
    return cast(scene, np.tile(o, (thetas.size, 1)), d, 0.25, 12.0, 0.005).astype(F32)


def pose_error3(P, Q):
    Rp = np.asarray(P[3:], np.float64).reshape(3, 3).T
    Rq = np.asarray(Q[3:], np.float64).reshape(3, 3).T
    c = (np.trace(Rp.T @ Rq) - 1) / 2
    return float(np.linalg.norm(np.asarray(P[:3], np.float64) - np.asarray(Q[:3], np.float64))), math.acos(min(1.0, max(-1.0, c)))


def pose6(th, t):
    c, s = math.cos(th), math.sin(th)
    return np.array([t[0], t[1], c, s, -s, c], F32)


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_jacobian_matches_finite_differences():
    rng = np.random.default_rng(3)
    for dim, scene in ((3, scene3), (2, scene2)):
        if dim == 3:
            P = [float(v) for v in pose12(rot([0.3, -1, 0.2], 0.05), np.array([0.02, -0.01, 0.03]))]
            loc = np.stack([rng.uniform(-0.5, 0.5, 200), rng.uniform(-0.4, 0.4, 200), rng.uniform(0.8, 1.6, 200)], 1).astype(F32)
        else:
            P = [float(v) for v in pose6(0.1, (0.2, -0.1))]
            loc = np.stack([rng.uniform(-2, 3, 200), rng.uniform(-1, 1.5, 200)], 1).astype(F32)
        nj = 6 if dim == 3 else 3
        x = track_ref.world(loc, P, dim)
        _, t = track_ref.pass_pose(P, dim)
        _, g = scene(x)
        J = track_ref.jacobian(x, g.astype(F32), t, dim)

        def r_at(xi):
            Q = track_ref.apply(P, list(xi), dim)
            Rq = np.asarray(Q[dim:]).reshape(dim, dim).T
            w = loc.astype(np.float64) @ Rq.T + np.asarray(Q[:dim])
            return scene(w)[0]
        h = 1e-6
        for i in range(nj):
            e = np.zeros(nj)
            e[i] = h
            fd = (r_at(e) - r_at(-e)) / (2 * h)
            assert np.allclose(J[:, i], fd, rtol=1e-4, atol=2e-5), (dim, i, np.abs(J[:, i] - fd).max())


def test_recovers_a_known_pose_3d():
    T_true = pose12(rot([1, 2, -1], math.radians(1.0)), np.array([0.01, -0.015, 0.01]))
    depth = depth_image(scene3, CAM, T_true)
    assert np.count_nonzero(np.isfinite(depth)) > 0.9 * depth.size
    R0 = rot([0.4, -1, 0.7], math.radians(2.0)) @ np.asarray(T_true[3:], np.float64).reshape(3, 3).T
    start = pose12(R0, np.asarray(T_true[:3], np.float64) + np.array([0.012, -0.01, 0.012]))
    o = track_ref.Opts(3, level=0.0, stride=1)
    out = track_ref.track_depth(analytic_fn(scene3, 3), depth, CAM, start, o)
    et, er = pose_error3(out["pose"], T_true)
    e0 = pose_error3(start, T_true)
    print("3-D: start %.4f m %.3f deg -> %.2e m %.2e deg, status %d, %d iterations, %d inliers of %d"
          % (e0[0], math.degrees(e0[1]), et, math.degrees(er), out["status"], out["iterations"], out["inliers"], out["points"]))
    assert out["status"] == 0 and out["iterations"] <= 10
    assert out["passes"] == out["iterations"] + 1
    assert et < 1e-4 and er < math.radians(0.005)
    assert out["cost"] < out["cost0"]


def test_recovers_a_known_pose_2d():
    th = np.linspace(-math.pi, math.pi, 360, endpoint=False).astype(F32)
    T_true = pose6(0.15, (0.3, -0.2))
    ranges = scan(scene2, th, T_true)
    assert np.count_nonzero(np.isfinite(ranges)) == th.size
    start = pose6(0.15 + math.radians(2.0), (0.3 + 0.015, -0.2 - 0.013))
    o = track_ref.Opts(2, level=0.0)
    out = track_ref.track_scan(analytic_fn(scene2, 2), th, ranges, start, OFF2, o)
    P = out["pose"].astype(np.float64)
    et = float(np.hypot(P[0] - T_true[0], P[1] - T_true[1]))
    er = abs(math.atan2(P[3], P[2]) - 0.15)
    print("2-D: status %d, %d iterations, error %.2e m %.2e deg" % (out["status"], out["iterations"], et, math.degrees(er)))
    assert out["status"] == 0 and out["iterations"] <= 10
    assert et < 1e-4 and er < math.radians(0.005)


def test_plane_is_degenerate():
    depth = np.full(CAM[4] * CAM[5], 1.5, F32)
    P0 = pose12(np.eye(3), np.zeros(3))
    out = track_ref.track_depth(analytic_fn(plane3, 3), depth, CAM, P0, track_ref.Opts(3, level=0.0, stride=1))
    assert out["status"] == 3 and out["iterations"] == 0 and out["passes"] == 1
    assert np.array_equal(out["pose"], P0)
    H = out["H"]
    assert H[0, 0] == 0.0 and H[1, 1] == 0.0 and H[5, 5] == 0.0 and H[2, 2] > 0


def test_max_iters_zero_evaluates_the_given_pose():
    T = pose12(rot([0, 1, 0], 0.01), np.array([0.0, 0.0, 0.01]))
    depth = depth_image(scene3, CAM, pose12(np.eye(3), np.zeros(3)))
    o = track_ref.Opts(3, level=0.0, stride=2, max_iters=0)
    out = track_ref.track_depth(analytic_fn(scene3, 3), depth, CAM, T, o)
    assert out["status"] == 1 and out["iterations"] == 0 and out["passes"] == 1
    assert np.array_equal(out["pose"], T)
    assert out["cost"] == out["cost0"] > 0
    # the same H by hand from the points and the records
    loc, pix = track_ref.points3(depth, CAM, 2)
    x = track_ref.world(loc, [float(v) for v in T], 3)
    rec = track_ref.query(analytic_fn(scene3, 3), x, 3)
    H, b, cost, cnt = track_ref.normal_equations(track_ref.tree_sum(track_ref.terms(x, rec, T[:3], 3, o)), 3)
    assert np.array_equal(H, out["H"]) and np.array_equal(b, out["b"]) and cnt == out["inliers"]
    r, inl = track_ref.residual(rec, 3, o)
    assert np.count_nonzero(np.isfinite(out["resid"])) == inl.sum()
    assert np.array_equal(out["resid"][pix[inl]], r[inl])


def test_tree_reduction_matches_exact_sum():
    rng = np.random.default_rng(7)
    for m in (0, 1, 255, 256, 257, 1000, 76800, 100003):
        T = rng.standard_normal((m, 4)) * np.exp(rng.uniform(-6, 6, (m, 1)))
        T[:, 3] = np.abs(T[:, 3])
        S = track_ref.tree_sum(T)
        for c in range(4):
            exact = math.fsum(T[:, c].tolist())
            scale = math.fsum(np.abs(T[:, c]).tolist())
            assert abs(S[c] - exact) <= 1e-12 * max(scale, 1e-300), (m, c, S[c], exact)
