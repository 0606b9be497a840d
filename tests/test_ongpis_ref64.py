"""CPU tests of the float64 OnGPIS reference (ongpis_ref64.py): it restates arbiter64 and the oracle's kernel matrix, the
accuracy bound holds for the oracle's `tiled` arithmetic (the operation order the HIP kernels reproduce bit for bit) on every
size class up to K = 3600, and the checker rejects a factor, an alpha and a prediction that are subtly wrong."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

import oracle_lib
import ongpis_ref64 as R

sys.path.insert(0, os.path.join(oracle_lib.ROOT, "oracle"))
import arbiter64  # noqa: E402

from test_gpu_ongpis import make_cluster  # noqa: E402


def oracle_kernel_matrix(p):
    """The oracle's build of Problem p's kernel matrix (lower triangle)."""
    ng = int((p.gidx >= 0).sum())
    Kc = np.zeros(p.K * p.K, dtype=np.float32)
    oracle_lib.lib().orc_matern32_train(p.dim, p.pos.shape[0], oracle_lib._p(np.ascontiguousarray(p.pos)),
                                        oracle_lib._p(p.gidx.astype(np.int32), C.c_int), ng, C.c_float(p.scale),
                                        oracle_lib._p(p.sigx.astype(np.float32)), oracle_lib._p(p.sg), oracle_lib._p(Kc))
    return np.tril(Kc.reshape(p.K, p.K).T)


def problem(dim, scale, n, frac_nograd, dense=1.0, seed=0):
    rng = np.random.default_rng(seed + 7 * n + dim)
    pos, grad, val, sx, sg = make_cluster(rng, dim, n, scale * dense, frac_nograd=frac_nograd)
    return R.Problem(dim, scale, pos, grad, val, sx, sg, R.queries(rng, pos, scale))


def oracle_outputs(p):
    o = oracle_lib.ongpis_train(p.dim, p.scale, p.pos, p.grad, p.val, p.sx, p.sg)
    assert o["K"] == p.K
    np.testing.assert_array_equal(o["gidx"], p.gidx.astype(np.int32))
    pr = oracle_lib.ongpis_predict(p.dim, p.scale, p.pos, p.grad, p.val, p.sx, p.sg, p.xq)
    nc = 1 + p.dim
    return dict(Kmat=oracle_kernel_matrix(p), L=o["L"], alpha=o["alpha"], mean=pr[:, :nc], var=pr[:, nc:])


@pytest.mark.parametrize("dim,scale,n", [(3, 0.04, 1), (3, 0.04, 23), (2, 1.2, 1), (2, 1.2, 19)])
def test_reference_equals_arbiter64(dim, scale, n):
    """Gather, kernel matrix, k*, factor, alpha and predictions equal the loop-by-loop arbiter to float64 round-off (value-only
    points of both kinds mixed in)."""
    rng = np.random.default_rng(50 + n + dim)
    pos, grad, val, sx, sg = make_cluster(rng, dim, n, scale, frac_nograd=0.4)
    if n > 1:
        grad[-1] = 0.0; sg[-2] = 0.5                          # both value-only rules also at the end of the list
    a = arbiter64.ongpis_train(pos, grad, val, sx, sg, scale)
    r = R.train(pos, grad, val, sx, sg, scale)
    np.testing.assert_array_equal(r["gidx"], a["gidx"])
    assert r["K"] == a["K"]
    gidx, sigx, sigg, y = R.gather(pos, grad, val, sx, sg)
    Ka = arbiter64.matern_train_K(pos, a["gidx"], scale, sigx, sigg)
    Kr = R.kernel_matrix(pos, gidx, scale, sigx, sigg)
    assert np.abs(Kr - Ka).max() <= 1e-12 * np.abs(Ka).max()
    assert np.abs(r["L"] - a["L"]).max() <= 1e-12 * np.abs(a["L"]).max()
    assert np.abs(r["alpha"] - a["alpha"]).max() <= 1e-12 * np.abs(a["alpha"]).max()
    xq = R.queries(rng, pos, scale, n_each=3)
    ks = R.cross(pos, gidx, scale, xq)
    mean, var = R.predict(r["L"], r["alpha"], ks, dim, scale)
    for q in range(xq.shape[0]):
        kq = arbiter64.matern_cross(pos, a["gidx"], scale, xq[q])
        assert np.abs(ks[:, q, :] - kq).max() <= 1e-12 * max(np.abs(kq).max(), 1e-300)
        ma, va = arbiter64.ongpis_test(a, xq[q])
        assert np.abs(mean[q] - ma).max() <= 1e-12 * (1 + np.abs(ma).max())
        assert np.abs(var[q] - va).max() <= 1e-12 * np.abs(va).max()


@pytest.mark.parametrize("dim,scale,n", [(3, 0.04, 60), (3, 0.04, 150), (2, 1.2, 40)])
def test_reference_matrix_equals_the_oracles(dim, scale, n):
    """Same bar as test_oracle.py's comparison of the oracle's build with arbiter64."""
    p = problem(dim, scale, n, 0.3)
    K64 = np.tril(p.K64())
    assert np.abs(oracle_kernel_matrix(p) - K64).max() < 2e-6 * np.abs(K64).max()


# (dim, scale, N, fraction value-only, patch density): every size class of the training and prediction kernels up to K = 3600
TILED_SHAPES = [
    (3, 0.04, 1, 0.0, 1.0),       # K = 4
    (3, 0.04, 8, 0.0, 1.0),       # K = 32: one block row
    (3, 0.04, 64, 0.0, 1.0),      # K = 256: the largest fused cluster
    (3, 0.04, 257, 1.0, 1.0),     # K = 257 value-only: first separate one
    (3, 0.04, 65, 0.0, 1.0),      # K = 260
    (3, 0.04, 150, 0.3, 1.0),     # mixed
    (3, 0.04, 150, 0.0, 0.2),     # dense
    (3, 0.04, 300, 0.0, 1.0),     # K = 1200: cooperative
    (3, 0.04, 300, 0.2, 0.2),
    (3, 0.04, 600, 0.0, 1.0),     # K = 2400
    (3, 0.04, 900, 0.0, 1.0),     # K = 3600: four row groups of K4
    (3, 0.04, 3600, 1.0, 3.5),    # K = 3600 value-only, at a 300-point cluster's density: the fmaf-chain effect (chain_ratio)
    (2, 1.2, 1, 0.0, 1.0),        # K = 3
    (2, 1.2, 40, 0.2, 1.0),
    (2, 1.2, 100, 0.0, 0.2),
    (2, 1.2, 400, 0.1, 1.0),      # K = 1160
]


@pytest.mark.parametrize("shape", TILED_SHAPES, ids=lambda s: "d%d_n%d_v%g_x%g" % (s[0], s[2], s[3], s[4]))
def test_bound_holds_for_the_tiled_arithmetic(shape):
    dim, scale, n, frac, dense = shape
    p = problem(dim, scale, n, frac, dense)
    t0 = time.time()
    out = oracle_outputs(p)
    t1 = time.time()
    rows, ok = R.assess(p, **out)
    print("\nK=%d  %s  (oracle %.1fs, reference %.1fs)" % (p.K, R.format_rows(rows), t1 - t0, time.time() - t1))
    assert set(rows) == {"build", "factor", "alpha", "f", "grad", "var_f", "var_g", "own_f", "own_grad", "own_var_f", "own_var_g"}
    assert ok, R.format_rows(rows)


@pytest.fixture(scope="module")
def k510():
    p = problem(3, 0.04, 150, 0.2)            # K = 510: value and gradient rows, 16 block rows
    return p, oracle_outputs(p)


def test_checker_accepts_the_unaltered_outputs(k510):
    p, out = k510
    assert R.assess(p, **out)[1]


@pytest.mark.parametrize("tile", [(1, 0), (9, 7)])
def test_checker_rejects_one_tile_of_the_factor_off_by_2e_12(k510, tile):
    """One off-diagonal 32 x 32 tile of L scaled by (1 + 2^-12), once among the value rows, once among the gradient rows."""
    p, out = k510
    L = out["L"].copy()
    bi, bj = tile
    L[32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32] *= np.float32(1 + 2.0 ** -12)
    assert not np.array_equal(L, out["L"])
    rows, ok = R.assess(p, Kmat=out["Kmat"], L=L)
    assert not rows["factor"]["ok"] and not ok


def test_checker_rejects_alpha_with_one_entry_zeroed(k510):
    p, out = k510
    a = out["alpha"].copy()
    a[np.argmax(np.abs(a))] = 0.0
    rows, ok = R.assess(p, Kmat=out["Kmat"], alpha=a)
    assert not rows["alpha"]["ok"] and not ok


def test_checker_rejects_a_prediction_without_one_row_of_k_star(k510):
    """Predictions from the candidate's own L and alpha in float64, but with the row of k* that weighs most in the first query's
    mean left out (a row dropped from a K4 chunk)."""
    p, out = k510
    ks = p.ks64().copy()
    row = int(np.argmax(np.abs(ks[:, 0, 0] * out["alpha"])))
    ks[row] = 0.0
    mean, var = R.predict(np.tril(out["L"]), out["alpha"], ks, p.dim, p.scale)
    rows, ok = R.assess(p, L=None, alpha=None, mean=mean, var=var)
    assert not ok
    rows, ok = R.assess(p, Kmat=out["Kmat"], L=out["L"], alpha=out["alpha"], mean=mean, var=var)
    assert not rows["own_f"]["ok"] and not ok


@pytest.mark.parametrize("N,ng,dim", [(4096, 4096, 3), (6000, 2000, 3), (7256, 0, 3), (5183, 5183, 2), (300, 100, 3)])
def test_row_group_queries_reach_every_row_group(N, ng, dim):
    """Each row group of 1024 rows of K holds a row of the point its query is placed next to."""
    rng = np.random.default_rng(N)
    gidx = np.full(N, -1, dtype=np.int64)
    gidx[rng.permutation(N)[:ng]] = rng.permutation(ng)
    K = N + dim * ng
    pts = R.row_group_points(gidx, K)
    assert pts.size == -(-K // 1024)
    for g, k in enumerate(pts):
        rows = [k] + ([N + c * ng + gidx[k] for c in range(dim)] if gidx[k] >= 0 else [])
        assert any(1024 * g <= r < 1024 * (g + 1) for r in rows), (g, k, rows)
    pos = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    xq = R.row_group_queries(rng, pos, gidx, K, 0.04)
    assert xq.shape == (pts.size, dim) and np.abs(xq - pos[pts]).max() < 0.04
