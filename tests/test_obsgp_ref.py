"""CPU tests of the ObsGP reference (obsgp_ref.py): its partitions and lookups equal the oracle's, the accuracy bound holds for
the oracle's GPou (the arithmetic the HIP kernels copy) on every group of the GPU suite's shape table, and the bound and the
mask comparison reject candidates that are subtly wrong."""
import functools
import os

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import oracle_lib
import obsgp_ref as R
import replay

F32 = np.float32


def oracle_group(x, f, xq=None):
    """The oracle's GPou on one group: (L [n, n] lower, alpha) and, with queries, (mean, var)."""
    L_ = oracle_lib.lib()
    x = np.ascontiguousarray(x, dtype=F32); f = np.ascontiguousarray(f, dtype=F32)
    n = f.size
    dim = x.size // n
    oL = np.zeros(n * n, dtype=F32); oa = np.zeros(n, dtype=F32)
    L_.orc_gpou_train(oracle_lib._p(x), oracle_lib._p(f), dim, n, oracle_lib._p(oL), oracle_lib._p(oa))
    out = dict(L=np.tril(oL.reshape(n, n).T), alpha=oa)
    if xq is not None and len(xq):
        xq = np.ascontiguousarray(xq, dtype=F32)
        nq = xq.size // dim
        val = np.zeros(nq, dtype=F32); var = np.zeros(nq, dtype=F32)
        L_.orc_gpou_test(oracle_lib._p(x), oracle_lib._p(f), dim, n, oracle_lib._p(xq), nq, oracle_lib._p(val), oracle_lib._p(var))
        out.update(xq=xq.reshape(nq, dim), mean=val, var=var)
    return out


def groups2d(part, vu, f):
    px = np.asarray(vu, dtype=F32).reshape(-1, 2)
    return [R.Group(px[m], f[m]) if m.size else None for m in part.members(f)]


def groups1d(part, theta, f):
    return [R.Group(theta[m].reshape(-1, 1), f[m]) for m in part.members()]


def oracle_passes(groups, gref, q, which, tag, worst):
    """assess() of the oracle's GPou on the groups `which`, at the queries the reference lookup routes to each."""
    q = np.asarray(q, dtype=F32).reshape(len(gref), -1)
    fin = ~np.isnan(q).any(axis=1)
    for g in which:
        grp = groups[g]
        if grp is None:
            continue
        out = oracle_group(grp.x, grp.f, q[(gref == g) & fin])
        rows, ok = R.assess(grp, **out)
        worst.add("%s/g%d(n=%d)" % (tag, g, grp.n), rows)


# ------------------------------------------------------------------------------------------------ against the oracle's partitions
@pytest.fixture(scope="module")
def bigbird():
    frames = replay.load_bigbird()
    om = oracle_lib.OracleMap3(frames[0]["cam"])
    om.update(frames[0]["depth"], frames[0]["pose"])
    vu, zinv, ni, nj = om.obs()
    return om, vu, zinv, ni, nj


def test_partition2d_and_membership_equal_the_oracles(bigbird):
    om, vu, zinv, ni, nj = bigbird
    part = R.partition2d(vu, ni, nj)
    assert (part.ng0, part.ng1) == (48, 64) and part.ngroups == om.obsgp_num_tiles() == 48 * 64      # known answer: bigbird
    px = vu.reshape(-1, 2)
    mem = part.members(zinv)
    trained = 0
    for t in range(part.ngroups):
        n, x, _, _ = om.obsgp_tile(t)
        assert n == mem[t].size, t
        np.testing.assert_array_equal(x, px[mem[t]])
        trained += n > 0
    assert 50 < trained < part.ngroups            # untrained tiles are part of the case


def test_lookup2d_hit_mask_equals_the_oracles(bigbird):
    om, vu, zinv, ni, nj = bigbird
    part = R.partition2d(vu, ni, nj)
    trained = np.array([m.size > 0 for m in part.members(zinv)])
    q = R.queries2d(part, vu, seed=3)
    _, ovar = om.obsgp_query(q)
    gref = R.lookup2d(part, trained, q)
    hit = ~(ovar == R.MISS_VAR)                    # (a NaN coordinate routed to a tile answers NaN: a hit)
    np.testing.assert_array_equal(gref >= 0, hit)
    assert hit.sum() > 1000 and (~hit).sum() > 1000


def test_lookup2d_routes_a_nan_coordinate_as_the_oracle_does():
    """The reference's behaviour, not a goal: a NaN v with a regular u is answered by tile 0 of the next row of tiles (when there is
    one); a NaN u never is."""
    vu, part, f = _case2d(18, 13)
    tr = np.ones(part.ngroups, dtype=bool)
    uc = R._centres(part.valj)
    q = np.array([[np.nan, uc[0]], [np.nan, uc[1]], [np.nan, uc[2]], [0.0, np.nan], [np.nan, np.nan]], dtype=F32)
    assert list(R.lookup2d(part, tr, q)) == [part.ng0, 2 * part.ng0, -1, -1, -1]
    allq = R.queries2d(part, vu)
    nanq = np.isnan(allq).any(axis=1)
    g = R.lookup2d(part, tr, allq)
    assert (g[nanq] >= 0).any() and (g[nanq] < 0).any()


def test_partition1d_equals_the_oracles_on_the_gazebo_scan():
    fr = replay.load_gazebo()[0]
    om = oracle_lib.OracleMap2()
    om.update(fr["thetas"], fr["ranges"], fr["pose"])
    part = R.partition1d(np.asarray(fr["thetas"], dtype=F32))
    assert list(part.length) == om.obsgp_sizes() == [26] * 12 + [22, 15]                              # known answer: gazebo
    assert list(part.start) == [20 * i for i in range(12)] + [240, 255]


def test_partition1d_refuses_fewer_than_20_beams():
    for N in (1, 19):
        with pytest.raises(ValueError):
            R.partition1d(R.scan(N))
    assert R.partition1d(R.scan(20)).ngroups == 2


@pytest.mark.parametrize("ni,want", [(1, (1, 1)), (2, (1, 2)), (3, (1, 3)), (7, (1, 7)), (8, (2, 3)), (12, (2, 7)), (13, (3, 3)), (18, (4, 3))])
def test_last_tile_is_3_to_7_pixels_wide(ni, want):
    part = R.partition2d(R.lattice(ni, 3), ni, 3)
    assert (part.ng0, part.i1[-1] - part.i0[-1] + 1) == want and part.ng1 == 1


# ----------------------------------------------------------------------------------------------------------- the bound holds
def _case2d(ni, nj, kind="smooth", pattern="all", **lat):
    vu = R.lattice(ni, nj, **lat)
    part = R.partition2d(vu, ni, nj)
    f = R.validity(pattern, part, R.field2d(vu, kind), seed=ni + nj)
    return vu, part, f


def test_bound_holds_for_the_oracle_on_every_small_grid():
    worst = R.Worst()
    for ni, nj in R.GRIDS_SMALL + [R.GRID_NONSQUARE, R.GRID_WARPED]:
        lat = dict(pitch=(0.03, 0.008)) if (ni, nj) == R.GRID_NONSQUARE else dict(warp=0.3) if (ni, nj) == R.GRID_WARPED else {}
        vu, part, f = _case2d(ni, nj, "step" if (ni + nj) % 2 else "smooth", **lat)
        groups = groups2d(part, vu, f)
        q = R.queries2d(part, vu, seed=ni)
        gref = R.lookup2d(part, [g is not None for g in groups], q)
        oracle_passes(groups, gref, q, range(part.ngroups), "%dx%d" % (ni, nj), worst)
    print("\n2-D small grids, oracle GPou: " + str(worst))
    assert not worst.bad, worst.bad[:5]


@pytest.mark.parametrize("ni,nj", R.GRIDS_BIG)
def test_bound_holds_for_the_oracle_on_the_large_grids(ni, nj):
    worst = R.Worst()
    vu, part, f = _case2d(ni, nj)
    which = R.assessed_groups(part.ngroups, part.ng0)
    px = vu.reshape(-1, 2)
    mem = part.members(f)
    pick = set(which)
    groups = [R.Group(px[mem[g]], f[mem[g]]) if g in pick else None for g in range(part.ngroups)]
    q = R.queries2d(part, vu, seed=ni)
    gref = R.lookup2d(part, np.ones(part.ngroups, dtype=bool), q)
    oracle_passes(groups, gref, q, which, "%dx%d" % (ni, nj), worst)
    print("\n%d x %d, %d of %d groups, oracle GPou: %s" % (ni, nj, len(which), part.ngroups, worst))
    assert not worst.bad, worst.bad[:5]


@pytest.mark.parametrize("pattern", R.VALIDITY)
def test_bound_holds_for_the_oracle_on_every_validity_pattern(pattern):
    worst = R.Worst()
    for ni, nj in ((14, 12), (64, 48)):
        vu, part, f = _case2d(ni, nj, pattern=pattern)
        groups = groups2d(part, vu, f)
        if pattern == "all":
            assert all(g.n == 64 for g in (groups[m * part.ng0 + n] for m in range(part.ng1 - 1) for n in range(part.ng0 - 1)))
        if pattern == "one":
            assert all(g.n == 1 for g in groups)
        if pattern == "tiles":
            assert any(g is None for g in groups)
        q = R.queries2d(part, vu, seed=1)
        gref = R.lookup2d(part, [g is not None for g in groups], q)
        oracle_passes(groups, gref, q, range(part.ngroups), "%s/%dx%d" % (pattern, ni, nj), worst)
    print("\n%s, oracle GPou: %s" % (pattern, worst))
    assert not worst.bad, worst.bad[:5]


def test_bound_holds_for_the_oracle_on_every_scan_length():
    worst = R.Worst()
    for N in R.N_1D + [-271]:
        theta = R.scan(abs(N), warp=0.3 if N < 0 else 0.0)
        part = R.partition1d(theta)
        f = R.field1d(theta, "step" if N % 2 else "smooth")
        groups = groups1d(part, theta, f)
        q = R.queries1d(part, theta, seed=abs(N))
        gref = R.lookup1d(part, np.ones(part.ngroups, dtype=bool), q)
        oracle_passes(groups, gref, q, range(part.ngroups), "N%d" % N, worst)
    print("\n1-D scans, oracle GPou: " + str(worst))
    assert not worst.bad, worst.bad[:5]


# ---------------------------------------------------------------------------------------------------- the bound catches defects
def _train64(x, f, noise=R.NOISE, exp_err=0.0):
    x = np.asarray(x, dtype=np.float64)
    K = np.exp(-np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2) / R.SCALE) * (1.0 + exp_err)
    np.fill_diagonal(K, 1.0 + noise)
    L = cholesky(K, lower=True)
    return L, solve_triangular(L.T, solve_triangular(L, np.asarray(f, dtype=np.float64), lower=True), lower=False)


def _test64(x, L, alpha, xq, prior=1.0 + R.NOISE, exp_err=0.0, drop_last=False):
    x = np.asarray(x, dtype=np.float64); xq = np.asarray(xq, dtype=np.float64)
    k = np.exp(-np.linalg.norm(x[:, None, :] - xq[None, :, :], axis=2) / R.SCALE) * (1.0 + exp_err)
    v = solve_triangular(L, k, lower=True)
    n = x.shape[0] - (1 if drop_last else 0)
    return k[:n].T @ alpha[:n], prior - np.sum(v * v, axis=0)


@functools.lru_cache(maxsize=None)
def control_groups():
    """Groups the controls run on: a full tile at the suite's 6 mm pitch and one at 30 mm, a 3 x 3 last tile, a 26-beam group."""
    vu, part, f = _case2d(18, 13, "step")
    g2 = groups2d(part, vu, f)
    theta = R.scan(270)
    p1 = R.partition1d(theta)
    g1 = groups1d(p1, theta, R.field1d(theta))
    out = {}
    vu30 = R.lattice(18, 13, pitch=(0.03, 0.03))
    g30 = groups2d(R.partition2d(vu30, 18, 13), vu30, R.field2d(vu30))
    for tag, grp in (("tile64", g2[0]), ("tile64_30mm", g30[0]), ("tile_last", g2[-1]), ("beams26", g1[3])):
        rng = np.random.default_rng(grp.n)
        xq = (grp.x[rng.integers(0, grp.n, 24)].astype(np.float64) + rng.normal(0, 0.002, (24, grp.x.shape[1]))).astype(F32)
        out[tag] = (grp, xq)
    return out


CONTROL_TAGS = ("tile64", "tile64_30mm", "tile_last", "beams26")
FULL_TILES = CONTROL_TAGS[:2]


@pytest.fixture(params=CONTROL_TAGS)
def control(request):
    return (request.param,) + control_groups()[request.param]


def test_float64_candidate_passes(control):
    """The controls below alter this candidate in one place each."""
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f)
    mean, var = _test64(grp.x, L, alpha, xq)
    rows, ok = R.assess(grp, L=L.astype(F32), alpha=alpha.astype(F32), xq=xq, mean=mean.astype(F32), var=var.astype(F32))
    assert ok and set(rows) == {"factor", "alpha", "mean", "var"}, R.format_rows(rows)


def test_diagonal_without_the_noise_term_is_rejected(control):
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f, noise=0.0) if grp.n > 1 else (np.ones((1, 1)), grp.y.copy())
    rows, ok = R.assess(grp, L=L.astype(F32), alpha=alpha.astype(F32))
    assert not ok and not rows["factor"]["ok"] and not rows["alpha"]["ok"]


def test_variance_from_a_prior_of_1_is_rejected(control):
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f)
    mean, var = _test64(grp.x, L, alpha, xq, prior=1.0)
    rows, ok = R.assess(grp, xq=xq, mean=mean.astype(F32), var=var.astype(F32))
    assert not ok and not rows["var"]["ok"] and rows["mean"]["ok"]


def test_exp_with_2e_6_relative_error_is_rejected(control):
    """Rejected on the small tile and on the 26-beam group (factor 23 x, alpha 25 x, var 13 - 19 x the float32 pipeline).  On a full
    64-point tile the float32 pipeline's own error is of this size (the tile's matrix is within 0.05 of all ones off the diagonal):
    the same defect measures factor 8.5 x / var 5.5 x there (alpha 17 x at 30 mm) and stays inside the bound with its 4-ulp floor, at 6 mm and at 30 mm
    pitch alike: that is asserted too, so the finding is pinned.  The GPU suite holds every grid's last tiles, the sparse validity patterns and all 1-D groups to the bound, and
    those see it."""
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f, exp_err=2e-6)
    mean, var = _test64(grp.x, L, alpha, xq, exp_err=2e-6)
    rows, ok = R.assess(grp, L=L.astype(F32), alpha=alpha.astype(F32), xq=xq, mean=mean.astype(F32), var=var.astype(F32))
    print(tag, R.format_rows(rows))
    if tag in FULL_TILES:
        # the finding, pinned: inside the bound, although one quantity (the factor at 6 mm: 8.5 x, alpha at 30 mm: 17 x) is beyond
        # 8 x the float32 pipeline -- held by the 4-ulp floor alone
        worst = max(rows.values(), key=lambda r: r["ratio"])
        assert ok and R.RATIO < worst["ratio"] < 20 and worst["err"] <= worst["lim"]
    else:
        assert not ok and not rows["var"]["ok"]


def test_alpha_with_two_entries_swapped_is_rejected(control):
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f)
    a = alpha.copy()
    i = int(np.argmax(np.abs(a))); j = int(np.argmin(np.abs(a)))
    a[i], a[j] = alpha[j], alpha[i]
    rows, ok = R.assess(grp, alpha=a.astype(F32))
    assert not ok and not rows["alpha"]["ok"]


def test_mean_summed_over_n_minus_1_points_is_rejected(control):
    tag, grp, xq = control
    L, alpha = _train64(grp.x, grp.f)
    xq = np.concatenate([xq, grp.x[-1:]])                      # (a query next to the dropped point)
    mean, var = _test64(grp.x, L, alpha, xq, drop_last=True)
    rows, ok = R.assess(grp, xq=xq, mean=mean.astype(F32), var=var.astype(F32))
    assert not ok and not rows["mean"]["ok"] and rows["var"]["ok"]


def test_lookup_with_less_or_equal_on_a_boundary_is_rejected():
    vu, part, f = _case2d(18, 13)
    q = R.queries2d(part, vu, seed=2)
    tr = np.ones(part.ngroups, dtype=bool)
    good, bad = R.lookup2d(part, tr, q), R.lookup2d(part, tr, q, boundary_le=True)
    assert not np.array_equal(good, bad)
    on = np.isin(q[:, 0], part.vali[1:-1]) | np.isin(q[:, 1], part.valj[1:-1])
    assert np.array_equal(good[~on], bad[~on])                 # only the queries exactly on an inner boundary tell them apart
    # 1-D: a boundary belongs to no group; `<=` would answer it
    theta = R.scan(61)
    p1 = R.partition1d(theta)
    g = R.lookup1d(p1, np.ones(p1.ngroups, dtype=bool), p1.range)
    assert (g == -1).all()


def test_a_margin_of_0_0174_is_rejected():
    theta = R.scan(270)
    p1 = R.partition1d(theta)
    q = R.queries1d(p1, theta)
    tr = np.ones(p1.ngroups, dtype=bool)
    assert not np.array_equal(R.lookup1d(p1, tr, q) >= 0, R.lookup1d(p1, tr, q, margin=0.0174) >= 0)
    vu, part, f = _case2d(18, 13)
    q = R.queries2d(part, vu)
    tr = np.ones(part.ngroups, dtype=bool)
    assert not np.array_equal(R.lookup2d(part, tr, q) >= 0, R.lookup2d(part, tr, q, margin=0.0049) >= 0)


# ------------------------------------------------------------------------------------------------------------- known answers
def test_one_point_group_has_the_closed_form():
    grp = R.Group(np.array([[0.1, -0.2]], dtype=F32), np.array([0.625], dtype=F32))
    np.testing.assert_allclose(grp.alpha64, [0.625 / (1.0 + R.NOISE)], rtol=1e-15)
    mean, var = grp.predict64(grp.x)
    np.testing.assert_allclose(var, [(1.0 + R.NOISE) - 1.0 / (1.0 + R.NOISE)], rtol=1e-13)
    np.testing.assert_allclose(mean, [0.625 / (1.0 + R.NOISE)], rtol=1e-15)
    out = oracle_group(grp.x, grp.f, grp.x)
    assert abs(float(out["alpha"][0]) - 0.625 / 1.01) <= R.ULP and R.assess(grp, **out)[1]     # (two divisions by L: one ulp)
    m32, v32 = grp.predict32(grp.x)
    assert abs(float(v32[0]) - (1.01 - 1 / 1.01)) < 4 * R.ULP


def test_two_coincident_points():
    """K = [[1.01, 1], [1, 1.01]]: alpha = (f1 + f2) / (2.01 * 0.01) * [1.01, -1; -1, 1.01] f ... in closed form."""
    x = np.array([[0.3, 0.3], [0.3, 0.3]], dtype=F32); f = np.array([0.5, 0.75], dtype=F32)
    grp = R.Group(x, f)
    K = np.array([[1.0 + R.NOISE, 1.0], [1.0, 1.0 + R.NOISE]])
    np.testing.assert_allclose(grp.alpha64, np.linalg.solve(K, f.astype(np.float64)), rtol=1e-12)
    mean, var = grp.predict64(x[:1])
    k = np.array([1.0, 1.0])
    np.testing.assert_allclose(var, [(1.0 + R.NOISE) - k @ np.linalg.solve(K, k)], rtol=1e-10)
    out = oracle_group(x, f, x[:1])
    rows, ok = R.assess(grp, **out)
    assert ok, R.format_rows(rows)


def test_reachable_cells_of_the_lattices():
    """At most the last row and the last column of tiles can be swallowed by the margins on the suite's lattices; a one-pixel
    axis (both table entries on the same pixel) is swallowed whole."""
    for ni, nj in R.GRIDS_SMALL + R.GRIDS_BIG:
        part = R.partition2d(R.lattice(ni, nj), ni, nj)
        r = part.reachable().reshape(part.ng1, part.ng0)
        assert r[:-1, :-1].all(), (ni, nj)
        assert r.any() == (ni > 2 and nj > 2), (ni, nj)
    for N in R.N_1D:
        assert R.partition1d(R.scan(N)).reachable().all(), N


def test_query_route_symbol_is_exported():
    import gpismap_amd
    L = gpismap_amd.lib()
    hdr = open(os.path.join(oracle_lib.ROOT, "include", "gpismap_amd.h")).read()
    doc = open(os.path.join(oracle_lib.ROOT, "INTEGRATION.md")).read()
    for name in ("gpis_obsgp_query_route", "gpis_obsgp_pending"):
        assert hasattr(L, name), name
        assert "int   %s(" % name in hdr and name in doc, name
    for meth in ("query_route", "query_begin_b", "query_end_b", "pending"):
        assert callable(getattr(gpismap_amd.ObsGP, meth, None)), meth
