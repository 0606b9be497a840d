"""The distance-field reference (tests/dfield_ref.py) against its own contract: the separable passes against a brute force over all
sites, scipy's exact EDT, the mesh vertices, the bound of DESIGN §7e, analytic fields and the sampling rules.  CPU only."""
import numpy as np
import pytest

import dfield_ref as R
import mesh_ref

F32 = np.float32


def _random_shapes(rng, k):
    out = []
    for t in range(k):
        dim = 2 + t % 2
        out.append(tuple(int(v) for v in rng.integers(2, 12, dim)))
    return out + [(2, 2), (2, 2, 2), (2, 9, 2), (13, 2), (7, 2, 11), (1 + 2 * 5, 1 + 2 * 4, 1 + 2 * 3)]


def _symmetric_sites(shape):
    """Sites in mirror-symmetric patterns: every point has many equidistant nearest sites."""
    g = np.meshgrid(*[np.arange(n) for n in shape[::-1]], indexing="ij")
    s = np.zeros(shape[::-1], bool)
    for a in range(len(shape)):
        s |= (g[a] == 0) | (g[a] == shape[::-1][a] - 1)           # the box's faces
    c = np.zeros(shape[::-1], bool)
    c[tuple(n // 2 for n in shape[::-1])] = True
    corners = np.zeros(shape[::-1], bool)
    corners[tuple(slice(None, None, max(1, n - 1)) for n in shape[::-1])] = True
    chk = (sum(g) % 3 == 0)
    return [s.ravel(), c.ravel(), corners.ravel(), chk.ravel(), (c | corners).ravel()]


def test_separable_passes_equal_brute_force():
    rng = np.random.default_rng(0)
    for shape in _random_shapes(rng, 60):
        n = int(np.prod(shape))
        pats = [rng.random(n) < p for p in (0.02, 0.2, 0.6)] + _symmetric_sites(shape)
        one = np.zeros(n, bool)
        one[rng.integers(n)] = True
        pats += [one, np.zeros(n, bool), np.ones(n, bool)]
        for site in pats:
            assert np.array_equal(R.edt_separable(site, shape), R.edt_brute(site, shape)), shape


def test_squared_distances_equal_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for shape in [(17, 9, 6), (31, 23), (2, 40, 3), (50, 2)]:
        n = int(np.prod(shape))
        for p in (0.01, 0.1, 0.5):
            site = rng.random(n) < p
            site[rng.integers(n)] = True
            q = R.edt_separable(site, shape)
            ours = R._d2(np.arange(n), q, shape)
            d = nd.distance_transform_edt(~site.reshape(shape[::-1]))
            assert np.array_equal(np.rint(d.ravel() ** 2).astype(np.int64), ours), shape


def _smooth(shape, origin, step, seed):
    rng = np.random.default_rng(seed)
    X = mesh_ref.lattice(shape, origin, [step] * len(shape)).astype(np.float64)
    f = np.zeros(X.shape[0])
    for _ in range(5):
        k = rng.normal(0, 2.0, X.shape[1])
        f += np.sin(X @ k + rng.uniform(0, 6.3))
    return f.astype(F32)


def _cases():
    yield _smooth((23, 19, 14), (-0.5, 0.2, 0.0), 0.1, 2), (23, 19, 14), (-0.5, 0.2, 0.0), 0.1, 0.2
    yield _smooth((47, 38), (1.0, -1.0), 0.05, 3), (47, 38), (1.0, -1.0), 0.05, -0.3
    v = (np.round(_smooth((21, 17, 9), (0.0, 0.0, 0.0), 0.2, 4) * 2) / 2).astype(F32)   # exact ties at the level
    v[np.random.default_rng(5).choice(v.size, 200, replace=False)] = np.nan
    yield v, (21, 17, 9), (0.0, 0.0, 0.0), 0.2, 0.5


def test_anchors_are_mesh_vertices():
    for val, shape, origin, step, level in _cases():
        site, _ = R.sites(val, shape, level)
        idx = np.nonzero(site)[0]
        assert idx.size > 50
        a = R.anchors(val, shape, origin, step, level, idx)
        verts, _, _, _ = mesh_ref.extract(val, shape, origin, [step] * len(shape), level)
        vk = {row.tobytes() for row in np.ascontiguousarray(verts)}
        assert all(row.tobytes() in vk for row in np.ascontiguousarray(a))


def test_bound_against_every_anchor():
    """d_min <= |dist| <= d_min + 2 s, d_min in float64 over every site's anchor (float32 rounding of dist allowed for)."""
    for val, shape, origin, step, level in _cases():
        dim = len(shape)
        dist, q = R.distance_field(val, shape, origin, step, level)
        site, ins = R.sites(val, shape, level)
        idx = np.nonzero(site)[0]
        A = R.anchors(val, shape, origin, step, level, idx).astype(np.float64)
        X = mesh_ref.lattice(shape, origin, [step] * dim).astype(np.float64)
        dmin = np.full(X.shape[0], np.inf)
        for b in range(0, A.shape[0], 256):
            d = np.sqrt(((X[:, None, :] - A[None, b:b + 256, :]) ** 2).sum(2))
            dmin = np.minimum(dmin, d.min(1))
        ad = np.abs(dist.astype(np.float64))
        tol = 1e-6 * (1 + ad)
        assert np.all(ad >= dmin - tol)
        assert np.all(ad <= dmin + 2 * step + tol)
        assert np.array_equal(dist < 0, ins)
        assert np.all(site[q])


# Tolerances of the analytic fields, in steps.  First CPU run: sphere max 0.67 (3-D) / 0.64 (2-D); tilted plane max 0.56 /
# 0.42 over the points whose foot point lies at least 2 steps inside the box (outside that, the nearest surface point is off
# the lattice).  Rule 6 bounds the error by 2 steps plus the distance of the anchors from the true surface (linear crossings
# of a curved f); 1 step leaves room for neither.
ANALYTIC_TOL_STEPS = 1.0


@pytest.mark.parametrize("dim", [2, 3])
def test_analytic_fields(dim):
    shape = (41, 37, 33)[:dim] if dim == 3 else (61, 53)
    step = 0.05
    origin = [-(n - 1) * step / 2 for n in shape]
    X = mesh_ref.lattice(shape, origin, [step] * dim).astype(np.float64)
    r = np.sqrt((X ** 2).sum(1))
    R0 = 0.6
    d, _ = R.distance_field((r - R0).astype(F32), shape, origin, step, 0.0)
    assert np.abs(d - (r - R0)).max() <= ANALYTIC_TOL_STEPS * step
    nrm = np.array([0.3, -0.5, 0.81][:dim])
    nrm /= np.linalg.norm(nrm)
    exact = X @ nrm - 0.1
    d, _ = R.distance_field(exact.astype(F32), shape, origin, step, 0.0)
    foot = X - exact[:, None] * nrm
    lo = np.array(origin) + 2 * step
    hi = np.array(origin) + (np.array(shape) - 1 - 2) * step
    inner = np.all((foot >= lo) & (foot <= hi), axis=1)
    assert inner.sum() > X.shape[0] // 3
    assert np.abs(d - exact)[inner].max() <= ANALYTIC_TOL_STEPS * step


def test_no_sites_gives_infinities():
    shape = (5, 4, 3)
    v = np.ones((3, 4, 5), F32)
    v[0, 0, 0] = -1.0                                    # one inside point walled off by NaN: no finite crossing
    v[0, 0, 1] = np.nan
    v[0, 1, 0] = np.nan
    v[1, 0, 0] = np.nan
    d, q = R.distance_field(v.ravel(), shape, (0, 0, 0), 1.0, 0.0)
    assert np.all(q == -1)
    assert d[0] == -np.inf and np.all(d[1:] == np.inf)


def test_sampling_rules():
    shape, origin, step = (9, 7, 6), (0.5, -1.0, 2.0), F32(0.25)
    rng = np.random.default_rng(7)
    field = rng.normal(size=int(np.prod(shape))).astype(F32)
    X = mesh_ref.lattice(shape, origin, [step] * 3)
    out = R.sample(field, shape, origin, step, X)
    # lattice points (u exact for this origin and step): the lattice value, exactly off the upper faces (there w = 1, and
    # a + (b - a) rounds)
    upper = np.zeros(shape[::-1], bool)
    upper[-1], upper[:, -1], upper[:, :, -1] = True, True, True
    upper = upper.ravel()
    assert np.array_equal(out[~upper, 0], field[~upper])
    assert np.allclose(out[upper, 0], field[upper], rtol=1e-6, atol=1e-6)
    # along an axis inside one cell the interpolant is linear: equal steps give equal differences (up to rounding)
    base = np.array([0.5 + 2 * 0.25, -1.0 + 3 * 0.25, 2.0 + 1 * 0.25])
    t = np.linspace(0.05, 0.95, 10)
    for a in range(3):
        x = np.repeat(base[None], t.size, 0)
        x[:, a] += t * 0.25
        v = R.sample(field, shape, origin, step, x.astype(F32))[:, 0].astype(np.float64)
        dv = np.diff(v)
        assert np.allclose(dv, dv[0], atol=1e-5)
    # the gradient against central differences inside cells
    x = (np.array(origin) + rng.uniform(0.3, 0.7, (200, 3)) * step + rng.integers(0, 4, (200, 3)) * step).astype(F32)
    g = R.sample(field, shape, origin, step, x)
    h = 1e-3
    for a in range(3):
        xp, xm = x.astype(np.float64).copy(), x.astype(np.float64).copy()
        xp[:, a] += h
        xm[:, a] -= h
        cd = (R.sample(field, shape, origin, step, xp.astype(F32))[:, 0].astype(np.float64)
              - R.sample(field, shape, origin, step, xm.astype(F32))[:, 0]) / (2 * h)
        assert np.allclose(g[:, 1 + a], cd, rtol=2e-2, atol=2e-2)
    # outside the lattice: NaN; exactly on the upper faces: inside
    up = np.array([[0.5 + 8 * 0.25, -1.0 + 6 * 0.25, 2.0 + 5 * 0.25]], F32)
    assert np.all(np.isfinite(R.sample(field, shape, origin, step, up)))
    assert np.isclose(R.sample(field, shape, origin, step, up)[0, 0], field[-1], rtol=1e-6, atol=1e-6)
    out = R.sample(field, shape, origin, step, np.array([[0.49, 0.0, 2.5], [1.0, -1.0, 3.26], [np.nan, 0, 2.5]], F32))
    assert np.all(np.isnan(out))
