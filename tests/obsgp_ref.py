"""Reference of the observation GP (ObsGP2D / ObsGP1D / GPou) and the accuracy bound its kernels are held to.

Test infrastructure only (numpy + scipy).  Written from oracle/gp.hpp and oracle/arbiter64.py, not from the kernels:
  partition2d / partition1d   index ranges, float32 boundary tables, group membership
  lookup2d / lookup1d         the group a query falls into, compared in float32 as the oracle compares
  Group                       one group's float64 train / predict (arbiter64.ou_train / ou_test) and the plain float32 LAPACK
                              pipeline on the same float32 operands (numpy float32 build, spotrf, strtrs): the baseline
  assess                      error(candidate) <= RATIO * error(float32 pipeline) + FLOOR_ULP ulp, both against float64
The bound and its constants are ongpis_ref64's (RATIO = 8, FLOOR_ULP = 4), not retuned.  Quantities:
  factor   max |L L^T - K64|_ij / sqrt(K_ii K_jj)
  alpha    |K alpha - y|_inf / (|K| |alpha| + |y|)_inf on the float64 matrix
  mean     max over the group's queries of |mean - mean64|, scale max |mean64|
  var      max over the group's queries of |var - var64|, scale the prior 1.01"""
import os
import sys

import numpy as np
from scipy.linalg import lapack

from ongpis_ref64 import RATIO, FLOOR_ULP, ULP, format_rows  # noqa: F401  (the project's bound, as it stands there)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import arbiter64  # noqa: E402

F32 = np.float32
MARGIN2 = F32(0.005)      # ObsGP2D::margin
MARGIN1 = F32(0.0175)     # ObsGP1D::margin
OVERLAP2, GROUP2 = 3, 5
OVERLAP1, GROUP1 = 6, 20
SCALE = 0.5
NOISE = float(F32(0.01))  # the float32 operand, seen in float64
PRIOR32 = F32(1) + F32(0.01)
MISS_VAR = F32(1e6)


def _cdiv(a, b):
    """C++ integer division (truncation toward zero): (ni - 3) / 5 for ni < 3."""
    return int(a / b) if a * b < 0 else a // b


# ----------------------------------------------------------------------------------------------------------------- partitions
class Partition2D:
    """ObsGP2D::computePartition.  Pixel (i, j) is element j * ni + i; vu[2 * ind] runs with i (table vali), vu[2 * ind + 1] with
    j (valj).  Group g = m * ng0 + n is tile n along i, m along j."""

    def __init__(self, vu, ni, nj):
        vu = np.asarray(vu, dtype=F32).reshape(-1)
        assert vu.size == 2 * ni * nj and ni > 0 and nj > 0
        self.ni, self.nj = ni, nj
        self.ng0 = _cdiv(ni - OVERLAP2, GROUP2) + 1
        self.ng1 = _cdiv(nj - OVERLAP2, GROUP2) + 1
        self.ngroups = self.ng0 * self.ng1

        def axis(ng, size, stride, off):
            a0, a1, tab = [], [], [vu[off]]
            for n in range(ng):
                a = n * GROUP2
                b = a + GROUP2 + OVERLAP2 - 1
                if n < ng - 1:
                    tab.append(vu[2 * (b - OVERLAP2 // 2) * stride + off])
                else:
                    b = size - 1
                    tab.append(vu[2 * b * stride + off])
                a0.append(a); a1.append(b)
            return np.array(a0), np.array(a1), np.array(tab, dtype=F32)

        self.i0, self.i1, self.vali = axis(self.ng0, ni, 1, 0)
        self.j0, self.j1, self.valj = axis(self.ng1, nj, ni, 1)

    def pixels(self, g):
        """Pixel indices of group g, j-outer / i-inner."""
        n, m = g % self.ng0, g // self.ng0
        jj, ii = np.meshgrid(np.arange(self.j0[m], self.j1[m] + 1), np.arange(self.i0[n], self.i1[n] + 1), indexing="ij")
        return (jj * self.ni + ii).reshape(-1)

    def members(self, f):
        """Per group: the pixel indices with f > 0 in compaction order (NaN, 0 and negative f are all invalid by f > 0)."""
        f = np.asarray(f, dtype=F32).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok = f > 0
        out = []
        for g in range(self.ngroups):
            p = self.pixels(g)
            out.append(p[ok[p]])
        return out

    def reachable(self):
        """bool [ngroups]: the group's lookup cell holds at least one float32 point that passes the margin tests."""
        def axis(tab):
            ng = tab.size - 1
            liml, limr = tab[0] + MARGIN2, tab[-1] - MARGIN2
            lo = np.array([liml if n == 0 else max(tab[n], liml) for n in range(ng)], dtype=F32)
            return (lo < tab[1:]) & (lo <= limr)
        return (axis(self.valj)[:, None] & axis(self.vali)[None, :]).reshape(-1)


def partition2d(vu, ni, nj):
    return Partition2D(vu, ni, nj)


class Partition1D:
    """ObsGP1D::train: groups of 26 beams every 20, the last 20 to 39 beams split into two."""

    def __init__(self, theta):
        theta = np.asarray(theta, dtype=F32).reshape(-1)
        N = theta.size
        if N < GROUP1:
            raise ValueError("ObsGP1D needs at least %d beams (got %d): nGroup = N / 20 + 1 leaves no group" % (GROUP1, N))
        ngr = N // GROUP1 + 1
        start, length, rng = [], [], [theta[0]]
        n = 0
        while n < ngr - 1:
            if n < ngr - 2:
                a = n * GROUP1
                b = a + GROUP1 + OVERLAP1
                rng.append(theta[b - OVERLAP1 // 2])
                start.append(a); length.append(GROUP1 + OVERLAP1)
            else:
                a = n * GROUP1
                b = a + (N - a) // 2 + OVERLAP1
                rng.append(theta[b - OVERLAP1 // 2])
                start.append(a); length.append(b - a + 1)
                n += 1
                a = a + (N - a) // 2
                b = N - 1
                rng.append(theta[b])
                start.append(a); length.append(b - a + 1)
            n += 1
        self.N = N
        self.start, self.length = np.array(start), np.array(length)
        self.range = np.array(rng, dtype=F32)
        self.ngroups = self.start.size

    def members(self):
        return [np.arange(a, a + n) for a, n in zip(self.start, self.length)]

    def reachable(self):
        r = self.range
        liml, limr = r[0] + MARGIN1, r[-1] - MARGIN1
        lo = np.maximum(np.nextafter(r[:-1], F32(np.inf)), liml)
        hi = np.minimum(np.nextafter(r[1:], F32(-np.inf)), limr)
        return lo <= hi


def partition1d(theta):
    return Partition1D(theta)


# -------------------------------------------------------------------------------------------------------------------- lookups
def _first_less(q, tab, chunk=1 << 15):
    """Per query the count of k = 1 .. len(tab) - 1 passed before q < tab[k] first holds (all of them when it never does)."""
    out = np.empty(q.size, dtype=np.int64)
    for s in range(0, q.size, chunk):
        with np.errstate(invalid="ignore"):
            lt = q[s:s + chunk, None] < tab[None, 1:]
        out[s:s + chunk] = np.where(lt.any(axis=1), lt.argmax(axis=1), tab.size - 1)
    return out


def lookup2d(part, trained, q, margin=MARGIN2, boundary_le=False):
    """ObsGP2D::lookup for q [nq, 2] float32: the group index, or -1.  `trained`: bool [ngroups].  Every comparison is a float32
    one, against float32(table) +- float32(margin).
    The reference's behaviour for NaN (not a goal): every comparison with NaN is false, so the margin tests pass and the loop of
    that axis runs to its end (n = ng0, or m = ng1); the index m * ng0 + n that results is answered when it names a trained
    group (a NaN v with a regular u lands on tile 0 of the next row)."""
    q = np.asarray(q, dtype=F32).reshape(-1, 2)
    margin = F32(margin)
    v, u = q[:, 0], q[:, 1]
    with np.errstate(invalid="ignore"):
        out_ = (v < part.vali[0] + margin) | (v > part.vali[-1] - margin) | (u < part.valj[0] + margin) | (u > part.valj[-1] - margin)
    if boundary_le:       # (a defective lookup, for the negative control: `<=` on a boundary)
        n = np.array([next((k - 1 for k in range(1, part.vali.size) if x <= part.vali[k]), part.ng0) for x in v], dtype=np.int64)
        m = np.array([next((k - 1 for k in range(1, part.valj.size) if x <= part.valj[k]), part.ng1) for x in u], dtype=np.int64)
    else:
        n, m = _first_less(v, part.vali), _first_less(u, part.valj)
    ind = m * part.ng0 + n
    trained = np.asarray(trained, dtype=bool)
    ok = ~out_ & (ind < part.ngroups)
    ok[ok] = trained[ind[ok]]
    return np.where(ok, ind, -1)


def lookup1d(part, trained, q, margin=MARGIN1):
    """ObsGP1D::lookup: the first k with range[k] < q < range[k + 1] (strict, float32) inside [range[0] + margin,
    range[-1] - margin]; -1 otherwise, on a boundary, and for NaN (every comparison false)."""
    q = np.asarray(q, dtype=F32).reshape(-1)
    margin = F32(margin)
    r = part.range
    with np.errstate(invalid="ignore"):
        out_ = (q < r[0] + margin) | (q > r[-1] - margin)
        inside = (q[:, None] > r[None, :-1]) & (q[:, None] < r[None, 1:])
    k = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    ok = ~out_ & (k >= 0)
    ok[ok] = np.asarray(trained, dtype=bool)[k[ok]]
    return np.where(ok, k, -1)


# ------------------------------------------------------------------------------------------------------------------ one group
def _dist(a, b, dt):
    a = np.asarray(a).astype(dt); b = np.asarray(b).astype(dt)
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


class Group:
    """One group's training set (x [n, dim] float32, f [n] float32): float64 and float32-pipeline quantities, computed once."""

    def __init__(self, x, f):
        self.x = np.ascontiguousarray(x, dtype=F32).reshape(len(f), -1)
        self.f = np.ascontiguousarray(f, dtype=F32)
        self.n = self.f.size
        self.y = self.f.astype(np.float64)
        self.K64 = np.exp(-_dist(self.x, self.x, np.float64) / SCALE)
        np.fill_diagonal(self.K64, 1.0 + NOISE)
        self.L64, self.alpha64 = arbiter64.ou_train(self.x, self.f, SCALE, NOISE)
        K32 = np.exp(-F32(1 / SCALE) * _dist(self.x, self.x, F32)).astype(F32)
        np.fill_diagonal(K32, PRIOR32)
        c, info = lapack.spotrf(K32, lower=1)
        assert info == 0
        self.L32 = np.tril(c)
        z, info = lapack.strtrs(self.L32, self.f, lower=1)
        assert info == 0
        self.alpha32, info = lapack.strtrs(self.L32, z, lower=1, trans=1)
        assert info == 0

    def predict64(self, xq):
        xq = np.asarray(xq, dtype=F32).reshape(-1, self.x.shape[1])
        ok = ~np.isnan(xq).any(axis=1)          # (a NaN coordinate makes every k* entry NaN, and with it the mean and the variance)
        mean = np.full(xq.shape[0], np.nan); var = np.full(xq.shape[0], np.nan)
        if ok.any():
            mean[ok], var[ok] = arbiter64.ou_test(self.x, self.L64, self.alpha64, xq[ok], SCALE, NOISE)
        return mean, var

    def predict32(self, xq):
        xq = np.asarray(xq, dtype=F32).reshape(-1, self.x.shape[1])
        k = np.exp(-F32(1 / SCALE) * _dist(self.x, xq, F32)).astype(F32)      # [n, nq]
        mean = k.T @ self.alpha32
        v, info = lapack.strtrs(self.L32, k, lower=1)
        assert info == 0
        return mean, PRIOR32 - (v * v).sum(axis=0, dtype=F32)


def factor_error(L, K64):
    n = K64.shape[0]
    L = np.tril(np.asarray(L, dtype=np.float64)[:n, :n])
    s = 1.0 / np.sqrt(np.diag(K64))
    return float((np.abs(L @ L.T - K64) * s[:, None] * s[None, :]).max())


def alpha_error(alpha, K64, y):
    al = np.asarray(alpha, dtype=np.float64)[:y.size]
    return float(np.abs(K64 @ al - y).max() / (np.abs(K64) @ np.abs(al) + np.abs(y)).max())


def _judge(name, err, base, scale, rows):
    lim = RATIO * base + FLOOR_ULP * ULP * scale
    ratio = err / base if base > 0 else (0.0 if err == 0 else np.inf)
    rows[name] = dict(err=err, base=base, ratio=ratio, lim=lim, ok=bool(np.isfinite(err) and err <= lim))


def assess(grp, L=None, alpha=None, xq=None, mean=None, var=None):
    """Holds what a candidate computed for Group `grp` to the bound.  L: its factor (lower, [>= n, >= n]); alpha; mean / var: its
    answers at the queries xq (all of them finite).  Returns (rows, ok); rows[name] = dict(err, base, ratio, ok)."""
    rows = {}
    if L is not None:
        _judge("factor", factor_error(L, grp.K64), factor_error(grp.L32, grp.K64), 1.0, rows)
    if alpha is not None:
        _judge("alpha", alpha_error(alpha, grp.K64, grp.y), alpha_error(grp.alpha32, grp.K64, grp.y), 1.0, rows)
    if mean is not None:
        m64, v64 = grp.predict64(xq)
        m32, v32 = grp.predict32(xq)
        sc = float(np.abs(m64).max())
        _judge("mean", float(np.abs(np.asarray(mean, dtype=np.float64) - m64).max()), float(np.abs(m32 - m64).max()), sc, rows)
        _judge("var", float(np.abs(np.asarray(var, dtype=np.float64) - v64).max()), float(np.abs(v32 - v64).max()), float(PRIOR32), rows)
    return rows, all(r["ok"] for r in rows.values())


class Worst:
    """Keeps, per quantity, the row that comes closest to (or furthest beyond) its limit; printed like R.format_rows, with the
    fraction of the limit it used."""

    def __init__(self):
        self.rows, self.where, self.bad = {}, {}, []

    def add(self, tag, rows):
        for k, r in rows.items():
            key = (not r["ok"], r["err"] / r["lim"] if np.isfinite(r["err"]) and r["lim"] > 0 else 1e300)
            if k not in self.rows or key > self.rows[k][0]:
                self.rows[k] = (key, r); self.where[k] = tag
            if not r["ok"]:
                self.bad.append((tag, k, r["err"], r["base"]))

    def __str__(self):
        return (format_rows({k: v[1] for k, v in self.rows.items()}) + "   of the limit: " +
                " ".join("%s %.2f" % (k, v[0][1]) for k, v in self.rows.items()) + "   at " + " ".join("%s:%s" % kv for kv in self.where.items()))


# --------------------------------------------------------------------------------------------------------------------- inputs
# The shape table of the GPU suite (tests/test_gpu_obsgp64.py); the CPU suite proves the bound on the same groups first.
PITCH = 0.006             # lattice pitch: above the 2-D margin, so that no two table entries of distinct pixels fall inside it
GRIDS_SMALL = [(ni, nj) for nj in (1, 3, 7, 8, 12, 13) for ni in range(1, 19)]
GRIDS_BIG = [(64, 48), (321, 243), (640, 480)]
GRID_NONSQUARE = (23, 9)          # pitches 0.03 x 0.008
GRID_WARPED = (17, 13)            # non-uniform, monotone pitch
N_1D = list(range(20, 46)) + [59, 60, 61, 270, 1081]
VAL0 = F32(-7.0)                  # the caller's sentinel in val: a miss leaves it


def lattice(ni, nj, pitch=(PITCH, PITCH), origin=(-0.31, -0.23), warp=0.0):
    """vu [2 ni nj] float32, interleaved: v runs with i, u with j.  warp > 0: pitch modulated by 1 + warp cos(.), still monotone."""
    i = np.arange(ni, dtype=np.float64); j = np.arange(nj, dtype=np.float64)
    v = (origin[0] + pitch[0] * (i + warp * np.sin(0.7 * i) / 0.7)).astype(F32)
    u = (origin[1] + pitch[1] * (j + warp * np.sin(0.9 * j + 1.0) / 0.9)).astype(F32)
    vu = np.empty((nj, ni, 2), dtype=F32)
    vu[:, :, 0] = v[None, :]; vu[:, :, 1] = u[:, None]
    return vu.reshape(-1)


def field2d(vu, kind="smooth"):
    """f = 1 / depth on the lattice: a smooth surface, or one with a depth step."""
    v, u = vu[0::2].astype(np.float64), vu[1::2].astype(np.float64)
    z = 1.5 + 0.4 * np.sin(3.0 * v) * np.cos(2.0 * u)
    if kind == "step":
        z = np.where(np.floor(40.0 * (v + u)) % 2 == 0, z, z + 0.8)
    return (1.0 / z).astype(F32)


def validity(name, part, f, seed=0):
    """The validity patterns: f with the invalid pixels written as 0, -1 or NaN (all invalid by f > 0)."""
    rng = np.random.default_rng(seed)
    f = f.copy()
    npx = f.size
    bad = np.zeros(npx, dtype=bool)
    if name == "all":
        pass
    elif name in ("holes10", "holes90"):
        bad = rng.random(npx) < (0.1 if name == "holes10" else 0.9)
    elif name == "tiles":                       # every pixel of a third of the tiles (their neighbours lose the shared ones)
        for g in np.flatnonzero(rng.random(part.ngroups) < 0.34):
            bad[part.pixels(g)] = True
    elif name == "one":                         # exactly one valid pixel in every tile
        def own(a0, a1):
            """Per tile a coordinate no other tile contains (tiles overlap by 3; a last tile only 3 wide lies wholly inside its
            neighbour: the two then share their one pixel)."""
            c = [a0[n] if n == 0 else min(a0[n] + 3, a1[n]) for n in range(len(a0))]
            if len(a0) > 1 and a1[-1] - a0[-1] == 2:
                c[-2] = c[-1] = a1[-1]
            return c
        ci, cj = own(part.i0, part.i1), own(part.j0, part.j1)
        bad[:] = True
        for j in cj:
            for i in ci:
                bad[j * part.ni + i] = False
    elif name == "checker":
        ind = np.arange(npx)
        bad = ((ind % part.ni) + (ind // part.ni)) % 2 == 1
    elif name in ("zero", "minus", "nan"):
        bad = rng.random(npx) < 0.3
    else:
        raise KeyError(name)
    f[bad] = {"zero": F32(0), "minus": F32(-1), "nan": F32(np.nan)}.get(name, (F32(0), F32(-1), F32(np.nan))[seed % 3])
    return f


VALIDITY = ["all", "holes10", "holes90", "tiles", "one", "checker", "zero", "minus", "nan"]


def _around(t):
    t = np.asarray(t, dtype=F32)
    return np.concatenate([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))])


def _axis_probes(tab, margin):
    """Table entries exactly and one ulp to either side; table[0] + margin and table[-1] - margin likewise."""
    margin = F32(margin)
    return np.concatenate([_around(tab), _around([tab[0] + margin, tab[-1] - margin])])


def _centres(tab):
    return ((tab[:-1].astype(np.float64) + tab[1:].astype(np.float64)) / 2).astype(F32)


def queries2d(part, vu, seed=0, margin=MARGIN2):
    """The query classes of the 2-D suite, [nq, 2] float32."""
    rng = np.random.default_rng(seed)
    px = np.asarray(vu, dtype=F32).reshape(-1, 2)
    v, u = px[:part.ni, 0], px[::part.ni, 1]
    pv = float(np.diff(v).min()) if part.ni > 1 else PITCH
    pu = float(np.diff(u).min()) if part.nj > 1 else PITCH
    out = [px]                                                                           # every lattice point exactly
    out.append(px + (rng.uniform(-1, 1, px.shape) * 1e-3 * np.array([pv, pu])).astype(F32))
    out.append(px + (rng.uniform(-1, 1, px.shape) * 0.3 * np.array([pv, pu])).astype(F32))
    out.append(px + (0.5 * np.array([pv, pu])).astype(F32))                              # pixel-cell centres
    vp, up = _axis_probes(part.vali, margin), _axis_probes(part.valj, margin)
    vc = np.concatenate([_centres(part.vali), v[:1], v[-1:]]); uc = np.concatenate([_centres(part.valj), u[:1], u[-1:]])
    for a, b in ((vp, uc), (vc, up), (vp, up)):
        out.append(np.stack(np.meshgrid(a, b, indexing="ij"), axis=-1).reshape(-1, 2))
    lo, hi = np.array([v[0], u[0]], dtype=np.float64), np.array([v[-1], u[-1]], dtype=np.float64)
    far = rng.uniform(lo - 0.2, hi + 0.2, (64, 2))
    out.append(far[np.any((far < lo) | (far > hi), axis=1)].astype(F32))                 # outside the grid
    sp = np.array([np.inf, -np.inf, np.nan], dtype=F32)
    out.append(np.stack(np.meshgrid(sp, np.concatenate([uc, sp]), indexing="ij"), axis=-1).reshape(-1, 2))
    out.append(np.stack(np.meshgrid(vc, sp, indexing="ij"), axis=-1).reshape(-1, 2))
    return np.ascontiguousarray(np.concatenate(out), dtype=F32)


def scan(N, pitch=0.00436, warp=0.0):
    i = np.arange(N, dtype=np.float64)
    return (-0.5 * pitch * (N - 1) + pitch * (i + warp * np.sin(0.37 * i) / 0.37)).astype(F32)


def field1d(theta, kind="smooth"):
    t = theta.astype(np.float64)
    r = 3.0 + 1.2 * np.sin(2.5 * t + 0.3)
    if kind == "step":
        r = np.where(np.floor(25.0 * t) % 2 == 0, r, r + 1.5)
    return (1.0 / np.sqrt(r)).astype(F32)


def queries1d(part, theta, seed=0, margin=MARGIN1):
    rng = np.random.default_rng(seed)
    th = np.asarray(theta, dtype=F32)
    p = float(np.diff(th).min())
    out = [th, th + (rng.uniform(-1, 1, th.size) * 1e-3 * p).astype(F32), th + (rng.uniform(-1, 1, th.size) * 0.3 * p).astype(F32),
           th + F32(0.5 * p), _axis_probes(part.range, margin), _centres(part.range),
           rng.uniform(th[0] - 0.1, th[0], 8).astype(F32), rng.uniform(th[-1], th[-1] + 0.1, 8).astype(F32),
           np.array([np.inf, -np.inf, np.nan], dtype=F32)]
    return np.ascontiguousarray(np.concatenate(out), dtype=F32)


def assessed_groups(ngroups, ng0, limit=600, seed=5):
    """The groups whose accuracy is assessed: all of them up to `limit`; above it the four corners, a seeded draw from the last
    row and the last column of tiles, and a seeded draw from the rest (the float64 work per group is 64 x 64)."""
    if ngroups <= limit:
        return np.arange(ngroups)
    rng = np.random.default_rng(seed)
    ng1 = ngroups // ng0
    last_row = (ng1 - 1) * ng0 + np.arange(ng0); last_col = np.arange(ng1) * ng0 + ng0 - 1
    pick = [np.array([0, ng0 - 1, (ng1 - 1) * ng0, ngroups - 1, (ng1 - 2) * ng0 + ng0 - 2]),
            rng.choice(last_row, 24, replace=False), rng.choice(last_col, 24, replace=False), rng.choice(ngroups, 200, replace=False)]
    return np.unique(np.concatenate(pick))


def assess_answers(groups, gref, q, val, var, which, worst, tag, model=None):
    """Holds the answers (val, var) of the queries q that the reference lookup (gref) routes to the groups `which` to the bound,
    and -- with model(g) -> (L, alpha) -- the factor and alpha of those groups.  groups[g] -> Group or None.  Answers to queries
    with a NaN coordinate are compared with the float64 reference under equal_nan.  Returns the groups that had answers."""
    q = np.asarray(q, dtype=F32).reshape(len(gref), -1)
    nanq = np.isnan(q).any(axis=1)
    order = np.argsort(gref, kind="stable")
    bounds = np.searchsorted(gref[order], np.arange(len(groups) + 1))
    answered = []
    for g in which:
        grp = groups[g]
        sel = order[bounds[g]:bounds[g + 1]]
        if grp is None:
            assert sel.size == 0, (tag, g)
            continue
        fin = sel[~nanq[sel]]
        kw = {}
        if model is not None:
            L, alpha = model(g)
            kw.update(L=L, alpha=alpha)
        if fin.size:
            kw.update(xq=q[fin], mean=val[fin], var=var[fin])
            answered.append(g)
        if kw:
            rows, ok = assess(grp, **kw)
            worst.add("%s/g%d(n=%d)" % (tag, g, grp.n), rows)
        nn = sel[nanq[sel]]
        if nn.size:
            m64, v64 = grp.predict64(q[nn])
            np.testing.assert_allclose(val[nn], m64, rtol=1e-5, equal_nan=True)
            np.testing.assert_allclose(var[nn], v64, rtol=1e-5, equal_nan=True)
    return answered
