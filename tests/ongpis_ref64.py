"""Float64 reference of OnGPIS cluster training and prediction, and the accuracy bound the kernels are held to.

Test infrastructure only.  A vectorised restatement of oracle/arbiter64.py (the gather rule, the Matern-3/2 kernel matrix with
its first-derivative blocks, the 2-D sqrt(sigx sigg) diagonal, train and predict) that is fast enough for the largest cluster
training accepts (K = 16384), plus a plain float32 LAPACK pipeline (numpy float32 build, spotrf, strtrs) as the baseline.

The bound: for every measured quantity, error(candidate) <= RATIO * error(float32 pipeline) + FLOOR_ULP ulp of the quantity's
scale, both errors taken against float64 on the same operands.  RATIO = 8 throughout, except for what is computed from the factor
(the factor, alpha, and the predictions from it: K4 reads an inverse made of the same chains) of clusters with more than VO_ROWS
value-only points: chain_ratio.
Quantities:
  build     max |K - K64|_ij / sqrt(K64_ii K64_jj)
  factor    backward error max |L L^T - K|_ij / sqrt(K_ii K_jj) on the matrix L factors
  alpha     residual |K alpha - y|_inf / (|K| |alpha| + |y|)_inf on the same matrix
  f, grad   max over queries (and components) of |mean - mean64|, scale max |mean64|
  var_f     max over queries of |var - var64|, scale the prior
  var_g     the same for the gradient variances divided by 3 / s^2
Both scaled measures are invariant to the diagonal scaling of K (the value rows are O(1), the gradient rows O(3 / s^2)), so a
defect in the value block is not hidden under the size of the gradient block."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

RATIO = 8.0
FLOOR_ULP = 4.0
VO_ROWS = 2400       # value-only rows above which everything computed from the factor gets more room: chain_ratio
ULP = 2.0 ** -23
ROWS = 2048          # row block of the float64 products (bounds their temporaries at K = 16384)


def gather(pos, grad, val, sx, sg):
    """The training rule of OnGPIS::train: a point is value-only (sigx = 2, no gradient rows) when its gradient noise exceeds
    0.1001 or its gradient is zero.  Returns (gidx, sigx, sigg, y) in float64; y is ordered [f; d/dx; d/dy; (d/dz)]."""
    pos = np.asarray(pos); grad = np.asarray(grad, dtype=np.float64)
    N, dim = pos.shape
    sg32 = np.asarray(sg, dtype=np.float32)
    vo = (sg32.astype(np.float64) > 0.1001) | np.all(np.abs(grad) < 1e-6, axis=1)
    gidx = np.full(N, -1, dtype=np.int64)
    gidx[~vo] = np.arange(int((~vo).sum()))
    sigx = np.asarray(sx, dtype=np.float64).copy()
    sigx[vo] = 2.0
    y = np.concatenate([np.asarray(val, dtype=np.float64)] + [grad[~vo, c] for c in range(dim)])
    return gidx, sigx, np.asarray(sg, dtype=np.float64), y


def _a(scale, dt):
    return np.sqrt(dt(3.0)) / dt(scale)


def kernel_matrix(x, gidx, scale, sigx, sigg, dtype=np.float64, quirk2d=True):
    """Full symmetric Matern-3/2 kernel matrix in arithmetic `dtype`; rows [f; d/dx; d/dy; (d/dz)] as arbiter64.matern_train_K."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    N, dim = x.shape
    gp = np.flatnonzero(np.asarray(gidx) >= 0)
    gp = gp[np.argsort(np.asarray(gidx)[gp])]
    ng = gp.size
    K = N + dim * ng
    a = _a(scale, dt)
    M = np.empty((K, K), dtype=dt)
    D = x[:, None, :] - x[None, :, :]                    # D[k, j] = x_k - x_j
    r = np.sqrt(np.einsum("kjc,kjc->kj", D, D))
    e = np.exp(-a * r)
    M[:N, :N] = (1 + a * r) * e
    M[np.arange(N), np.arange(N)] = dt(1) + np.asarray(sigx).astype(dt)
    if ng:
        a2 = a * a
        Dg = D[gp]                                        # [ng, N, dim]
        eg = e[gp]
        for c in range(dim):
            blk = -a2 * Dg[:, :, c] * eg
            M[N + c * ng:N + (c + 1) * ng, :N] = blk
            M[:N, N + c * ng:N + (c + 1) * ng] = blk.T
        del Dg
        Dgg = D[np.ix_(gp, gp)]                           # [ng, ng, dim]
        rg = r[np.ix_(gp, gp)]
        with np.errstate(divide="ignore"):
            rinv = np.where(rg > 0, dt(1) / rg, dt(0))
        egg = e[np.ix_(gp, gp)]
        del D, r, e
        sg_ = np.asarray(sigg).astype(dt)[gp]
        for c1 in range(dim):
            for c2 in range(dim):
                blk = a2 * ((dt(1) if c1 == c2 else dt(0)) - a * Dgg[:, :, c1] * Dgg[:, :, c2] * rinv) * egg
                if c1 == c2:
                    blk[np.arange(ng), np.arange(ng)] = a2 + sg_
                    if dim == 2 and c1 == 0 and quirk2d:      # covFnc.cpp:352
                        blk[np.arange(ng), np.arange(ng)] = a2 + np.sqrt(np.asarray(sigx).astype(dt)[gp] * sg_)
                M[N + c1 * ng:N + (c1 + 1) * ng, N + c2 * ng:N + (c2 + 1) * ng] = blk
    return M


def cross(x, gidx, scale, xq, dtype=np.float64):
    """k* of every query: [K, Q, 1 + dim] (column 0 the value, 1 + c the derivative by query coordinate c, as arbiter64)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt); xq = np.asarray(xq).astype(dt)
    N, dim = x.shape
    gp = np.flatnonzero(np.asarray(gidx) >= 0)
    gp = gp[np.argsort(np.asarray(gidx)[gp])]
    ng = gp.size
    a = _a(scale, dt)
    a2 = a * a
    D = x[:, None, :] - xq[None, :, :]                   # [N, Q, dim]
    r = np.sqrt(np.einsum("kqc,kqc->kq", D, D))
    e = np.exp(-a * r)
    out = np.empty((N + dim * ng, xq.shape[0], 1 + dim), dtype=dt)
    out[:N, :, 0] = (1 + a * r) * e
    out[:N, :, 1:] = a2 * D * e[:, :, None]
    Dg, rg, eg = D[gp], r[gp], e[gp]
    for c1 in range(dim):
        rows = slice(N + c1 * ng, N + (c1 + 1) * ng)
        out[rows, :, 0] = -a2 * Dg[:, :, c1] * eg
        for c2 in range(dim):
            out[rows, :, 1 + c2] = a2 * ((dt(1) if c1 == c2 else dt(0)) - a * Dg[:, :, c1] * Dg[:, :, c2] / rg) * eg
    return out


def prior(dim, scale, dtype=np.float64):
    dt = np.dtype(dtype).type
    tos = dt(3) / (dt(scale) * dt(scale))
    return np.array([1.001] + [tos + dt(0.001)] * 3, dtype=dt) if dim == 3 else np.array([1.01] + [tos + dt(0.1)] * 2, dtype=dt)


def predict(L, alpha, ks, dim, scale, dtype=np.float64):
    """mean, var [Q, 1 + dim] from factor L (lower), alpha and k* [K, Q, 1 + dim], all in arithmetic `dtype`."""
    dt = np.dtype(dtype)
    K, Q, nc = ks.shape
    B = ks.reshape(K, Q * nc).astype(dt, copy=False)
    mean = (B.T @ np.asarray(alpha).astype(dt)).reshape(Q, nc)
    V = solve_triangular(np.asarray(L).astype(dt, copy=False), B, lower=True, check_finite=False)
    var = prior(dim, scale, dt)[None, :] - np.einsum("kq,kq->q", V, V).reshape(Q, nc)
    return mean, var


def chol(K, dtype):
    """Cholesky factor of K in `dtype` (LAPACK potrf), strict upper triangle zero."""
    return cholesky(np.asarray(K, dtype=dtype), lower=True, check_finite=False, overwrite_a=True)


def solve_alpha(L, y, dtype):
    L = np.asarray(L, dtype=dtype)
    z = solve_triangular(L, np.asarray(y, dtype=dtype), lower=True, check_finite=False)
    return solve_triangular(L, z, lower=True, trans="T", check_finite=False)


def train(pos, grad, val, sx, sg, scale, dtype=np.float64):
    """OnGPIS training in arithmetic `dtype` (float64: the reference; float32: the LAPACK baseline): dict(gidx, K, L, alpha)."""
    gidx, sigx, sigg, y = gather(pos, grad, val, sx, sg)
    if np.dtype(dtype) == np.float64:
        M = kernel_matrix(np.asarray(pos, dtype=np.float32), gidx, scale, sigx, sigg, np.float64)
    else:
        M = kernel_matrix(np.asarray(pos, dtype=np.float32), gidx, scale, sigx.astype(np.float32), np.asarray(sg, dtype=np.float32), np.float32)
    L = chol(M, dtype)
    return dict(gidx=gidx, K=y.size, L=L, alpha=solve_alpha(L, y, dtype))


def queries(rng, pos, scale, n_each=6):
    """Queries of every regime of the cross-covariance: 0.3 s and 1e-3 s from training points (the latter: the 1 / r terms of
    the derivative blocks), 1 s from them, and 65 s beyond the patch's radius, where a r > 112 for every training point and
    float32 exp underflows to 0."""
    n, dim = pos.shape
    out = [pos[rng.integers(0, n, n_each)] + rng.normal(0, f * scale, (n_each, dim)) for f in (0.3, 1e-3)]
    u = rng.normal(size=(n_each, dim)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    out.append(pos[rng.integers(0, n, n_each)] + scale * u)
    u = rng.normal(size=(n_each, dim)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = pos.mean(axis=0)
    out.append(c + (np.linalg.norm(pos - c, axis=1).max() + 65 * scale) * u)
    return np.concatenate(out).astype(np.float32)


def row_group_points(gidx, K, rows=1024):
    """For each group of `rows` rows of K (K4 streams a large cluster's factor in row groups of 32 block rows): the training point
    that owns the group's middle row."""
    gidx = np.asarray(gidx)
    N = gidx.size
    ng = int((gidx >= 0).sum())
    owner = np.empty(max(ng, 1), dtype=np.int64)
    owner[gidx[gidx >= 0]] = np.flatnonzero(gidx >= 0)
    return np.array([r if r < N else owner[(r - N) % ng] for r in (min(r0 + rows // 2, K - 1) for r0 in range(0, K, rows))])


def row_group_queries(rng, pos, gidx, K, scale, rows=1024):
    """One query 0.3 s from the owner of each row group (row_group_points): that point's k* row in the group is large, so a
    defect confined to one row group reaches the mean, not only the variance."""
    pts = row_group_points(gidx, K, rows)
    return (pos[pts] + rng.normal(0, 0.3 * scale, (pts.size, pos.shape[1]))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- measures
def _sym64(Klow):
    """Symmetric float64 matrix from one whose lower triangle holds K (the kernels' layout)."""
    K = np.tril(np.asarray(Klow, dtype=np.float64))
    K += np.tril(K, -1).T
    return K


def build_error(Kc, K64):
    """max over the lower triangle of |Kc - K64|_ij / sqrt(K64_ii K64_jj)."""
    s = 1.0 / np.sqrt(np.diag(K64))
    worst = 0.0
    for i0 in range(0, K64.shape[0], ROWS):
        i1 = min(i0 + ROWS, K64.shape[0])
        d = np.abs(np.asarray(Kc[i0:i1, :i1], dtype=np.float64) - K64[i0:i1, :i1]) * s[i0:i1, None] * s[None, :i1]
        worst = max(worst, float(np.tril(d, i0).max()))
    return worst


def backward_error(L, K64):
    """max |L L^T - K|_ij / sqrt(K_ii K_jj) over the lower triangle; L's strict upper triangle is ignored."""
    n = K64.shape[0]
    s = 1.0 / np.sqrt(np.diag(K64))
    L64 = np.tril(np.asarray(L[:n, :n], dtype=np.float64))
    worst = 0.0
    for i0 in range(0, n, ROWS):
        i1 = min(i0 + ROWS, n)
        d = np.abs(L64[i0:i1, :i1] @ L64[:i1, :i1].T - K64[i0:i1, :i1]) * s[i0:i1, None] * s[None, :i1]
        worst = max(worst, float(np.tril(d, i0).max()))
        del d
    return worst


def alpha_residual(alpha, K64, y):
    al = np.asarray(alpha, dtype=np.float64)
    return float(np.abs(K64 @ al - y).max() / (np.abs(K64) @ np.abs(al) + np.abs(y)).max())


def pred_errors(mean, var, mean64, var64, dim, scale):
    """Per column group: {name: (error, scale)}."""
    tos = 3.0 / (float(scale) ** 2)
    pr = prior(dim, scale)
    return dict(
        f=(float(np.abs(mean[:, 0] - mean64[:, 0]).max()), float(np.abs(mean64[:, 0]).max())),
        grad=(float(np.abs(mean[:, 1:] - mean64[:, 1:]).max()), float(np.abs(mean64[:, 1:]).max())),
        var_f=(float(np.abs(var[:, 0] - var64[:, 0]).max()), float(pr[0])),
        var_g=(float(np.abs(var[:, 1:] - var64[:, 1:]).max()) / tos, float(pr[1]) / tos))


def chain_ratio(n_value_only):
    """Ratio for the factor's backward error, alpha's residual and the predictions: RATIO, growing in proportion to the
    number of value-only points above VO_ROWS of them.  The kernels accumulate every element of L as ONE fmaf chain in a fixed order,
    LAPACK's blocked spotrf in another.  Where the value-only block is large (every off-diagonal entry O(1), thousands of comparable
    terms per chain) the gap grows with K; the oracle's `tiled` order (which the GPU reproduces bit for bit), value-only clusters at
    a 300-point cluster's density, factor / alpha ratios:
        K = 1200: 5.1 / 2.5    2400: 7.4 / 5.3    3600: 9.2 / 4.9    5000: 9.4 / 7.3    7256 (GPU, the same digits): 8.3 / 9.9
    and end to end at K = 3600 f 9.7 (5.5 from its own factor); at K = 7256 the gradient from its own factor 11.3 (GPU and `tiled`
    alike: 1.79e-5 against LAPACK's 1.58e-6), 16.0 end to end.  Alpha grows about linearly, 1.4 x per 1000 value-only rows: the
    allowance, 8 x per 2400, keeps twice that.  Clusters with normals stay at 8 up to K = 16384 (factor 5.9, alpha 6.4 measured there).
    A dropped or stale tile costs orders of magnitude, not these factors."""
    return RATIO * max(1.0, n_value_only / VO_ROWS)


def _judge(name, err, base, scale, rows, ratio=RATIO):
    lim = ratio * base + FLOOR_ULP * ULP * scale
    ratio = err / base if base > 0 else (0.0 if err == 0 else np.inf)
    rows[name] = dict(err=err, base=base, ratio=ratio, ok=bool(np.isfinite(err) and err <= lim))


# ---------------------------------------------------------------------------------------------------------------- the checker
class Problem:
    """One cluster and its queries, with the float64 and float32-pipeline quantities computed once."""

    def __init__(self, dim, scale, pos, grad, val, sx, sg, xq):
        self.dim = dim
        self.scale = float(np.float32(scale))                # the kernels see float32 operands: so does the reference
        self.pos = np.asarray(pos, dtype=np.float32); self.grad = np.asarray(grad, dtype=np.float32)
        self.val = np.asarray(val, dtype=np.float32); self.sx = np.asarray(sx, dtype=np.float32)
        self.sg = np.asarray(sg, dtype=np.float32); self.xq = np.asarray(xq, dtype=np.float32)
        self.gidx, self.sigx, self.sigg, self.y = gather(self.pos, self.grad, self.val, self.sx, self.sg)
        self.K = self.y.size
        self.n_value_only = int((self.gidx < 0).sum())
        self._ks64 = self._ks32 = self._e2e = None

    def K64(self):
        return kernel_matrix(self.pos, self.gidx, self.scale, self.sigx, self.sigg, np.float64)

    def K32(self):
        return kernel_matrix(self.pos, self.gidx, self.scale, self.sigx.astype(np.float32), self.sg, np.float32)

    def ks64(self):
        if self._ks64 is None:
            self._ks64 = cross(self.pos, self.gidx, self.scale, self.xq, np.float64)
        return self._ks64

    def ks32(self):
        if self._ks32 is None:
            self._ks32 = cross(self.pos, self.gidx, self.scale, self.xq, np.float32)
        return self._ks32

    def end_to_end(self):
        """(mean64, var64, mean32, var32): the float64 pipeline and the float32 LAPACK pipeline, from the inputs."""
        if self._e2e is None:
            t = train(self.pos, self.grad, self.val, self.sx, self.sg, self.scale, np.float64)
            m64, v64 = predict(t["L"], t["alpha"], self.ks64(), self.dim, self.scale, np.float64)
            del t
            t = train(self.pos, self.grad, self.val, self.sx, self.sg, self.scale, np.float32)
            m32, v32 = predict(t["L"], t["alpha"], self.ks32(), self.dim, self.scale, np.float32)
            del t
            self._e2e = (m64, v64, m32, v32)
        return self._e2e


def assess(p, Kmat=None, L=None, alpha=None, mean=None, var=None):
    """Holds what a candidate (the GPU, or the oracle) computed for Problem `p` to the bound.
      Kmat         its kernel matrix (lower triangle)                       -> "build"
      L, alpha     its factor (lower) and alpha, on its own matrix Kmat     -> "factor", "alpha"
      mean, var    its predictions [Q, 1 + dim] at p.xq                      -> end to end: "f", "grad", "var_f", "var_g";
                   with L and alpha also from its own L / alpha: "own_f", ...
    Returns (rows, ok): rows[name] = dict(err, base, ratio, ok)."""
    rows = {}
    if Kmat is not None:
        K64 = p.K64()
        _judge("build", build_error(Kmat, K64), build_error(p.K32(), K64), 1.0, rows)
        del K64
    if L is not None or alpha is not None:
        Kown = _sym64(Kmat)
        Lb = chol(Kown.astype(np.float32), np.float32)
        if L is not None:
            _judge("factor", backward_error(L, Kown), backward_error(Lb, Kown), 1.0, rows, chain_ratio(p.n_value_only))
        if alpha is not None:
            ab = solve_alpha(Lb, p.y.astype(np.float32), np.float32)
            _judge("alpha", alpha_residual(alpha, Kown, p.y), alpha_residual(ab, Kown, p.y), 1.0, rows, chain_ratio(p.n_value_only))
        del Kown, Lb
    if mean is not None:
        if L is not None and alpha is not None:
            Lk = np.tril(np.asarray(L[:p.K, :p.K]))
            m64, v64 = predict(Lk, alpha, p.ks64(), p.dim, p.scale, np.float64)
            m32, v32 = predict(Lk.astype(np.float32), np.asarray(alpha, dtype=np.float32), p.ks32(), p.dim, p.scale, np.float32)
            del Lk
            e, b = pred_errors(mean, var, m64, v64, p.dim, p.scale), pred_errors(m32, v32, m64, v64, p.dim, p.scale)
            for k in e:
                _judge("own_" + k, e[k][0], b[k][0], e[k][1], rows, chain_ratio(p.n_value_only))
        m64, v64, m32, v32 = p.end_to_end()
        e, b = pred_errors(mean, var, m64, v64, p.dim, p.scale), pred_errors(m32, v32, m64, v64, p.dim, p.scale)
        for k in e:
            _judge(k, e[k][0], b[k][0], e[k][1], rows, chain_ratio(p.n_value_only))      # inherits the factor's chains
    return rows, all(r["ok"] for r in rows.values())


def format_rows(rows):
    return "  ".join("%s %.2f%s" % (k, r["ratio"], "" if r["ok"] else "(FAIL %.2e vs %.2e)" % (r["err"], r["base"])) for k, r in rows.items())
