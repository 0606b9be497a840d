"""The objective the trajectory smoothers descend, in float64, written from DESIGN.md §7e (the sampler), §7i (the point
smoother), §7r (the body rule) and §7t (the body smoother) and from nothing else: it imports no reference of the smoothers, of the
footprint or of the field, so an error it shares with them has to be made twice.  Everything is vectorised over a batch of
trajectories x [m, N, dim]; a field is (dist, shape, origin, step) with dist the float32 lattice values, x fastest; a footprint is
a dict with b [balls, dim] and rho [balls]; opts is a dict with clearance, margin, w_smooth, w_obs (and sub for evaluate).

The gradient is taken by central differences, never by a formula: what is compared with the smoothers' step is the derivative of
the cost itself."""
import itertools

import numpy as np

F64 = np.float64
COST_VARIANTS = ("band_double", "inside_flat")


def interp(dist, shape, origin, step, p):
    """The bilinear / trilinear interpolant of the lattice values (cast to float64) at p [..., dim]: the cell of axis a is
    i0 = min(floor(u), n - 2) with u = (p - origin) / step; NaN outside 0 <= u <= n - 1."""
    shape = tuple(int(v) for v in shape)
    dim = len(shape)
    F = np.asarray(dist).ravel().astype(F64)
    n = np.asarray(shape, np.int64)
    u = (np.asarray(p, F64) - np.asarray(origin, F64)[:dim]) / float(step)
    with np.errstate(invalid="ignore"):
        ok = np.all((u >= 0) & (u <= (n - 1)), axis=-1)
    u = np.where(ok[..., None], u, 0.0)
    i0 = np.minimum(np.floor(u).astype(np.int64), n - 2)
    w = u - i0
    stride = np.cumprod((1,) + shape[:-1]).astype(np.int64)
    base = (i0 * stride).sum(axis=-1)
    val = np.zeros(u.shape[:-1], F64)
    for corner in itertools.product((0, 1), repeat=dim):
        wt = np.ones(u.shape[:-1], F64)
        for a in range(dim):
            wt = wt * (w[..., a] if corner[a] else 1.0 - w[..., a])
        val = val + wt * F[base + sum(corner[a] * int(stride[a]) for a in range(dim))]
    return np.where(ok, val, np.nan)


def point_cost(e, margin, variant=None):
    """0 for e >= margin, (e - margin)^2 / (2 margin) for 0 <= e < margin, margin / 2 - e inside.  variant: one of
    COST_VARIANTS, a cost that is not the contract's (u^2 / margin in the band; no slope inside)."""
    e = np.asarray(e, F64)
    mg = float(margin)
    u = e - mg
    band = u * u / (mg if variant == "band_double" else 2.0 * mg)
    inside = 0.5 * mg - (0.0 if variant == "inside_flat" else e)
    return np.where(e >= mg, 0.0, np.where(e >= 0, band, inside))


def _smooth_terms(x, opts):
    """[m, N]: 1/2 w_smooth |x_{k+1} - x_k|^2 at k, 0 at N - 1."""
    v = x[:, 1:] - x[:, :-1]
    out = np.zeros(x.shape[:2], F64)
    out[:, :-1] = 0.5 * float(opts["w_smooth"]) * (v * v).sum(axis=-1)
    return out


def ball_points(x, body):
    """[m, N, balls, dim]: w_ij = x_i + R(c_i, s_i) b_j with (c_i, s_i) the unit chord x_{k+1} - x_k, k = min(i, N - 2), about
    z only; b_z is added unrotated."""
    x = np.asarray(x, F64)
    m, N, dim = x.shape
    b = np.asarray(body["b"], F64).reshape(-1, dim)
    k = np.minimum(np.arange(N), N - 2)
    e = x[:, k + 1, :2] - x[:, k, :2]
    nn = np.sqrt((e * e).sum(axis=-1))
    c, s = (e[..., 0] / nn)[..., None], (e[..., 1] / nn)[..., None]
    w = np.empty((m, N, b.shape[0], dim), F64)
    w[..., 0] = x[:, :, None, 0] + (c * b[:, 0] - s * b[:, 1])
    w[..., 1] = x[:, :, None, 1] + (s * b[:, 0] + c * b[:, 1])
    if dim == 3:
        w[..., 2] = x[:, :, None, 2] + b[:, 2]
    return w


def point_excess(x, field, opts):
    """e [m, N] = d(x_i) - clearance."""
    return interp(*field, np.asarray(x, F64)) - float(opts["clearance"])


def body_excess(x, field, body, opts):
    """e [m, N, balls] = d(w_ij) - rho_j - clearance."""
    return interp(*field, ball_points(x, body)) - np.asarray(body["rho"], F64) - float(opts["clearance"])


def J_point(x, field, opts, terms=False, cost=None):
    """1/2 w_smooth sum_k |x_{k+1} - x_k|^2 + w_obs sum_{interior i} c(d(x_i) - clearance), [m].  terms: the summands [m, N],
    the chord k and the waypoint i at their own index, so that x_i enters the terms i - 1 and i only."""
    x = np.asarray(x, F64)
    t = _smooth_terms(x, opts)
    c = point_cost(point_excess(x, field, opts), opts["margin"], cost)
    t[:, 1:-1] += float(opts["w_obs"]) * c[:, 1:-1]
    return t if terms else t.sum(axis=1)


def J_body(x, field, body, opts, ends=True, terms=False, cost=None):
    """The same smoothness term plus w_obs sum_i sum_j c(d(w_ij) - rho_j - clearance); i runs over all N waypoints when `ends`
    and over the interior ones otherwise.  terms: as J_point; x_i enters the terms i - 1, i and, through the last chord,
    N - 1 when i = N - 2."""
    x = np.asarray(x, F64)
    t = _smooth_terms(x, opts)
    c = point_cost(body_excess(x, field, body, opts), opts["margin"], cost).sum(axis=-1)
    if ends:
        t += float(opts["w_obs"]) * c
    else:
        t[:, 1:-1] += float(opts["w_obs"]) * c[:, 1:-1]
    return t if terms else t.sum(axis=1)


def perturbations(x, h):
    """(idx, a, x+, x-): the interior waypoints idx = 1 + r, 4 + r, ... moved by +-h in coordinate a, for r < 3 and every a."""
    x = np.asarray(x, F64)
    N, dim = x.shape[1:]
    for r in range(3):
        idx = np.arange(1 + r, N - 1, 3)
        if idx.size == 0:
            continue
        for a in range(dim):
            xp, xm = x.copy(), x.copy()
            xp[:, idx, a] += h
            xm[:, idx, a] -= h
            yield idx, a, xp, xm


def fd_gradient(J, x, h, local=True):
    """g [m, N - 2, dim]: central differences of J in every interior coordinate.  local: J(x, terms=True) gives the summands
    [m, N]; moving x_i changes the summands i - 1, i and i + 1 at most, so every third waypoint moves at once and 6 * dim
    evaluations serve any N.  Otherwise J(x) gives [m] and every coordinate is a batch member of its own."""
    x = np.asarray(x, F64)
    m, N, dim = x.shape
    g = np.zeros((m, N - 2, dim), F64)
    if local:
        for idx, a, xp, xm in perturbations(x, h):
            D = J(xp, terms=True) - J(xm, terms=True)
            g[:, idx - 1, a] = (D[:, idx - 1] + D[:, idx] + D[:, idx + 1]) / (2.0 * h)
        return g
    for i in range(1, N - 1):
        for a in range(dim):
            xp, xm = x.copy(), x.copy()
            xp[:, i, a] += h
            xm[:, i, a] -= h
            g[:, i - 1, a] = (J(xp) - J(xm)) / (2.0 * h)
    return g


def _metric(n):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def solve_metric(g):
    """inverse(tridiag(-1, 2, -1)) g over the waypoint axis of g [m, n, dim], by a float64 solve."""
    g = np.asarray(g, F64)
    m, n, dim = g.shape
    return np.linalg.solve(_metric(n), g.transpose(1, 0, 2).reshape(n, m * dim)).reshape(n, m, dim).transpose(1, 0, 2)


def recover(x0, x1, kappa):
    """(delta, g) [m, N - 2, dim] of a step x1 = x0 - kappa delta: delta = (x0 - x1) / kappa at the interior waypoints and
    g = tridiag(-1, 2, -1) delta, in float64."""
    d = (np.asarray(x0, F64) - np.asarray(x1, F64))[:, 1:-1] / float(kappa)
    return d, np.einsum("ij,mjk->mik", _metric(d.shape[1]), d)


def descend(J, x, kappa, h):
    """One step in float64: x with its interior waypoints moved by -kappa solve_metric(fd_gradient(J))."""
    x1 = np.asarray(x, F64).copy()
    x1[:, 1:-1] -= float(kappa) * solve_metric(fd_gradient(J, x1, h))
    return x1


def _face_margin(field, p):
    """The least distance, in lattice steps, of the points p [..., dim] from a cell face; -1 if one is off the lattice."""
    _, shape, origin, step = field
    dim = len(shape)
    u = (np.asarray(p, F64) - np.asarray(origin, F64)[:dim]) / float(step)
    if not np.all((u >= 0) & (u <= np.asarray(shape) - 1)):
        return -1.0
    f = u - np.floor(u)
    return float(np.minimum(f, 1.0 - f).min())


def margins(x, field, body, h):
    """(face, chord): the least distance, in lattice steps, of any sampled point from a cell face, and the least chord length
    (of the first two components when there is a body: what the heading divides by).  Sampled points are the waypoints and, with
    a body, its balls, at x and at every x +- h that fd_gradient visits."""
    x = np.asarray(x, F64)
    face, chord = np.inf, np.inf
    for xs in itertools.chain([x], *[(xp, xm) for _, _, xp, xm in perturbations(x, h)]):
        face = min(face, _face_margin(field, xs))
        v = xs[:, 1:] - xs[:, :-1]
        if body is not None:
            face = min(face, _face_margin(field, ball_points(xs, body)))
            v = v[..., :2]
        chord = min(chord, float(np.sqrt((v * v).sum(axis=-1)).min()))
    return face, chord


def evaluate(x, field, opts, body=None):
    """dict(length, smooth, obstacle, min_dist) [m] of §7i's evaluation in float64: the sum of the chords' lengths, of their
    squares, of the point cost at the interior waypoints (with a body: at the balls of the interior waypoints), and the least
    interpolated distance over the waypoints and `sub` equally spaced points inside every chord."""
    x = np.asarray(x, F64)
    v = x[:, 1:] - x[:, :-1]
    sq = (v * v).sum(axis=-1)
    if body is None:
        c = point_cost(point_excess(x, field, opts), opts["margin"])
    else:
        c = point_cost(body_excess(x, field, body, opts), opts["margin"]).sum(axis=-1)
    sub = int(opts["sub"])
    d = [interp(*field, x)] + [interp(*field, x[:, :-1] + (s / (sub + 1.0)) * v) for s in range(1, sub + 1)]
    return dict(length=np.sqrt(sq).sum(axis=1), smooth=sq.sum(axis=1), obstacle=c[:, 1:-1].sum(axis=1),
                min_dist=np.concatenate(d, axis=1).min(axis=1))


__all__ = ["interp", "point_cost", "ball_points", "point_excess", "body_excess", "J_point", "J_body", "perturbations", "fd_gradient",
           "solve_metric", "recover", "descend", "margins", "evaluate", "COST_VARIANTS"]
