"""Inputs and tolerances shared by tests/test_traj_grad64.py (the references against the float64 objective, CPU) and
tests/test_gpu_traj_grad64.py (the device against it): two small analytic scenes, the footprints, trajectories built so that no
sampled point lies near a cell face, the populations the comparisons need, and the table of floors the tolerances come from."""
import functools

import numpy as np

import body_ref
import traj_obj64 as obj

F32 = np.float32
F64 = np.float64
NS = (3, 4, 5, 63, 64, 65, 66, 128, 129, 256)
M = 8
BATCH = "batch"                  # the key of the extra batch: BATCH_M trajectories of BATCH_N waypoints
BATCH_M, BATCH_N = 300, 5
H = 1e-6                         # the finite-difference step, world units
FACE = 0.05                      # every sampled point keeps this many lattice steps from a cell face
CLEARANCE = 0.1
TWO_STEP_NS = (5, 65)            # test_two_steps_compose: one wavefront and two
TWO_STEP_RATE = 2.0 ** -6
SMOOTHERS = ("point", "body")


# ---- scenes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(dim):
    """dict(f, shape, origin, step, centre): f the analytic signed distance of two discs (40 x 30) or one ball (24 x 20 x 16) on
    a lattice of step 0.25 at origin 0, float32, x fastest; centre: the obstacle the trajectories pass."""
    step = 0.25
    if dim == 2:
        shape = (40, 30)
        X, Y = np.meshgrid(np.arange(shape[0]) * step, np.arange(shape[1]) * step)
        f = np.minimum(np.hypot(X - 5.0, Y - 3.5) - 1.0, np.hypot(X - 2.5, Y - 5.0) - 0.6)
        centre = (5.0, 3.5)
    else:
        shape = (24, 20, 16)
        Z, Y, X = np.meshgrid(np.arange(shape[2]) * step, np.arange(shape[1]) * step, np.arange(shape[0]) * step, indexing="ij")
        f = np.sqrt((X - 2.9) ** 2 + (Y - 2.4) ** 2 + (Z - 1.9) ** 2) - 0.8
        centre = (2.9, 2.4, 1.9)
    return dict(f=np.ascontiguousarray(f, F32).ravel(), shape=shape, origin=(0.0,) * dim, step=F32(step), centre=centre)


@functools.lru_cache(maxsize=None)
def footprint(dim):
    """2-D: three discs covering a 0.6 x 0.3 rectangle; 3-D: three balls, one of them off the plane (b_z != 0)."""
    if dim == 2:
        return body_ref.box(0.6, 0.3, 3)
    return body_ref.make(3, [[0.25, 0.0, 0.0], [-0.25, 0.05, 0.0], [0.0, 0.0, 0.15]], [0.15, 0.15, 0.1])


def opts(dim, step, balls=None, **kw):
    """The documented defaults (§7i; with `balls`, §7t's w_obs = 0.25 step / balls) as float32 values, with the options of these
    tests: one unclipped step of rate 1, clearance 0.1."""
    s = F32(step)
    wo = F32(0.25) * s
    o = dict(clearance=F32(CLEARANCE), margin=F32(3) * s, w_smooth=F32(1), w_obs=wo if balls is None else wo / F32(balls),
             rate=F32(1), max_move=F32(1e30), tol=F32(0), iters=1, sub=3)
    o.update(kw)
    return o


CALL = ("clearance", "rate", "max_move", "tol", "iters")     # what a call passes; the rest are the library's defaults


# ---- trajectories -------------------------------------------------------------------------------------------------------------
# (theta, offset, half length) in 2-D, (theta, phi, offset, psi, half length) in 3-D: a line of direction t through
# centre + offset n, n a unit normal of t; angles in degrees.
LINES = {2: ((20, 0.3, 1.9), (75, 0.9, 1.6), (130, 1.4, 1.4), (-40, 1.7, 1.3), (100, -1.25, 1.7), (10, 2.3, 1.5), (-60, -2.4, 1.2),
             (45, 2.0, 0.9)),
         3: ((15, 10, 0.2, 0, 1.7), (80, -8, 0.75, 30, 1.5), (140, 5, 1.2, 60, 1.4), (-50, 12, 1.5, -45, 1.2), (110, -12, -1.0, 20, 1.5),
             (5, 6, 1.9, 10, 1.5), (-70, -5, -1.8, -10, 1.2), (40, 15, 1.3, 70, 0.9))}
SLACK = 0.02                     # built with FACE + SLACK, so that x +- H and the float32 cast of x stay past FACE
TRIES = 400


def _random_lines(dim, m, rng):
    if dim == 2:
        return np.stack([rng.uniform(0, 360, m), rng.uniform(-2.2, 2.2, m), rng.uniform(0.9, 1.6, m)], axis=1)
    return np.stack([rng.uniform(0, 360, m), rng.uniform(-10, 10, m), rng.uniform(-1.6, 1.6, m), rng.uniform(-30, 30, m),
                     rng.uniform(0.8, 1.3, m)], axis=1)


def _unit(dim, th, ph):
    if dim == 2:
        return np.stack([np.cos(th), np.sin(th)], axis=-1)
    return np.stack([np.cos(th) * np.cos(ph), np.sin(th) * np.cos(ph), np.sin(ph)], axis=-1)


def _clear(sc, p):
    """[k] bool: every point of p [k, P, dim] is on the lattice and FACE + SLACK steps from every cell face."""
    u = p / float(sc["step"])
    f = u - np.floor(u)
    on = np.all((u >= 0) & (u <= np.asarray(sc["shape"]) - 1), axis=(1, 2))
    return on & (np.minimum(f, 1.0 - f).min(axis=(1, 2)) >= FACE + SLACK)


def _balls_at(body, p, th):
    """[k, balls, dim]: the body rule at p [k, dim] with heading th [k]."""
    b = np.asarray(body["b"], F64)
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    w = np.repeat(p[:, None, :], b.shape[0], axis=1)
    w[..., 0] += c * b[:, 0] - s * b[:, 1]
    w[..., 1] += s * b[:, 0] + c * b[:, 1]
    if p.shape[1] == 3:
        w[..., 2] += b[:, 2]
    return w


def build(dim, N, lines, seed):
    """x [m, N, dim] float32, one trajectory per line: waypoint i + 1 = waypoint i + l_i (the line's direction turned by up to
    0.2 rad, in 3-D also tilted by up to 0.1), l_i within 0.6 .. 1.4 of the spacing that is left (longer where a face's zone has
    to be crossed), every draw repeated (fixed seed) until the waypoint and the footprint's balls at both ends of the chord keep
    FACE + SLACK from every cell face.  The chords' directions stay within 0.2 rad of the line's, so every chord has length."""
    sc, body = scene(dim), footprint(dim)
    rng = np.random.default_rng(seed)
    L = np.asarray(lines, F64)
    m = L.shape[0]
    th0 = np.deg2rad(L[:, 0])
    ph0 = np.deg2rad(L[:, 1]) if dim == 3 else np.zeros(m)
    t = _unit(dim, th0, ph0)
    n1 = np.stack([-np.sin(th0), np.cos(th0)] + ([np.zeros(m)] if dim == 3 else []), axis=-1)
    if dim == 2:
        off, half = L[:, 1, None] * n1, L[:, 2]
    else:
        psi = np.deg2rad(L[:, 3])
        off, half = L[:, 2, None] * (np.cos(psi)[:, None] * n1 + np.sin(psi)[:, None] * np.cross(t, n1)), L[:, 4]
    plan = 2.0 * half * (0.8 if N >= 63 else 1.0)            # (the longer chords at the faces add to it)
    mean = plan / (N - 1)
    step = float(sc["step"])

    def heading(k):
        return th0[k] + rng.uniform(-0.2, 0.2, k.size), ph0[k] + (rng.uniform(-0.1, 0.1, k.size) if dim == 3 else 0.0)

    def f32(p):
        return p.astype(F32).astype(F64)

    x = np.zeros((m, N, dim), F64)
    th, ph = np.zeros(m), np.zeros(m)
    todo = np.arange(m)
    for _ in range(TRIES):                                   # the first waypoint and its heading
        p = f32(np.asarray(sc["centre"]) + off[todo] - half[todo, None] * t[todo] + rng.uniform(-0.05, 0.05, (todo.size, dim)))
        a, b = heading(todo)
        ok = _clear(sc, p[:, None, :]) & _clear(sc, _balls_at(body, p, a))
        x[todo[ok], 0], th[todo[ok]], ph[todo[ok]] = p[ok], a[ok], b[ok]
        todo = todo[~ok]
        if todo.size == 0:
            break
    assert todo.size == 0, ("no clear start", dim, N, todo)
    for i in range(1, N):
        todo = np.arange(m)
        nth, nph = th.copy(), ph.copy()
        left = plan - ((x[:, i - 1] - x[:, 0]) * t).sum(axis=1)
        base = np.maximum(left / (N - i), 0.3 * mean)
        for k in range(TRIES):
            # a waypoint cannot cross a face's zone in a chord shorter than the zone: after a few draws the chord may be
            # longer, by up to a step, and what it takes comes off the chords that follow; every other draw also turns anew
            ln = base[todo] * rng.uniform(0.6, 1.4, todo.size) + rng.uniform(0, min(1.0, 0.05 * max(k - 4, 0)), todo.size) * step
            ca, cb = (th[todo], ph[todo]) if k < 3 or k % 2 else heading(todo)
            p = f32(x[todo, i - 1] + ln[:, None] * _unit(dim, ca, cb))
            e = p - x[todo, i - 1]
            real = np.arctan2(e[:, 1], e[:, 0])              # the chord's heading after the cast
            ok = _clear(sc, p[:, None, :]) & _clear(sc, _balls_at(body, x[todo, i - 1], real))
            if i == N - 1:
                ok &= _clear(sc, _balls_at(body, p, real))   # the last waypoint shares the chord
            else:
                a, b = heading(todo)
                ok &= _clear(sc, _balls_at(body, p, a))
                nth[todo[ok]], nph[todo[ok]] = a[ok], b[ok]
            x[todo[ok], i] = p[ok]
            todo = todo[~ok]
            if todo.size == 0:
                break
        assert todo.size == 0, ("no clear waypoint", dim, N, i, todo)
        th, ph = nth, nph
    return x.astype(F32)


@functools.lru_cache(maxsize=None)
def trajectories(dim, N):
    """x [M, N, dim] float32 (N = BATCH: [BATCH_M, BATCH_N, dim] on seeded random lines); read-only."""
    if N == BATCH:
        x = build(dim, BATCH_N, _random_lines(dim, BATCH_M, np.random.default_rng(1000 + dim)), 2000 + dim)
    else:
        x = build(dim, N, LINES[dim], 100 * dim + N)
    x.setflags(write=False)
    return x


def field(dim, dist):
    """The field tuple of traj_obj64 for scene(dim) with the lattice values `dist`."""
    sc = scene(dim)
    return (np.ascontiguousarray(dist, F32).ravel(), sc["shape"], sc["origin"], sc["step"])


# ---- populations --------------------------------------------------------------------------------------------------------------
def census(dim, N, dist):
    """The populations of trajectories(dim, N) on `dist`, from the float64 objective: margins, branches and end terms."""
    x, fld, body = trajectories(dim, N), field(dim, dist), footprint(dim)
    op, ob = opts(dim, fld[3]), opts(dim, fld[3], body["m"])
    mg = float(op["margin"])
    ep = obj.point_excess(x, fld, op)
    eb = obj.body_excess(x, fld, body, ob)
    band = (eb >= 0) & (eb < mg)
    ends_band = band[:, 0].any(axis=1) | band[:, -1].any(axis=1)
    g1 = obj.fd_gradient(lambda y, terms: obj.J_body(y, fld, body, ob, True, terms), x, H)
    g0 = obj.fd_gradient(lambda y, terms: obj.J_body(y, fld, body, ob, False, terms), x, H)
    fp, cp = obj.margins(x, fld, None, H)
    fb, cb = obj.margins(x, fld, body, H)
    return dict(face=min(fp, fb), chord=min(cp, cb), finite=bool(np.isfinite(ep).all() and np.isfinite(eb).all()),
                free=int((ep[:, 1:-1] >= mg).sum()), band=int(((ep[:, 1:-1] >= 0) & (ep[:, 1:-1] < mg)).sum()),
                inside=int((ep[:, 1:-1] < 0).sum()), ball_inside=int((eb < 0).sum()), ends_band=ends_band,
                end_term=float(np.abs(g1 - g0)[ends_band].max()) if ends_band.any() else 0.0)


def check_census(c):
    """What the comparisons rest on; nothing is masked out afterwards."""
    assert c["finite"], c
    assert c["face"] >= FACE and c["chord"] > 0, c
    assert c["free"] > 0 and c["band"] > 0 and c["inside"] > 0, c
    assert c["ball_inside"] > 0 and c["ends_band"].any() and c["end_term"] > 0, c


# ---- tolerances ---------------------------------------------------------------------------------------------------------------
# The floors: the largest deviation of the numpy references (tests/traj_ref.py, tests/traj_body_ref.py: the float32 contract) from
# the float64 objective on the inputs above, measured by tests/test_traj_grad64.py, which asserts that every entry is at least
# the floor it measures and at most 1.25 times it.  A tolerance is FACTOR times the floor: the factor covers other seeds, not
# the device, which has the references' bits.  Nothing here was measured on a device.
FACTOR = 4.0
# (smoother, dim, N) -> (floor of delta relative to the trajectory's largest |delta|, the same for g or None where the g-space
# comparison cannot separate the controls from the floor at that N).
STEP_FLOOR = {
    ('point', 2, 3): (9.47e-07, 9.47e-07), ('point', 2, 4): (2.71e-06, 2.99e-06), ('point', 2, 5): (1.73e-06, 2.74e-06), ('point', 2, 63): (1.29e-06, 7e-05),
    ('point', 2, 64): (7e-07, 8.47e-05), ('point', 2, 65): (7.51e-07, 7.88e-05), ('point', 2, 66): (9.52e-07, 0.000107), ('point', 2, 128): (2.25e-06, 0.000641),
    ('point', 2, 129): (2.15e-06, 0.000655), ('point', 2, 256): (2.23e-06, 0.00307), ('point', 2, BATCH): (3.12e-06, 4.82e-06),
    ('point', 3, 3): (7.18e-07, 7.18e-07), ('point', 3, 4): (1.05e-06, 1.72e-06), ('point', 3, 5): (1.7e-06, 2.72e-06), ('point', 3, 63): (1.08e-06, 4.45e-05),
    ('point', 3, 64): (1.02e-06, 6.47e-05), ('point', 3, 65): (2.24e-06, 7.77e-05), ('point', 3, 66): (9.01e-07, 7.72e-05), ('point', 3, 128): (2.19e-06, 0.000375),
    ('point', 3, 129): (1.5e-06, 0.0004), ('point', 3, 256): (3.92e-06, 0.00222), ('point', 3, BATCH): (2.27e-06, 5.21e-06),
    ('body', 2, 3): (6.63e-07, 6.63e-07), ('body', 2, 4): (2.13e-06, 2.56e-06), ('body', 2, 5): (1.15e-06, 2.06e-06), ('body', 2, 63): (1.07e-06, 7.32e-05),
    ('body', 2, 64): (7.52e-07, 0.000105), ('body', 2, 65): (7.26e-07, 7.51e-05), ('body', 2, 66): (1.12e-06, 8.14e-05), ('body', 2, 128): (1.59e-06, 0.000431),
    ('body', 2, 129): (1.58e-06, 0.000418), ('body', 2, 256): (2.42e-06, 0.000925), ('body', 2, BATCH): (3.04e-06, 5.33e-06),
    ('body', 3, 3): (1.12e-06, 1.12e-06), ('body', 3, 4): (1.15e-06, 1.7e-06), ('body', 3, 5): (9.7e-07, 1.67e-06), ('body', 3, 63): (8.34e-07, 5.54e-05),
    ('body', 3, 64): (8.11e-07, 4.91e-05), ('body', 3, 65): (2.24e-06, 3.93e-05), ('body', 3, 66): (9.01e-07, 8.8e-05), ('body', 3, 128): (2.19e-06, 0.00018),
    ('body', 3, 129): (1.5e-06, 0.000256), ('body', 3, 256): (3.92e-06, 0.000568), ('body', 3, BATCH): (2.12e-06, 4.4e-06),
}
# (smoother, dim, N) -> floor of (x0 - x2) / (2 rate) after two steps of rate TWO_STEP_RATE, relative to its largest value.
TWO_STEP_FLOOR = {('point', 2, 5): 5.45e-05, ('point', 2, 65): 1.99e-05, ('point', 3, 5): 3.37e-05, ('point', 3, 65): 5.78e-05,
                  ('body', 2, 5): 6.87e-05, ('body', 2, 65): 2.05e-05, ('body', 3, 5): 4.63e-05, ('body', 3, 65): 5.78e-05}
# (smoother, dim) -> dict(length, smooth, obstacle, min_dist): floors relative to the batch's largest value, over every N.
EVAL_FLOOR = {
    ('point', 2): dict(length=8.75e-08, smooth=8.42e-08, obstacle=1.05e-07, min_dist=2.59e-07),
    ('point', 3): dict(length=9.24e-08, smooth=8.47e-08, obstacle=1.13e-07, min_dist=3.36e-07),
    ('body', 2): dict(length=8.75e-08, smooth=8.42e-08, obstacle=9.96e-08, min_dist=2.59e-07),
    ('body', 3): dict(length=9.24e-08, smooth=8.47e-08, obstacle=1.28e-07, min_dist=3.36e-07),
}


def step_tol(smoother, dim, N):
    d, g = STEP_FLOOR[smoother, dim, N]
    return FACTOR * d, (None if g is None else FACTOR * g)


def rel(a, b):
    """[m]: max |a - b| of every trajectory relative to its max |b|."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    m = a.shape[0]
    return np.abs(a - b).reshape(m, -1).max(axis=1) / np.abs(b).reshape(m, -1).max(axis=1)
