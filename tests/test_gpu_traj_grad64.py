"""The smoothers on the GPU (traj_opt_kernel<DIM, BODY> of csrc/traj.hip) against the float64 objective of
tests/traj_obj64.py on the device's own dist: the step they take is the gradient of the cost, two steps compose, the evaluation's
terms are the cost's, and the sampler's gradient is the interpolant's derivative.  No reference of the smoothers is imported; the
tolerances are tests/traj_grad_cases.py's (four floors of the float32 contract, measured on the CPU by tests/test_traj_grad64.py)
and, for the sampler, a bound derived from the number format."""
import functools

import numpy as np
import pytest

import traj_grad_cases as gc
import traj_obj64 as obj

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
EVAL = ("length", "smooth", "obstacle", "min_dist")
DIM_N = [(d, N) for d in (2, 3) for N in gc.NS]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def _env(dim):
    """(DistanceField, traj_obj64's field on the device's own dist)."""
    import gpismap_amd
    sc = gc.scene(dim)
    df = gpismap_amd.DistanceField()
    df.from_grid(_dev(sc["f"]).data_ptr(), sc["shape"], sc["origin"], float(sc["step"]), 0.0)
    dist = df.get()[0].ravel()
    assert np.isfinite(dist).all()
    return df, gc.field(dim, dist)


@functools.lru_cache(maxsize=None)
def _census(dim, N):
    c = gc.census(dim, N, _env(dim)[1][0])
    gc.check_census(c)
    return c


def _setup(smoother, dim):
    df, fld = _env(dim)
    body = gc.footprint(dim) if smoother == "body" else None
    return df, fld, body, gc.opts(dim, fld[3], body["m"] if body else None)


def _objective(smoother, fld, body, o):
    if smoother == "point":
        return lambda y, terms=False: obj.J_point(y, fld, o, terms)
    return lambda y, terms=False: obj.J_body(y, fld, body, o, True, terms)


def _smooth(smoother, dim, x, o):
    """One call with the options of `o` that a call passes; the others are the library's defaults, which are o's."""
    import gpismap_amd
    df, fld, body, _ = _setup(smoother, dim)
    call = {k: (int(o[k]) if k == "iters" else float(o[k])) for k in gc.CALL}
    if body is None:
        lib = gpismap_amd.traj_opts(dim, float(fld[3]), **call)
        kw = {}
    else:
        lib, wt = gpismap_amd.traj_body_opts(dim, float(fld[3]), body["m"], **call)
        assert wt == 1.0
        kw = dict(footprint=gpismap_amd.Footprint(dim).set(body["b"], body["rho"]), w_turn=1.0)
    for k, v in o.items():
        assert getattr(lib, k) == v, (k, getattr(lib, k), v)
    tj = gpismap_amd.Trajectories()
    df.smooth(np.array(x), trajectories=tj, **kw, **call)
    return tj.get()


def _check_step(smoother, dim, N):
    _census(dim, N)
    df, fld, body, o = _setup(smoother, dim)
    x = gc.trajectories(dim, N)
    got = _smooth(smoother, dim, x, o)
    assert (got["status"] == 1).all() and (got["iterations"] == 1).all()
    assert np.array_equal(got["x"][:, 0].view(np.uint32), x[:, 0].view(np.uint32))
    assert np.array_equal(got["x"][:, -1].view(np.uint32), x[:, -1].view(np.uint32))
    assert np.isfinite(got["x"]).all()
    delta, g = obj.recover(x, got["x"], o["rate"])
    g64 = obj.fd_gradient(_objective(smoother, fld, body, o), x, gc.H)
    ed, eg = gc.rel(delta, obj.solve_metric(g64)), gc.rel(g, g64)
    td, tg = gc.step_tol(smoother, dim, N)
    print("\n%s %dd N=%s: delta %.3g (tolerance %.3g), g %.3g (%s)" % (smoother, dim, N, ed.max(), td, eg.max(), tg))
    assert (ed <= td).all(), ("delta", np.flatnonzero(ed > td), ed.max(), td)
    if tg is not None:
        assert (eg <= tg).all(), ("g", np.flatnonzero(eg > tg), eg.max(), tg)


def test_inputs_and_options_on_the_device():
    """The device's dist gives the populations the CPU file asserts on the reference's dist."""
    for dim in (2, 3):
        for N in gc.NS + (gc.BATCH,):
            _census(dim, N)


@pytest.mark.parametrize("dim,N", DIM_N)
def test_point_step_is_the_objectives_gradient(dim, N):
    """One unclipped step of rate 1: delta and g recovered from the returned x against solve_metric(fd_gradient(J_point)) and
    fd_gradient(J_point); status 1, one iteration, the ends unmoved bit for bit."""
    _check_step("point", dim, N)


@pytest.mark.parametrize("dim,N", DIM_N)
def test_body_step_is_the_objectives_gradient(dim, N):
    """The same with the footprint and w_turn = 1 against J_body over all N waypoints."""
    _check_step("body", dim, N)


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
def test_large_batch(smoother, dim):
    """300 trajectories of 5 waypoints, more workgroups than compute units; every trajectory against its own tolerance."""
    _check_step(smoother, dim, gc.BATCH)


@pytest.mark.parametrize("N", gc.TWO_STEP_NS)
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
def test_two_steps_compose(smoother, dim, N):
    """iters = 2 at rate 2^-6 against two float64 steps, the second taken at the first one's result."""
    df, fld, body, o = _setup(smoother, dim)
    o = dict(o, rate=F32(gc.TWO_STEP_RATE), iters=2)
    x = gc.trajectories(dim, N)
    got = _smooth(smoother, dim, x, o)
    assert (got["iterations"] == 2).all() and (got["status"] == 1).all() and (got["nonfinite"] == 0).all()
    J = _objective(smoother, fld, body, o)
    x2 = obj.descend(J, obj.descend(J, x, o["rate"], gc.H), o["rate"], gc.H)
    assert np.isfinite(J(x2)).all()
    k = 2.0 * float(o["rate"])
    err = gc.rel(obj.recover(x, got["x"], k)[0], obj.recover(x, x2, k)[0])
    tol = gc.FACTOR * gc.TWO_STEP_FLOOR[smoother, dim, N]
    print("\n%s %dd N=%d two steps: %.3g (tolerance %.3g)" % (smoother, dim, N, err.max(), tol))
    assert (err <= tol).all(), (np.flatnonzero(err > tol), err.max(), tol)


@pytest.mark.parametrize("dim", (2, 3))
def test_evaluation_is_the_objectives_terms(dim):
    """iters = 0, both smoothers, every N: length, smooth, obstacle (the interior waypoints, for the body too) and min_dist
    against float64 sums, relative to the batch's largest value; x comes back as it went in."""
    for smoother in gc.SMOOTHERS:
        df, fld, body, o = _setup(smoother, dim)
        o = dict(o, iters=0)
        for N in gc.NS + (gc.BATCH,):
            x = gc.trajectories(dim, N)
            got = _smooth(smoother, dim, x, o)
            assert np.array_equal(got["x"].view(np.uint32), x.view(np.uint32)) and (got["iterations"] == 0).all()
            assert (got["nonfinite"] == 0).all() and (got["status"] == 1).all()
            want = obj.evaluate(x, fld, o, body)
            for k in EVAL:
                err = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
                tol = gc.FACTOR * gc.EVAL_FLOOR[smoother, dim][k]
                print("%s %dd N=%s %s: %.3g (tolerance %.3g)" % (smoother, dim, N, k, err, tol))
                assert err <= tol, (smoother, N, k, err, tol)


@pytest.mark.parametrize("dim", (2, 3))
def test_sampler_gradient_is_the_interpolants_derivative(dim):
    """DistanceField.sample at 300 points inside cells, at points on interior faces of one, two and all axes, on the last
    lattice point of one and of every axis, and off the lattice: the value against traj_obj64.interp, the gradient against
    differences of it, central inside a cell and one-sided, into the cell that i0 = min(floor(u), n - 2) selects, on a face
    (the interpolant is linear along an axis inside a cell, so either difference is its derivative).  The tolerance is derived:
    a chain of `dim` lerps on values of size V costs at most (2 dim + 1) 2^-24 V in the value, and that over the step in a
    derivative; the coordinates (multiples of 2^-10 steps on a lattice of step 0.25 at origin 0) add nothing."""
    df, fld = _env(dim)
    dist, shape, origin, step = fld
    step = float(step)
    n = np.asarray(shape)
    rng = np.random.default_rng(40 + dim)
    u = rng.integers(0, n - 1, (300, dim)) + rng.integers(103, 922, (300, dim)) / 1024.0      # inside a cell, 0.1 .. 0.9
    faces = []
    for k in range(1, dim + 1):                                                               # k axes on an interior face
        f = rng.integers(0, n - 1, (60, dim)) + rng.integers(103, 922, (60, dim)) / 1024.0
        for r in range(60):
            ax = rng.choice(dim, k, replace=False)
            f[r, ax] = rng.integers(1, n[ax] - 1)
        faces.append(f)
    last = rng.integers(0, n - 1, (dim + 1, dim)) + rng.integers(103, 922, (dim + 1, dim)) / 1024.0
    for a in range(dim):
        last[a, a] = n[a] - 1
    last[dim] = n - 1
    u = np.concatenate([u] + faces + [last, np.zeros((1, dim))])
    p = (u * step).astype(F32)
    assert np.array_equal(p.astype(F64), u * step)
    off = (n - 1 + 0.5) * step * np.eye(dim)[:1]
    got = df.sample(np.concatenate([p, off.astype(F32)]))
    assert np.isnan(got[-1]).all() and np.isnan(obj.interp(*fld, off)).all()
    got = got[:-1].astype(F64)
    V = float(np.abs(dist).max())
    tol = (2 * dim + 1) * 2.0 ** -24 * V
    P = p.astype(F64)
    ev = np.abs(got[:, 0] - obj.interp(*fld, P)).max()
    assert ev <= tol, (ev, tol)
    h = 0.05 * step
    i0 = np.minimum(np.floor(u), n - 2)
    w = u - i0
    worst = 0.0
    for a in range(dim):
        e = np.zeros(dim)
        e[a] = h
        lo = np.where((w[:, a] > 0)[:, None], P - e, P)                                       # w = 0: forward; w = 1: backward
        hi = np.where((w[:, a] < 1)[:, None], P + e, P)
        d = (obj.interp(*fld, hi) - obj.interp(*fld, lo)) / (hi - lo)[:, a]
        assert np.isfinite(d).all()
        worst = max(worst, float(np.abs(got[:, 1 + a] - d).max()))
    print("\nsampler %dd: value %.3g (bound %.3g), gradient %.3g (bound %.3g)" % (dim, ev, tol, worst, tol / step))
    assert ((w == 0).any() and (w == 1).any() and ((w == 0).sum(axis=1) == dim).any())
    assert worst <= tol / step, (worst, tol / step)
