"""The smoothers' numpy references (tests/traj_ref.py, tests/traj_body_ref.py: the float32 contract the kernels follow bit for
bit) against the float64 objective of tests/traj_obj64.py: the step they take is the gradient of the cost, through the inverse
metric.  This file measures the floor the float32 contract leaves, pins the table of tests/traj_grad_cases.py to it, and shows
that a tolerance of four floors rejects every defective control and passes every reordering of the same mathematics.
`python tests/test_traj_grad64.py` prints the tables of DESIGN.md §7v."""
import functools
import time

import numpy as np
import pytest

import dfield_ref
import traj_body_ref
import traj_grad_cases as gc
import traj_obj64 as obj
import traj_ref

F64 = np.float64
KEYS = [(d, N) for d in (2, 3) for N in gc.NS + (gc.BATCH,)]
IDS = ["%dd-N%s" % k for k in KEYS]
REJECTED = {"point": ("band_double", "inside_flat"),
            "body": ("tau_sign", "last_alone", "nearest_only", "r_unrotated", "w_turn0", "no_ends", "band_double", "inside_flat")}
PASSING = {"point": ("desc_j", "thomas", "fused_a"), "body": ()}
EVAL = ("length", "smooth", "obstacle", "min_dist")


@functools.lru_cache(maxsize=None)
def _dist(dim):
    sc = gc.scene(dim)
    d = dfield_ref.distance_field(sc["f"], sc["shape"], sc["origin"], sc["step"], 0.0)[0]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _census(dim, N):
    return gc.census(dim, N, _dist(dim))


def _setup(smoother, dim):
    fld = gc.field(dim, _dist(dim))
    body = gc.footprint(dim) if smoother == "body" else None
    return fld, body, gc.opts(dim, fld[3], body["m"] if body else None)


def _objective(smoother, fld, body, o, ends=True, cost=None):
    if smoother == "point":
        return lambda y, terms=False: obj.J_point(y, fld, o, terms, cost)
    return lambda y, terms=False: obj.J_body(y, fld, body, o, ends, terms, cost)


def _reference(smoother, fld, body, o, x, variant=None, w_turn=1.0):
    if smoother == "point":
        return traj_ref.optimize(fld[0], fld[1], fld[2], fld[3], x, None, o, variant)
    return traj_body_ref.optimize(fld[0], fld[1], fld[2], fld[3], body, x, None, o, w_turn, variant)


def _exact(J, x):
    g = obj.fd_gradient(J, x, gc.H)
    return obj.solve_metric(g), g


def _dev(step, exact, rows=slice(None)):
    """(delta, g): the largest deviation over the trajectories `rows`, relative to each trajectory's largest exact value."""
    return tuple(float(gc.rel(a, b)[rows].max()) for a, b in zip(step, exact))


@functools.lru_cache(maxsize=None)
def _measure(smoother, dim, N):
    """dict(floor, rejected {name: (delta, g)}, passing {name: (delta, g)}) of one (smoother, dim, N)."""
    fld, body, o = _setup(smoother, dim)
    x = gc.trajectories(dim, N)
    exact = _exact(_objective(smoother, fld, body, o), x)
    ref = _reference(smoother, fld, body, o, x)
    assert (ref["status"] == 1).all() and (ref["iterations"] == 1).all() and ref["nonfinite"].dtype == np.int32
    assert np.array_equal(ref["x"][:, 0], x[:, 0]) and np.array_equal(ref["x"][:, -1], x[:, -1])
    step = obj.recover(x, ref["x"], o["rate"])
    out = dict(floor=_dev(step, exact), rejected={}, passing={})
    for name in REJECTED[smoother]:
        if name in obj.COST_VARIANTS:
            out["rejected"][name] = _dev(step, _exact(_objective(smoother, fld, body, o, cost=name), x))
        elif name == "no_ends":
            rows = _census(dim, N)["ends_band"]
            out["rejected"][name] = _dev(step, _exact(_objective(smoother, fld, body, o, ends=False), x), rows)
        else:
            r = _reference(smoother, fld, body, o, x, None, 0.0) if name == "w_turn0" else _reference(smoother, fld, body, o, x, name)
            out["rejected"][name] = _dev(obj.recover(x, r["x"], o["rate"]), exact)
    for name in PASSING[smoother]:
        out["passing"][name] = _dev(obj.recover(x, _reference(smoother, fld, body, o, x, name)["x"], o["rate"]), exact)
    return out


def _pinned(floor, entry, what):
    """The table's entry is the measured floor, rounded up by at most a quarter."""
    assert floor <= entry <= 1.25 * floor, (what, "measured", floor, "table", entry)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def test_the_objective_imports_no_reference():
    with open(obj.__file__.replace(".pyc", ".py")) as f:
        imports = [ln.split()[1] for ln in f if ln.startswith(("import ", "from "))]
    assert sorted(imports) == ["itertools", "numpy"], imports


def test_options_are_the_documented_defaults():
    for dim in (2, 3):
        step, balls = gc.scene(dim)["step"], gc.footprint(dim)["m"]
        ref_p, (ref_b, wt) = traj_ref.default_opts(dim, step), traj_body_ref.default_opts(dim, step, balls)
        for k in traj_ref.OPT_NAMES:
            if k not in gc.CALL:
                assert gc.opts(dim, step)[k] == ref_p[k] and gc.opts(dim, step, balls)[k] == ref_b[k], k
        assert wt == 1 and gc.opts(dim, step)["clearance"] == np.float32(0.1)


@pytest.mark.parametrize("dim,N", KEYS, ids=IDS)
def test_inputs_have_every_population(dim, N):
    """No sampled point within 0.05 of a step from a cell face (waypoints and balls, at x and x +- h), every chord has length, no
    non-finite sample, interior waypoints free, in the band and inside, a ball inside, an end waypoint with a ball in the band
    whose term in the gradient is not zero."""
    x = gc.trajectories(dim, N)
    assert x.dtype == np.float32 and x.shape == ((gc.BATCH_M, gc.BATCH_N, dim) if N == gc.BATCH else (gc.M, N, dim))
    assert x.min() >= 0 and x.max() <= 10
    c = _census(dim, N)
    gc.check_census(c)
    fld, body, o = _setup("body", dim)
    ref = traj_body_ref.optimize(fld[0], fld[1], fld[2], fld[3], body, x, None, o, 1.0, trace=(tr := {}))
    assert tr["turn"].any() and tr["inside"].any() and tr["shared_last"].any(), {k: int(v.sum()) for k, v in tr.items()}
    assert not (tr["nonfinite"].any() or tr["ball_off"].any() or tr["zero_fwd"].any() or tr["zero_back"].any() or tr["zero_none"].any())
    fld, _, o = _setup("point", dim)
    traj_ref.optimize(fld[0], fld[1], fld[2], fld[3], x, None, o, trace=(tp := {}))
    assert tp["inside"].any() and not tp["nonfinite"].any() and not tp["trust"].any() and not tr["trust"].any()
    assert ref["status"].tolist() == [1] * x.shape[0]


@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
@pytest.mark.parametrize("dim", (2, 3))
def test_local_differences_are_the_plain_ones(smoother, dim):
    """fd_gradient's shortcut (every third waypoint at once, three summands each) against one coordinate at a time on the sum."""
    fld, body, o = _setup(smoother, dim)
    for N in (3, 4, 5, 63):
        x = gc.trajectories(dim, N)[:3]
        for ends in ((True, False) if smoother == "body" else (True,)):
            J = _objective(smoother, fld, body, o, ends)
            a, b = obj.fd_gradient(J, x, gc.H), obj.fd_gradient(J, x, gc.H, local=False)
            assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max(), (N, ends, np.abs(a - b).max())


def test_metric_round_trip():
    g = np.random.default_rng(5).normal(size=(3, 254, 3))
    d = obj.solve_metric(g)
    x0 = np.zeros((3, 256, 3))
    x1 = x0.copy()
    x1[:, 1:-1] -= 0.5 * d
    dd, gg = obj.recover(x0, x1, 0.5)
    assert np.abs(dd - d).max() <= 1e-12 * np.abs(d).max() and np.abs(gg - g).max() <= 1e-10 * np.abs(g).max()
    assert np.abs(obj.solve_metric(np.ones((1, 1, 2))) - 0.5).max() == 0          # n = 1: delta = g / 2


# ---- the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", KEYS, ids=IDS)
@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
def test_recovered_step_is_the_objectives_gradient(smoother, dim, N):
    """delta and g recovered from one step of rate 1 against solve_metric(fd_gradient(J)) and fd_gradient(J): J_point, and J_body
    over all N waypoints.  The table's floor is the one measured here; four floors reject every control of REJECTED and pass
    every control of PASSING, and are at most a quarter of the smallest deviation a rejected control shows."""
    r = _measure(smoother, dim, N)
    fd, fg = gc.STEP_FLOOR[smoother, dim, N]
    print("\n%s %dd N=%s floor delta %.3g g %.3g" % (smoother, dim, N, r["floor"][0], r["floor"][1]), r["rejected"], r["passing"])
    _pinned(r["floor"][0], fd, "delta")
    td, tg = gc.step_tol(smoother, dim, N)
    least = [min(v[s] for v in r["rejected"].values()) for s in (0, 1)]
    assert td <= 0.25 * least[0], ("delta", td, r["rejected"])
    for name, v in r["passing"].items():
        assert v[0] <= td, (name, v, td)
    if fg is None:
        assert gc.FACTOR * r["floor"][1] > 0.25 * least[1], ("g could be compared here", r["floor"][1], least[1])
        return
    _pinned(r["floor"][1], fg, "g")
    assert tg <= 0.25 * least[1], ("g", tg, r["rejected"])
    for name, v in r["passing"].items():
        assert v[1] <= tg, (name, v, tg)


def test_the_g_space_is_dropped_only_at_large_N():
    dropped = sorted((k for k, v in gc.STEP_FLOOR.items() if v[1] is None), key=str)
    print("\ng-space dropped at", dropped)
    assert sorted(gc.STEP_FLOOR, key=str) == sorted(((s, d, N) for s in gc.SMOOTHERS for d, N in KEYS), key=str)
    assert all(N != gc.BATCH and N >= 63 for _, _, N in dropped)


# ---- two steps ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_steps(smoother, dim, N):
    fld, body, o = _setup(smoother, dim)
    o = dict(o, rate=np.float32(gc.TWO_STEP_RATE), iters=2)
    x = gc.trajectories(dim, N)
    J = _objective(smoother, fld, body, o)
    x1 = obj.descend(J, x, o["rate"], gc.H)
    x2 = obj.descend(J, x1, o["rate"], gc.H)
    assert np.isfinite(J(x1)).all() and np.isfinite(J(x2)).all()
    stale = 2.0 * x1 - x.astype(F64)                         # the second step taken with the first step's gradient
    ref = _reference(smoother, fld, body, o, x)
    assert (ref["iterations"] == 2).all() and (ref["nonfinite"] == 0).all()
    k = 2.0 * float(o["rate"])
    want = obj.recover(x, x2, k)[0]
    return float(gc.rel(obj.recover(x, ref["x"], k)[0], want).max()), float(gc.rel(obj.recover(x, stale, k)[0], want).max())


@pytest.mark.parametrize("N", gc.TWO_STEP_NS)
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
def test_two_steps_compose(smoother, dim, N):
    """iters = 2 at rate 2^-6 against two float64 steps, the second at the first one's result; a second step taken at the stale
    waypoints is at least four tolerances away."""
    floor, stale = _two_steps(smoother, dim, N)
    print("\n%s %dd N=%d two steps: floor %.3g stale %.3g" % (smoother, dim, N, floor, stale))
    _pinned(floor, gc.TWO_STEP_FLOOR[smoother, dim, N], "two steps")
    assert gc.FACTOR * gc.TWO_STEP_FLOOR[smoother, dim, N] <= 0.25 * stale


# ---- the evaluation -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _evaluation(smoother, dim):
    fld, body, o = _setup(smoother, dim)
    o = dict(o, iters=0)
    worst = dict.fromkeys(EVAL, 0.0)
    for N in gc.NS + (gc.BATCH,):
        x = gc.trajectories(dim, N)
        ref = _reference(smoother, fld, body, o, x)
        assert np.array_equal(ref["x"], x) and (ref["iterations"] == 0).all() and (ref["nonfinite"] == 0).all()
        want = obj.evaluate(x, fld, o, body)
        for k in EVAL:
            worst[k] = max(worst[k], float(np.abs(ref[k] - want[k]).max() / np.abs(want[k]).max()))
        if smoother == "body":                               # the reported obstacle leaves the ends out: it is not J_body's
            full = (_objective(smoother, fld, body, o)(x) - _objective(smoother, fld, body, dict(o, w_obs=0.0))(x)) / float(o["w_obs"])
            rows = _census(dim, N)["ends_band"]
            assert ((full - want["obstacle"])[rows] > 0).all()
    return worst


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("smoother", gc.SMOOTHERS)
def test_evaluation_is_the_objectives_terms(smoother, dim):
    """iters = 0: length, smooth, obstacle (interior waypoints only, for the body too) and min_dist against float64 sums."""
    worst = _evaluation(smoother, dim)
    print("\n%s %dd evaluation floors" % (smoother, dim), worst)
    for k in EVAL:
        _pinned(worst[k], gc.EVAL_FLOOR[smoother, dim][k], k)


if __name__ == "__main__":
    t0 = time.time()
    for s in gc.SMOOTHERS:
        for d, N in KEYS:
            r = _measure(s, d, N)
            print("STEP", (s, d, N), "%.3g %.3g" % r["floor"], "| least rejected %.3g %.3g" % tuple(min(v[i] for v in r["rejected"].values()) for i in (0, 1)),
                  "|", " ".join("%s %.2g/%.2g" % (k, *v) for k, v in {**r["rejected"], **r["passing"]}.items()), flush=True)
    for s in gc.SMOOTHERS:
        for d in (2, 3):
            for N in gc.TWO_STEP_NS:
                print("TWO", (s, d, N), "%.3g stale %.3g" % _two_steps(s, d, N))
            print("EVAL", (s, d), {k: "%.3g" % v for k, v in _evaluation(s, d).items()})
    print("seconds", time.time() - t0)
