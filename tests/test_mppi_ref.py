"""The sampling controller's reference (tests/mppi_ref.py) on the CPU: the C-ABI's new symbols and defaults, hand-computed
cases, the invariants of the rollout, the defective variants of the contract the reference must tell apart on the GPU cases'
own inputs (tests/mppi_cases.py), and the behaviour of the whole controller in closed loop on the two ball scenes."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dfield_ref
import mppi_cases as mc
import mppi_ref

F32 = np.float32
F64 = np.float64
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_mppi_default_opts", "gpis_mppi_create", "gpis_mppi_destroy", "gpis_mppi_init", "gpis_mppi_set_nominal", "gpis_mppi_step",
         "gpis_mppi_shift", "gpis_mppi_get", "gpis_mppi_device", "gpis_mppi_info"}
VARIANTS = ("heading_first", "unclamped_d", "noisy0", "floor_index", "counter", "flat_sum", "sum_order")

# ---- the closed loops (recorded in DESIGN.md §7l) ----------------------------------------------------------------------------
LOOP2 = dict(dim=2, K=256, T=12, seed=1, start=1, heading=3.0, terminal="plan", budget=104,         # 69 steps at the first run
             opts=dict(dt=0.5, w_goal=4.0, w_obs=4.0))
LOOP3 = dict(dim=3, K=128, T=8, seed=1, start=0, heading=3.0, terminal="goal", budget=114,          # 76 steps at the first run
             opts=dict(dt=0.5, w_goal=20.0, w_obs=4.0, w_off=2.0, sigma=(0.15, 0.15, 0.15, 0.3)))


def _bits(a):
    return np.ascontiguousarray(a, F64).view(U64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_mppi[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_mppi_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_mppi_opts)]
    for dim, step in ((2, 0.25), (3, 0.2), (2, 0.1)):
        o = gpismap_amd.gpis_mppi_opts()
        assert L.gpis_mppi_default_opts(dim, step, C.byref(o)) == 0
        got = {k: (tuple(getattr(o, k)) if k in ("sigma", "umin", "umax") else getattr(o, "lambda" if k == "lam" else k))
               for k in mppi_ref.OPT_KEYS}
        assert got == mppi_ref.default_opts(dim, step), (dim, step)
        p = gpismap_amd.mppi_opts(dim, step, lam=0.5, sigma=(0.1,) * (4 if dim == 3 else 2), w_col=7.0)
        assert getattr(p, "lambda") == 0.5 and p.w_col == 7.0 and p.dt == o.dt
        assert tuple(p.sigma) == ((0.1,) * 4 if dim == 3 else (0.1, 0.1, 0.0, 0.0))
    assert mppi_ref.default_opts(2, 0.25) == dict(dt=0.1, lam=1.0, gamma=0.1, clearance=0.25, margin=0.5, w_obs=1.0, w_col=100.0,
                                                  w_off=100.0, w_goal=1.0, sigma=(0.25, 0.5, 0.0, 0.0), umin=(0.0, -1.0, 0.0, 0.0),
                                                  umax=(1.0, 1.0, 0.0, 0.0))
    d3 = mppi_ref.default_opts(3, 0.5)
    assert (d3["sigma"], d3["umin"], d3["umax"], d3["clearance"], d3["margin"]) == ((0.25, 0.25, 0.25, 0.5), (-1.0,) * 4, (1.0,) * 4, 0.5, 1.0)
    assert L.gpis_mppi_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_mppi_default_opts(2, 0.1, None) == -1
    assert L.gpis_mppi_default_opts(2, 0.0, C.byref(o)) == -1
    for meth in ("init", "step", "shift", "set_nominal", "get", "info", "device_ptrs", "close"):
        assert callable(getattr(gpismap_amd.Controller, meth)), meth
    assert callable(gpismap_amd.DistanceField.control)
    assert mppi_ref.MAX_K == 65536 and mppi_ref.MAX_T == 256 and mppi_ref.TAG == 2


def test_the_reference_rejects_bad_options():
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(lam=0.0), dict(lam=np.nan), dict(sigma=(0.1, -0.1, 0.0, 0.0)), dict(margin=-0.1),
               dict(w_obs=-1.0), dict(w_col=np.inf), dict(umin=(0.0, 2.0, 0.0, 0.0)), dict(gamma=np.nan), dict(clearance=np.inf)):
        with pytest.raises(ValueError):
            mppi_ref.check_opts(mc.opts(2, **kw), 2)
    mppi_ref.check_opts(mc.opts(2, margin=0.0, gamma=0.0, clearance=-1.0), 2)
    for K, T in ((0, 4), (65537, 4), (4, 0), (4, 257)):
        with pytest.raises(ValueError):
            mppi_ref.Controller(2, K, T)


# ---- hand-computed cases ----------------------------------------------------------------------------------------------------
def test_one_rollout_is_the_nominal():
    """K = 1: the only rollout has z = 0, so q = 2^32, every d_u is 0 and Ubar keeps its bits; u0 = Ubar[0]."""
    for dim in (2, 3):
        c = mc.shape_case(1, 33, dim)
        U0 = mc.nominal_of(c) * np.linspace(0.3, 1.0, 33)[:, None]
        r = mc.ref_step(c, U0, 1)
        assert r["q"][0] == U64(1 << 32) and (r["T"], r["Th"], r["S2"]) == (1 << 32, 1 << 16, 1 << 32) and r["neff"] == 1.0
        assert not r["d"].any() and _same(r["U"], U0) and _same(r["u0"], U0[0]) and r["best"] == 0
        assert _bits(r["nominal_cost"]) == _bits(r["J"][0]) and r["nominal_hits"] == r["hits"][0]


def test_one_step_into_a_wall_costs_w_col():
    sc = mc.scene(2)
    o = mc.opts(2, dt=0.5, gamma=0.0, w_goal=0.0, w_col=123.456)
    r = mppi_ref.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], mc.pose(2, (1.9, 6.0), 0.0), [[1.0, 0.0]], 1, 1, 1, o,
                      goal=sc["goal_point"])
    assert r["hits"][0] == 1 and r["branches"]["col"] == 1 and _bits(r["J"][0]) == _bits(123.456)
    assert _same(r["nominal_states"][1], [2.4, 6.0, 1.0, 0.0])


def test_half_margin_sample_costs_a_quarter_of_w_obs():
    """A field that is exactly x on a lattice of step 0.5: the sample at (1.25, 1.0) is 1.25 exactly; clearance 1 and margin 0.5
    give r = 0.5 and j = w_obs / 4."""
    shape, step = (8, 8), 0.5
    dist = np.tile(np.arange(8, dtype=F32) * F32(step), 8)
    o = mc.opts(2, dt=0.5, gamma=0.0, w_goal=0.0, w_obs=3.0, clearance=1.0, margin=0.5)
    r = mppi_ref.step(dist, shape, (0.0, 0.0), step, mc.pose(2, (0.75, 1.0), 0.0), [[1.0, 0.0]], 1, 1, 1, o, goal=(0.0, 0.0))
    assert r["branches"]["band"] == 1 and r["hits"][0] == 0 and _bits(r["J"][0]) == _bits(0.75)


# ---- invariants -------------------------------------------------------------------------------------------------------------
def test_heading_norm_stays_within_one_ulp_over_256_steps():
    """Exactly (rationals): (1 - 2^-52)^2 <= c^2 + s^2 <= (1 + 2^-52)^2 for every state of 64 rollouts of 256 steps."""
    for dim in (2, 3):
        c = mc.shape_case(64, 256, dim)
        sc = mc.scene(dim)
        cost, goal = mc.terminal_args(c)
        z = mppi_ref.noise(c["seed"], 1, np.arange(64, dtype=U64), 256, mppi_ref.ncontrols(dim))
        r = mppi_ref.rollouts(sc["dist"], sc["shape"], sc["origin"], sc["step"], mppi_ref.start_state(c["pose"], dim), mc.nominal_of(c), z,
                              c["opts"], cost, goal, states=True)
        cs = r["states"][:, :, dim:].reshape(-1, 2)
        assert np.unique(_bits(cs[:, 0])).size > 1000
        lo, hi = (1 - Fraction(1, 2 ** 52)) ** 2, (1 + Fraction(1, 2 ** 52)) ** 2
        n2 = cs[:, 0] * cs[:, 0] + cs[:, 1] * cs[:, 1]
        for i in np.argsort(np.abs(n2 - 1.0))[-200:]:                    # the 200 farthest from 1 in float are checked exactly
            e = Fraction(float(cs[i, 0])) ** 2 + Fraction(float(cs[i, 1])) ** 2
            assert lo <= e <= hi, (dim, i, float(e - 1))
        assert np.abs(n2 - 1.0).max() <= 2.0 ** -51


def test_clamped_perturbation_is_zero_where_the_clamp_pins_both():
    c = mc.branch_cases()["clamp"]
    U0 = mc.nominal_of(c)
    U0[:, 0] = 1.0                                       # the nominal at umax: every positive deviate is clamped away
    r = mc.ref_step(c, U0, 1)
    z = mppi_ref.noise(c["seed"], 1, np.arange(c["K"], dtype=U64), c["T"], 2)
    up = z[:, :, 0] > 0
    assert up.sum() > 500 and not r["d"][:, :, 0][up].any() and np.all(r["d"][:, :, 0][~up] <= 0)
    # the unclamped noise would have moved the mean up; the clamped one cannot
    assert np.all(r["U"][:, 0] <= 1.0)


def test_same_seed_and_tick_same_bits_and_J_does_not_depend_on_K():
    c = mc.shape_case(257, 33)
    a, b = mc.ref_step(c, mc.nominal_of(c), 3), mc.ref_step(c, mc.nominal_of(c), 3)
    assert all(_same(a[k], b[k]) for k in ("J", "U", "nominal_states")) and np.array_equal(a["q"], b["q"])
    other = mc.ref_step(c, mc.nominal_of(c), 4)
    assert np.count_nonzero(_bits(other["J"]) != _bits(a["J"])) > 250 and _bits(other["J"][0]) == _bits(a["J"][0])
    big = mc.ref_step(dict(c, K=1000), mc.nominal_of(c), 3)
    assert _same(big["J"][:257], a["J"]) and np.array_equal(big["hits"][:257], a["hits"])
    seeded = mc.ref_step(dict(c, seed=6), mc.nominal_of(c), 3)
    assert np.count_nonzero(_bits(seeded["J"]) != _bits(a["J"])) > 250


def test_shift_keeps_the_last_row():
    U = np.arange(10, dtype=F64).reshape(5, 2)
    S = mppi_ref.shift(U)
    assert np.array_equal(S[:4], U[1:]) and np.array_equal(S[4], U[4]) and np.array_equal(mppi_ref.shift(U[:1]), U[:1])


# ---- the branches and the defective variants, on the GPU cases' own inputs -----------------------------------------------------
_BASE = {}


def _gpu_cases():
    cases = dict(mc.branch_cases())
    cases.update({"shape2": mc.shape_case(1000, 33), "shape3": mc.shape_case(1000, 33, 3), "shape2_long": mc.shape_case(257, 256)})
    return cases


def test_every_branch_case_reaches_its_branches():
    for name, c in mc.branch_cases().items():
        br = mc.ref_step(c, mc.nominal_of(c), 1)["branches"]
        for e in c["expect"]:
            assert br.get(e, 0) > 0, (name, e, br)
    assert mc.branch_cases()["margin0"]["opts"]["margin"] == 0.0 and mc.branch_cases()["gamma0"]["opts"]["gamma"] == 0.0
    assert mc.branch_cases()["sigma0"]["opts"]["sigma"][1] == 0.0 and mc.branch_cases()["goal2"]["opts"]["gamma"] > 0.0
    r = mc.ref_step(mc.branch_cases()["into_ball"], mc.nominal_of(mc.branch_cases()["into_ball"]), 1)
    assert r["nhit"] > 0 and r["hits"].max() > 1
    s0 = mc.branch_cases()["sigma0"]
    assert not mc.ref_step(s0, mc.nominal_of(s0), 1)["d"][:, :, 1].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_defective_variant_changes_bits(variant):
    changed = []
    for name, c in _gpu_cases().items():
        if name not in _BASE:                            # the contract's own result: computed once, left unchanged
            _BASE[name] = mc.ref_step(c, mc.nominal_of(c), 1)
        a, b = _BASE[name], mc.ref_step(c, mc.nominal_of(c), 1, variant)
        if not all(_same(a[k], b[k]) for k in ("J", "U", "u0", "nominal_states", "nominal_cost")):
            changed.append(name)
    print(variant, "changes", changed)
    assert changed, variant


# ---- closed loop ------------------------------------------------------------------------------------------------------------
def closed_loop(cfg, step_fn=None):
    """Run cfg to the goal with the reference (or with step_fn(pose) -> u0, which steps and shifts, in its place).
    Returns (steps used or None, the least sampled distance over the visited positions, the final distance to the goal)."""
    import traj_cases
    dim = cfg["dim"]
    sc = mc.scene(dim)
    o = mc.opts(dim, **cfg["opts"])
    cost, goal = (sc["cost"], None) if cfg["terminal"] == "plan" else (None, sc["goal_point"])
    ctl = mppi_ref.Controller(dim, cfg["K"], cfg["T"], cfg["seed"])
    st = np.array(list(traj_cases.starts(sc)[cfg["start"]].astype(F64)) + [math.cos(cfg["heading"]), math.sin(cfg["heading"])])
    dmin = lambda p: float(dfield_ref.sample(sc["dist"], sc["shape"], sc["origin"], sc["step"], p[None, :dim].astype(F32))[0, 0])
    least = dmin(st)
    for n in range(cfg["budget"]):
        pose = mppi_ref.pose_of_state(st, dim)
        if step_fn is None:
            u0, _ = ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], pose, o, cost=cost, goal=goal)
            ctl.shift()
        else:
            u0 = step_fn(pose)
        st = mppi_ref.advance(st, u0, dim, o["dt"])
        d = dmin(st)
        if d != d:                                       # off the lattice
            return None, d, float("nan")
        least = min(least, d)
        e = float(np.linalg.norm(st[:dim] - sc["goal_point"]))
        if e <= 2 * sc["step"]:
            return n + 1, least, e
    return None, least, e


@pytest.mark.parametrize("cfg", (LOOP2, LOOP3), ids=("2d_planner", "3d_goal_point"))
def test_closed_loop_reaches_the_goal_with_clearance(cfg):
    sc = mc.scene(cfg["dim"])
    start = __import__("traj_cases").starts(sc)[cfg["start"]]
    hi = np.array(sc["origin"]) + (np.array(sc["shape"]) - 1) * sc["step"]
    assert np.all(start >= np.array(sc["origin"]) + 0.5 * (hi - np.array(sc["origin"])))     # a start in the far half
    steps, least, e = closed_loop(cfg)
    print("dim %d: %s steps of at most %d, least distance %.3f, %.3f from the goal" % (cfg["dim"], steps, cfg["budget"], least, e))
    assert steps is not None and steps <= cfg["budget"] and e <= 2 * sc["step"]
    assert least >= mc.opts(cfg["dim"])["clearance"]
