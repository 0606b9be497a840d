"""The moving obstacles' reference (tests/obst_ref.py) on the CPU: the C-ABI's new symbols and defaults, the identity with the
sampling controller's reference when there are no balls, every branch of the new term on the GPU cases' own inputs
(tests/obst_cases.py), the defective variants the reference must tell apart, the check of timed trajectories (tunnelling, a
resting robot, bb = 0, timing status 2 and 3) and the closed loops with a crossing ball."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mppi_cases as mc
import mppi_ref
import obst_cases as oc
import obst_ref
from test_mppi_ref import LOOP2, LOOP3

F64 = np.float64
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_obst_default_opts", "gpis_obst_create", "gpis_obst_destroy", "gpis_obst_set", "gpis_obst_set_opts", "gpis_obst_get",
         "gpis_obst_info", "gpis_obst_at", "gpis_obst_mppi_step", "gpis_obst_mppi_get", "gpis_obst_check_timing"}


def _bits(a):
    return np.ascontiguousarray(a, F64).view(U64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_obst[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    L.gpis_obst_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpismap_amd.gpis_obst_opts)]
    for dim, step in ((2, 0.25), (3, 0.2), (2, 0.1)):
        o = gpismap_amd.gpis_obst_opts()
        assert L.gpis_obst_default_opts(dim, step, C.byref(o)) == 0
        assert {k: getattr(o, k) for k in obst_ref.OPT_KEYS} == obst_ref.default_opts(dim, step), (dim, step)
        p = gpismap_amd.obst_opts(dim, step, w_col=7.0, margin=0.0)
        assert p.w_col == 7.0 and p.margin == 0.0 and p.clearance == o.clearance
    assert obst_ref.default_opts(2, 0.25) == dict(clearance=0.25, margin=1.0, w_obs=1.0, w_col=100.0)
    assert L.gpis_obst_default_opts(4, 0.1, C.byref(o)) == -1 and L.gpis_obst_default_opts(2, 0.1, None) == -1
    assert L.gpis_obst_default_opts(2, 0.0, C.byref(o)) == -1
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.obst_opts(2, 0.25, speed=1.0)
    # a set lives on a device, so without a handle the host-only entries answer GPIS_ERR_ARG; gpis_obst_at's values are held to
    # obst_ref.at in tests/test_gpu_obst.py
    L.gpis_obst_at.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double)]
    out = (C.c_double * 2)()
    assert L.gpis_obst_at(None, 0.0, out) == -1
    for meth in ("set", "set_opts", "get", "info", "at", "close"):
        assert callable(getattr(gpismap_amd.Obstacles, meth)), meth
    for meth in ("obstacle_stats", "get_obstacle"):
        assert callable(getattr(gpismap_amd.Controller, meth)), meth
    assert callable(gpismap_amd.Trajectories.check) and obst_ref.MAX_N == 256


def test_the_reference_rejects_bad_sets():
    ok = dict(centre=[(0.0, 0.0)], velocity=[(0.0, 1.0)], radius=[0.1])
    obst_ref.make(2, **ok)
    assert obst_ref.make(2, [], [], [])["n"] == 0
    for kw in (dict(centre=[(np.nan, 0.0)]), dict(velocity=[(0.0, np.inf)]), dict(radius=[-0.1]), dict(radius=[np.nan]), dict(epoch=np.inf),
               dict(clearance=-0.1), dict(margin=np.nan), dict(w_obs=-1.0), dict(w_col=np.inf)):
        with pytest.raises(ValueError):
            obst_ref.make(2, **dict(ok, **kw))
    with pytest.raises(ValueError):
        obst_ref.make(4, **ok)
    with pytest.raises(OverflowError):
        obst_ref.make(2, np.zeros((257, 2)), np.zeros((257, 2)), np.zeros(257))
    S = obst_ref.make(3, [(1.0, 2.0, 3.0), (0.0, 0.0, 0.0)], [(0.5, 0.0, -1.0), (0.0, 0.25, 0.0)], [0.1, 0.2], epoch=2.0)
    assert np.array_equal(obst_ref.at(S, 6.0), [(3.0, 2.0, -1.0), (0.0, 1.0, 0.0)]) and np.array_equal(obst_ref.at(S, 2.0), S["c"])


# ---- identity ---------------------------------------------------------------------------------------------------------------
def test_without_balls_the_reference_is_the_controllers():
    c = mc.shape_case(257, 33)
    sc = mc.scene(2)
    cost, goal = mc.terminal_args(c)
    U0 = mc.nominal_of(c)
    z = mppi_ref.noise(c["seed"], 1, np.arange(c["K"], dtype=U64), c["T"], 2)
    args = (sc["dist"], sc["shape"], sc["origin"], sc["step"], mppi_ref.start_state(c["pose"], 2), U0, z, c["opts"], cost, goal)
    a = mppi_ref.rollouts(*args, states=True)
    empty = obst_ref.make(2, [], [], [])
    for S in (None, empty):
        b = obst_ref.rollouts(*args, states=True, obst=S, t_now=4.0)
        assert all(_same(a[k], b[k]) for k in ("J", "d", "states")) and np.array_equal(a["hits"], b["hits"])
        assert all(a["branches"][k] == b["branches"][k] for k in a["branches"])
        assert not b["dyn_hits"].any() and np.all(np.isposinf(b["min_sep"]))
    full = mc.ref_step(c, U0, 1)
    for S in (None, empty):
        got = obst_ref.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], U0, c["seed"], 1, c["K"], c["opts"], cost, goal,
                            obst=S, t_now=4.0)
        assert all(_same(full[k], got[k]) for k in ("J", "U", "u0", "nominal_states", "nominal_cost", "neff"))
        assert np.array_equal(full["q"], got["q"]) and (full["T"], full["Th"], full["S2"], full["nhit"], full["nominal_hits"], full["best"]) == \
            (got["T"], got["Th"], got["S2"], got["nhit"], got["nominal_hits"], got["best"])
        assert got["ndyn"] == 0 and got["nominal_dyn_hits"] == 0 and got["nominal_min_sep"] == np.inf


# ---- the branches and the defective variants ----------------------------------------------------------------------------------
_BASE = {}


def _base(name, c):
    if name not in _BASE:                                # the contract's own result: computed once, left unchanged
        _BASE[name] = oc.ref_step(c, mc.nominal_of(c), 1)
    return _BASE[name]


def test_every_branch_case_reaches_its_branches():
    cases = oc.branch_cases()
    for name, c in cases.items():
        br = _base(name, c)["branches"]
        for e in c["expect"]:
            assert br.get(e, 0) > 0, (name, e, br)
    assert cases["margin0"]["obst"]["opts"]["margin"] == 0.0 and _base("margin0", cases["margin0"])["branches"]["dyn_band"] == 0
    r = _base("crossing", cases["crossing"])
    assert r["ndyn"] > 0 and r["dyn_hits"].max() > 1 and r["min_sep"].min() < 0 and np.isfinite(r["min_sep"]).all()
    # the field's hits keep their meaning: the static ball's are those of the case without the set
    plain = mc.ref_step(mc.branch_cases()["into_ball"], mc.nominal_of(cases["crossing"]), 1)
    assert np.array_equal(plain["hits"], r["hits"]) and not _same(plain["J"], r["J"])
    # two identical balls are one ball; a far first ball changes nothing either
    for other in ("identical", "second_nearer"):
        b = _base(other, cases[other])
        assert _same(b["J"], r["J"]) and _same(b["min_sep"], r["min_sep"]) and np.array_equal(b["dyn_hits"], r["dyn_hits"])


@pytest.mark.parametrize("variant", obst_ref.VARIANTS)
def test_defective_variant_changes_bits(variant):
    cases = dict(oc.branch_cases(), nan_first=oc.nan_first_case())
    changed = []
    for name, c in cases.items():
        a, b = _base(name, c), oc.ref_step(c, mc.nominal_of(c), 1, variant)
        if not (_same(a["J"], b["J"]) and _same(a["nominal_cost"], b["nominal_cost"])):
            changed.append(name)
    print(variant, "changes J in", changed)
    assert changed, variant
    if variant == "min_first":                           # a NaN separation is not reachable with a set the library accepts
        assert changed == ["nan_first"]


# ---- timed trajectories against a set ---------------------------------------------------------------------------------------
def test_check_special_cases():
    cases = oc.special_check_cases()
    trace = {}
    res = {name: oc.ref_check(c, trace=trace if name != "status23" else None) for name, c in cases.items()}
    for name, c in cases.items():
        tr = {}
        r = oc.ref_check(c, trace=tr)
        for k, want in c["expect"].items():
            if k in ("collides", "first_hit"):
                assert int(r[k][0]) == want, (name, k, r[k])
            else:
                assert tr.get(k, 0) >= want, (name, k, tr)
    t = res["tunnelling"]
    c = cases["tunnelling"]
    assert t["min_sep"][0] < 0 and abs(t["min_time"][0] - 6.5 * c["dt"]) < 1e-9 and t["min_obstacle"][0] == 0
    so = oc.ref_check(c, "sample_only")
    assert so["collides"][0] == 0 and so["first_hit"][0] == -1 and so["min_sep"][0] > 1.0     # both samples are clear
    s = res["still"]
    dur = float(cases["still"]["t"][0, -1])
    assert _bits(s["min_sep"][0]) == _bits(0.375) and s["min_time"][0] == np.ceil(dur / 0.5) * 0.5   # the first resting interval
    st = cases["status23"]["status"]
    r = res["status23"]
    assert set(st.tolist()) == {0, 2, 3}
    dead = st != 0
    assert np.isnan(r["min_sep"][dead]).all() and np.isnan(r["min_time"][dead]).all() and np.all(r["min_obstacle"][dead] == -1)
    assert np.all(r["first_hit"][dead] == -1) and not r["collides"][dead].any() and np.isfinite(r["min_sep"][~dead]).all()
    empty = oc.ref_check(dict(cases["status23"], obst=obst_ref.make(2, [], [], [])))
    assert np.all(np.isposinf(empty["min_sep"][~dead])) and np.isnan(empty["min_time"]).all() and np.all(empty["min_obstacle"] == -1)
    assert np.all(empty["first_hit"] == -1) and not empty["collides"].any() and np.isnan(empty["min_sep"][dead]).all()
    for kw in (dict(steps=0), dict(steps=4097), dict(dt=0.0), dict(dt=np.nan), dict(t0=-0.5), dict(clearance=-1.0), dict(t_begin=np.inf)):
        with pytest.raises(ValueError):
            oc.ref_check(dict(cases["still"], **kw))


@pytest.mark.parametrize("variant", obst_ref.CHECK_VARIANTS)
def test_defective_check_variant_changes_the_output(variant):
    changed = []
    for name, c in oc.special_check_cases().items():
        a, b = oc.ref_check(c), oc.ref_check(c, variant)
        if not all(np.array_equal(a[k], b[k], equal_nan=True) for k in a):
            changed.append(name)
    print(variant, "changes", changed)
    assert changed, variant


# ---- closed loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", (LOOP2, LOOP3), ids=("2d_disc", "3d_sphere"))
def test_closed_loop_avoids_a_crossing_ball(cfg):
    """tests/test_mppi_ref.py's closed loops with a ball of speed 0.3 and radius 0.4 through the unaware robot's position of step
    30 at step 30, perpendicular to its heading (DESIGN.md §7q records the numbers this prints)."""
    sc = mc.scene(cfg["dim"])
    unaware = oc.closed_loop(cfg)
    ball = oc.crossing_ball(cfg, unaware["states"], 0.3, 0.4)
    unaware = oc.closed_loop(cfg, track=ball)
    aware = oc.closed_loop(cfg, obst=ball)
    for name, r in (("without the set", unaware), ("with the set", aware)):
        print("dim %d %s: %s steps of at most %d, least field distance %.3f, least separation %.3f, %.3f from the goal"
              % (cfg["dim"], name, r["steps"], cfg["budget"], r["least"], r["sep"], r["e"]))
    assert unaware["sep"] < 0                                                            # a collision
    assert aware["sep"] >= ball["opts"]["clearance"]
    assert aware["steps"] is not None and aware["steps"] <= cfg["budget"] and aware["e"] <= 2 * sc["step"]
    assert aware["least"] >= mc.opts(cfg["dim"])["clearance"]
