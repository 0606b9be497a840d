"""The footprint's reference (tests/body_ref.py) on the CPU: the C-ABI's new symbols, the identities with the controller's and
the moving obstacles' references (no footprint, the empty one, the one-ball zero footprint), every branch of the body rule on the
GPU cases' own inputs (tests/body_cases.py), the defective variants the reference must tell apart, the batch query, the
trajectory check's chord rule, and the closed loop through a door wider than the robot and shorter than it is long."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_cases as bc
import body_ref
import mppi_cases as mc
import mppi_ref
import obst_cases as oc
import obst_ref

F32 = np.float32
F64 = np.float64
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_body_create", "gpis_body_destroy", "gpis_body_set", "gpis_body_get", "gpis_body_info", "gpis_body_clearance",
         "gpis_body_mppi_step", "gpis_body_traj_clearance"}


def _bits(a):
    return np.ascontiguousarray(a, F64).view(U64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- exports --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_body[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    # a footprint lives on a device, so without a handle the entries answer GPIS_ERR_ARG
    L.gpis_body_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.gpis_body_info.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    z = (C.c_double * 4)()
    assert L.gpis_body_set(None, 2, 1, z, z) == -1 and L.gpis_body_info(None, z, 4) == -1
    for meth in ("set", "get", "info", "close", "clearance", "box", "box_table"):
        assert callable(getattr(gpismap_amd.Footprint, meth)), meth
    assert callable(gpismap_amd.DistanceField.body_clearance) and callable(gpismap_amd.Trajectories.body_clearance)
    assert callable(gpismap_amd.states_from_poses) and gpismap_amd.Footprint.MAX == body_ref.MAX_M == 16
    # the host helpers: the library's table of a box and its states of poses are the reference's
    off, rad = gpismap_amd.Footprint.box_table(1.0, 0.4, 4)
    ref = body_ref.box(1.0, 0.4, 4)
    assert _same(off, ref["b"]) and _same(rad, ref["rho"]) and _same(rad, np.full(4, np.hypot(0.2, 0.125)))
    assert np.array_equal(off[:, 0], [-0.375, -0.125, 0.125, 0.375]) and not off[:, 1].any()
    for dim, poses in ((2, [mc.FREE2, mc.INTO_BALL2 * 3.0]), (3, [mc.FREE3, mc.INTO_BALL3 * 0.5])):
        assert _same(gpismap_amd.states_from_poses(poses), body_ref.states_from_poses(poses, dim))
        assert _same(body_ref.states_from_poses(poses, dim)[0], mppi_ref.start_state(poses[0], dim))


def test_the_reference_rejects_bad_footprints():
    body_ref.make(2, [(0.1, 0.0)], [0.1])
    assert body_ref.make(3, [], [])["m"] == 0 and body_ref.make(2, np.zeros((16, 2)), np.zeros(16))["m"] == 16
    for kw in (dict(offset=[(np.nan, 0.0)]), dict(offset=[(0.0, np.inf)]), dict(radius=[-0.1]), dict(radius=[np.nan])):
        with pytest.raises(ValueError):
            body_ref.make(2, **dict(dict(offset=[(0.0, 0.0)], radius=[0.1]), **kw))
    with pytest.raises(ValueError):
        body_ref.make(4, [(0.0, 0.0)], [0.1])
    with pytest.raises(OverflowError):
        body_ref.make(2, np.zeros((17, 2)), np.zeros(17))
    S = bc.states(2, 4)
    with pytest.raises(RuntimeError):
        bc.ref_clearance(2, body_ref.make(2, [], []), S)
    for bad in ((0, 1, np.nan), (1, 0, np.inf), (2, 2, 0.0)):
        T = S.copy()
        T[bad[0], bad[1]] = bad[2]
        if bad[2] == 0.0:
            T[bad[0], 3] = 0.0
        with pytest.raises(ValueError):
            bc.ref_clearance(2, bc.footprint(2, 2), T)
    with pytest.raises(ValueError):
        bc.ref_clearance(2, bc.footprint(3, 2), S)


# ---- identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (2, 3))
def test_without_a_footprint_and_with_the_point_the_reference_is_the_controllers(dim):
    """m = 0 is obst_ref's function itself; the one-ball zero footprint has its bits, with and without moving balls."""
    c = oc.shape_case(257, 33, 2, dim)
    sc = mc.scene(dim)
    cost, goal = mc.terminal_args(c)
    U0 = mc.nominal_of(c)
    args = (sc["dist"], sc["shape"], sc["origin"], sc["step"], c["pose"], U0, c["seed"], 1, c["K"], c["opts"], cost, goal)
    for S in (None, c["obst"]):
        full = obst_ref.step(*args, obst=S, t_now=c["t_now"]) if S is not None else mc.ref_step(c, U0, 1)
        for body in (None, body_ref.make(dim, [], []), body_ref.point(dim)):
            got = body_ref.step(*args, obst=S, t_now=c["t_now"], body=body)
            assert all(_same(full[k], got[k]) for k in ("J", "U", "u0", "nominal_states", "nominal_cost", "neff")), (dim, S is None, body)
            assert np.array_equal(full["q"], got["q"]) and np.array_equal(full["hits"], got["hits"])
            assert (full["T"], full["Th"], full["S2"], full["nhit"], full["nominal_hits"], full["best"]) == \
                (got["T"], got["Th"], got["S2"], got["nhit"], got["nominal_hits"], got["best"])
            if S is not None:
                assert _same(full["min_sep"], got["min_sep"]) and np.array_equal(full["dyn_hits"], got["dyn_hits"])
                assert (full["ndyn"], full["nominal_dyn_hits"]) == (got["ndyn"], got["nominal_dyn_hits"])
                assert _same(full["nominal_min_sep"], got["nominal_min_sep"])
    # the batch query of the point is the sampler
    import dfield_ref
    S = bc.states(dim, 257)
    r = bc.ref_clearance(dim, body_ref.point(dim), S)
    d = dfield_ref.sample(sc["dist"], sc["shape"], sc["origin"], sc["step"], S[:, :dim].astype(F32))[:, 0].astype(F64)
    assert np.array_equal(np.isnan(d), np.isnan(r["D"])) and _same(d[~np.isnan(d)], r["D"][~np.isnan(d)])
    assert r["off"] == int(np.isnan(d).sum()) > 0 and np.array_equal(r["ball"], np.where(np.isnan(d), -1, 0))


# ---- the branches and the defective variants ----------------------------------------------------------------------------------
_BASE = {}


def _base(name, c):
    if name not in _BASE:                                # the contract's own result: computed once, left unchanged
        _BASE[name] = bc.ref_step(c, mc.nominal_of(c), 1)
    return _BASE[name]


def test_every_branch_case_reaches_its_branches():
    cases = bc.branch_cases()
    seen = set()
    for name, c in cases.items():
        br = _base(name, c)["branches"]
        for e in c["expect"]:
            assert br.get(e, 0) > 0, (name, e, br)
        seen |= {k for k, v in br.items() if v > 0}
    assert {"off", "col", "band", "free", "second_ball_nearer", "tie", "dyn_col", "dyn_band", "dyn_free", "dyn_off", "dyn_rear"} <= seen
    assert cases["margin0"]["opts"]["margin"] == 0.0 and _base("margin0", cases["margin0"])["branches"]["band"] == 0
    # a body half off the lattice: some of those states have the reference point on the lattice
    c = cases["half_off"]
    pt = bc.ref_step(c, mc.nominal_of(c), 1, body=body_ref.point(2))
    assert pt["branches"]["off"] < _base("half_off", c)["branches"]["off"]
    # the moving ball clears the reference point and hits the rear disc: in the nominal rollout, and in most of the others
    c = cases["rear_hit"]
    r, pt = _base("rear_hit", c), bc.ref_step(c, mc.nominal_of(c), 1, body=body_ref.point(2))
    assert pt["nominal_dyn_hits"] == 0 and pt["nominal_min_sep"] > c["obst"]["opts"]["clearance"]
    assert r["nominal_dyn_hits"] > 0 and r["nominal_min_sep"] < 0 and r["ndyn"] > pt["ndyn"]
    # a wider body hits more
    assert _base("wide", cases["wide"])["nhit"] >= mc.ref_step(cases["wide"], mc.nominal_of(cases["wide"]), 1)["nhit"]


@pytest.mark.parametrize("variant", body_ref.VARIANTS)
def test_defective_variant_changes_bits(variant):
    cases = bc.branch_cases()
    changed = []
    for name, c in cases.items():
        a, b = _base(name, c), bc.ref_step(c, mc.nominal_of(c), 1, variant)
        if not (_same(a["J"], b["J"]) and _same(a["nominal_cost"], b["nominal_cost"])):
            changed.append(name)
    print(variant, "changes J in", changed)
    assert changed, variant
    if variant in ("min_first", "skip_off"):             # min_first shows only where a later ball leaves the lattice before the first
        assert "half_off" in changed and (variant == "skip_off" or changed == ["half_off"])
    if variant == "rot_b2":
        assert set(changed) <= {"sphere3", "leaves3"}


# ---- the batch query ----------------------------------------------------------------------------------------------------------
def test_batch_query_counts_and_positions():
    for dim in (2, 3):
        body = bc.footprint(dim, 5)
        S = bc.states(dim, 1000)
        br = {}
        r = bc.ref_clearance(dim, body, S, 0.1, br=br)
        D = r["D"]
        ok = ~np.isnan(D)
        assert r["off"] == int((~ok).sum()) > 0 and r["below"] == int((D[ok] < 0.1).sum()) > 0 and br["second_ball_nearer"] > 0
        assert r["least"] == int(np.flatnonzero(ok)[np.argmin(D[ok])]) and np.all(r["ball"][~ok] == -1) and np.all(r["ball"][ok] >= 0)
        assert len(set(r["ball"][ok].tolist())) > 1
        # a state has the same bits alone and anywhere in a batch
        one = bc.ref_clearance(dim, body, S[:1], 0.1)
        for at in (0, 63, 64, 999):
            T = S.copy()
            T[[0, at]] = T[[at, 0]]
            got = bc.ref_clearance(dim, body, T, 0.1)
            assert _same(got["D"][at], one["D"][0]) and got["ball"][at] == one["ball"][0]
        # ties go to the lowest index; every state off gives -1
        T = np.concatenate([S[r["least"]][None], S, S[r["least"]][None]])
        assert bc.ref_clearance(dim, body, T)["least"] == 0
        far = S[~ok]
        e = bc.ref_clearance(dim, body, far)
        assert e["least"] == -1 and e["off"] == far.shape[0] and e["below"] == 0
    for variant in ("rot_sign", "no_radius", "cast_first", "skip_off"):
        a, b = bc.ref_clearance(2, bc.footprint(2, 5), bc.states(2, 1000)), bc.ref_clearance(2, bc.footprint(2, 5), bc.states(2, 1000), variant=variant)
        assert not np.array_equal(a["D"].view(U64), b["D"].view(U64)), variant


# ---- trajectories -------------------------------------------------------------------------------------------------------------
def test_chord_rule_on_repeated_waypoints():
    x, names = bc.repeated_waypoints()
    d = (np.float64(0.5) / np.sqrt(np.float64(0.3125)), np.float64(0.25) / np.sqrt(np.float64(0.3125)))
    for r, name in enumerate(names):
        xy = x[r].astype(F64)
        hs = [body_ref.chord_heading(xy, i) for i in range(6)]
        if name == "all_equal":
            assert hs == [(1.0, 0.0)] * 6
        else:
            assert all(_same(h, d) for h in hs), (name, hs)          # the next chord with a length, else the last one before
    trace = {}
    st = np.zeros(5, np.uint8)
    body = bc.traj_body(2)
    ref = bc.ref_traj(2, body, x, st, 0.0, trace=trace)
    assert trace["zero_chord"] > 0 and trace["fwd"] > 0 and trace["back"] > 0 and trace["none"] == 6
    assert np.isfinite(ref["D_min"]).all() and np.all(ref["waypoint"] >= 0) and np.all(ref["ball"] >= 0)
    assert ref["waypoint"][names.index("all_equal")] == 0            # six equal waypoints tie: the first wins
    lx = bc.ref_traj(2, body, x, st, 0.0, variant="last_x")
    changed = [names[r] for r in range(5) if not (_same(ref["D_min"][r], lx["D_min"][r]) and ref["waypoint"][r] == lx["waypoint"][r])]
    print("last_x changes", changed)
    assert changed
    # a status without a result, a trajectory leaving the lattice, one wholly outside it
    y = bc.leaving_waypoints()
    r = bc.ref_traj(2, body, y, np.array([0, 1], np.uint8), 0.0)
    assert r["collides"].tolist() == [1, 1] and np.isfinite(r["D_min"][0]) and r["waypoint"][0] >= 0
    assert np.isnan(r["D_min"][1]) and r["waypoint"][1] == -1 and r["ball"][1] == -1
    r = bc.ref_traj(2, body, y, np.array([2, 2], np.uint8), 0.0)
    assert np.isnan(r["D_min"]).all() and r["collides"].tolist() == [0, 0] and r["waypoint"].tolist() == [-1, -1]


# ---- closed loop ------------------------------------------------------------------------------------------------------------
def test_closed_loop_through_a_door_shorter_than_the_robot():
    """A 1.0 x 0.4 robot and a door 0.7 wide (DESIGN.md §7r records the numbers this prints).  With its footprint of five discs
    the controller drives through without a body hit; the point robot with the circumscribed radius as clearance never gets
    through; the point robot with the inscribed radius gets through with its body in the wall."""
    robot = body_ref.box(bc.ROBOT["length"], bc.ROBOT["width"], bc.ROBOT["discs"])
    body = bc.closed_loop(body=robot, clearance=0.0)
    outer = bc.closed_loop(body=None, clearance=bc.R_OUT)
    inner = bc.closed_loop(body=None, clearance=bc.R_IN)
    for name, r in (("footprint", body), ("point, circumscribed", outer), ("point, inscribed", inner)):
        print("%s: %s steps of at most %d, %.3f from the goal, least body clearance %.3f, %d driven states with the body in the wall"
              % (name, r["steps"], bc.LOOP["budget"], r["e"], np.nanmin(r["D"]), r["hits"]))
    assert body["steps"] is not None and body["hits"] == 0 and np.nanmin(body["D"]) >= 0.0
    assert outer["steps"] is None and outer["states"][-1, 0] < 3.8                       # still in front of the wall
    assert inner["hits"] > 0 and np.nanmin(inner["D"]) < 0.0
