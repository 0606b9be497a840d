"""The footprint in the moving-obstacle check and in re-timing, host side and reference (tests/body_time_ref.py) on the CPU: the
exported C entries, the arguments the reference refuses, every branch of the contract on the shared cases
(tests/body_time_cases.py) counted by a trace, the certificate (a body schedule's own body check is clear), the one-ball zero
footprint against obst_ref.check, retime_ref.solve and retime_ref.check bit for bit, the relations of DESIGN.md §7x's table, and
the defective variants."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import body_ref
import body_time_cases as bc
import body_time_ref as btr
import obst_cases as oc
import obst_ref
import retime_cases as rc
import retime_ref as rr
import timing_cases as tc

F32 = np.float32
F64 = np.float64
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpis_timed_body_check", "gpis_timed_body_retime", "gpis_timed_body_info", "gpis_timed_body_retime_check",
         "gpis_timed_body_states"}
SKEYS = rr.RES_KEYS + ("own",)
POINT_KEYS = ("min_sep", "min_time", "min_obstacle", "first_hit", "collides")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == F64:
        return bool(((a.view(U64) == b.view(U64)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


@functools.lru_cache(maxsize=None)
def _solved(name):
    """The contract's own result of a special case with its trace and tables: computed once, left unchanged."""
    c = bc.special_cases()[name]
    trace, keep = {}, {}
    return c, bc.ref_solve(c, trace=trace, keep=keep), trace, keep


def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_timed_body[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    d, vp, i = C.c_double, C.c_void_p, C.c_int
    L.gpis_timed_body_check.argtypes = [vp, vp, vp, d, i, d, d, d] + [vp] * 6
    L.gpis_timed_body_retime.argtypes = [vp, vp, vp, d, vp, vp]
    L.gpis_timed_body_info.argtypes = [vp, vp, i]
    L.gpis_timed_body_retime_check.argtypes = [vp, vp, vp, i, d] + [vp] * 6
    L.gpis_timed_body_states.argtypes = [vp, d, i, d, i, vp]
    o = gpismap_amd.gpis_retime_opts()
    # the entries work on handles, which live on a device: without one they answer GPIS_ERR_ARG
    assert L.gpis_timed_body_check(None, None, None, 0.1, 4, 0.0, 0.0, 0.1, *[None] * 6) == -1
    assert L.gpis_timed_body_retime(None, None, None, 0.0, C.byref(o), None) == -1
    assert L.gpis_timed_body_info(None, None, 1) == -1
    assert L.gpis_timed_body_retime_check(None, None, None, 4, 0.1, *[None] * 6) == -1
    assert L.gpis_timed_body_states(None, 0.1, 4, 0.0, 0, None) == -1
    T = gpismap_amd.Trajectories
    for meth in ("check", "retime", "retimed_check"):
        assert "footprint" in inspect.signature(getattr(T, meth)).parameters, meth
    assert {"dt", "steps", "t0", "retimed"} <= set(inspect.signature(T.timed_states).parameters) and callable(T.retimed_body_balls)


def test_the_reference_refuses_what_the_library_refuses():
    c = bc.rear_only()
    a = (c["x"], c["v"], c["t"], c["status"], c["obst"])
    chk = lambda body=c["body"], S=c["obst"], **kw: btr.check(c["x"], c["v"], c["t"], c["status"], S, body,
                                                               **dict(dict(dt=0.25, steps=4, t0=0.0, t_begin=0.0, clearance=0.1), **kw))
    bad_bodies = (None, body_ref.make(2, np.zeros((0, 2)), []), bc.body(3, 2))
    for b in bad_bodies:
        with pytest.raises(ValueError):
            chk(body=b)
        with pytest.raises(ValueError):
            btr.solve(*a, b, 0.0, bc.BASE)
        with pytest.raises(ValueError):
            btr.sched_check(c["x"], c["v"], c["t"], c["status"], rr.solve(*a, 0.0, bc.BASE), c["obst"], b, 4, 0.1)
    for kw in (dict(dt=0.0), dict(dt=np.nan), dict(steps=0), dict(steps=4097), dict(t0=-1.0), dict(clearance=-0.1), dict(t_begin=np.inf),
               dict(S=oc.balls(3, 2, 0.2))):
        with pytest.raises(ValueError):
            chk(**kw)
    for o in (dict(bc.BASE, slot=0.0), dict(bc.BASE, max_pause=256), dict(bc.BASE, clearance=-1.0), dict(bc.BASE, press_on=2)):
        with pytest.raises(ValueError):
            btr.solve(*a, c["body"], 0.0, o)
    with pytest.raises(ValueError):
        btr.solve(*a, c["body"], np.nan, bc.BASE)
    with pytest.raises(ValueError):
        btr.states(c["x"], c["v"], c["t"], c["status"], 0.25, 0)
    with pytest.raises(ValueError):
        btr.states(c["x"], c["v"], c["t"], c["status"], -0.25, 4)


# ---- the zero footprint is the point ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oc.CHECK_SHAPES[:5] + oc.CHECK_SHAPES3)
def test_zero_footprint_check_has_the_point_checks_bits(shape):
    dim = 3 if shape in oc.CHECK_SHAPES3 else 2
    c = oc.check_shape_case(*shape, dim=dim)
    ref = oc.ref_check(c)
    got = btr.check(c["x"], c["v"], c["t"], c["status"], c["obst"], body_ref.point(dim), c["dt"], c["steps"], c["t0"], c["t_begin"], c["clearance"])
    for k in POINT_KEYS:
        assert _bits(got[k], ref[k]), (shape, k)
    timed = ~np.isnan(ref["min_sep"]) & np.isfinite(ref["min_sep"])
    assert np.array_equal(got["min_ball"], np.where(timed, 0, -1))


@pytest.mark.parametrize("name", sorted(rc.special_cases()))
def test_zero_footprint_solve_and_check_are_the_point_solves(name):
    c = rc.special_cases()[name]
    dim = c["x"].shape[2]
    a = (c["x"], c["v"], c["t"], c["status"])
    ref = rc.ref_solve(c)
    got = btr.solve(*a, c["obst"], body_ref.point(dim), c["t_begin"], c["opts"])
    assert all(np.array_equal(got[k], ref[k]) and got[k].dtype == ref[k].dtype for k in SKEYS) and got["body"] == 1
    steps = int(max(1, ref["arrive"].max() + 2))
    k0, k1 = rr.check(*a, ref, c["obst"], steps), btr.sched_check(*a, got, c["obst"], body_ref.point(dim), steps)
    for k in POINT_KEYS:
        assert _bits(k1[k], k0[k]), (name, k)
    # the poses' positions are the point's positions
    live = np.flatnonzero(ref["status"] <= 1)[:1]
    for r in live:
        Q = btr.sched_poses(*a[:3], got, r, 0, 6)
        assert _bits(Q[:, :dim], rr.sched_positions(*a[:3], ref, r, 0, 6))


# ---- every branch, and the certificate -----------------------------------------------------------------------------------------------
def test_every_branch_is_reached_and_counted():
    total = {}
    for name in sorted(bc.special_cases()):
        _, _, trace, _ = _solved(name)
        for k, v in trace.items():
            total[k] = total.get(k, 0) + v
    for k in ("status0", "status1", "status2", "status3", "status4", "n0", "both", "play", "pause", "past", "inside", "chord_own", "chord_none",
              "turn_block"):
        assert total.get(k, 0) > 0, (k, total)
    tr = {}
    bc.ref_check(bc.knot_case(), trace=tr)
    for k in ("on_knot", "past", "inside", "chord_own", "chord_none", "untimed", "front", "rear", "hit"):
        assert tr.get(k, 0) > 0, (k, tr)
    tr3 = {}
    bc.ref_check(bc.check_shape_case(*bc.CHECK_SHAPES3[0], dim=3), trace=tr3)
    assert tr3.get("chord_fwd", 0) > 0, tr3                # the corner's vertical first leg: the first horizontal chord ahead
    trb = {}
    d = bc.dup_end()
    bc.ref_check(d, trace=trb)
    assert trb.get("chord_back", 0) > 0 and d["status"][0] == 0, trb
    tr0 = {}
    bc.ref_check(bc.check_shape_case(*bc.CHECK_SHAPES[5]), trace=tr0)
    assert tr0.get("n0", 0) > 0


@pytest.mark.parametrize("name", sorted(bc.special_cases()))
def test_special_case_status_and_certificate(name):
    c, sch, _, _ = _solved(name)
    expect = dict(table=1, parked_beside=0, turn_knot=3).get(name, c.get("expect", {}).get("status"))
    if name in ("clear", "crossing", "crossing_late", "two_discs", "parked", "short_of_pauses", "empty", "point", "a1025", "table",
                "parked_beside", "turn_knot"):
        assert int(sch["status"][0]) == expect, (name, sch["status"])
    clr = c["opts"]["clearance"]
    a = (c["x"], c["v"], c["t"], c["status"])
    for r in np.flatnonzero((sch["status"] <= 1) & (sch["arrive"] >= 1)):
        k = btr.sched_check(*a, sch, c["obst"], c["body"], int(sch["arrive"][r]), clr)
        assert k["collides"][r] == 0 and k["first_hit"][r] == -1 and (c["obst"]["n"] == 0 or k["min_sep"][r] >= clr), (name, r, k["min_sep"][r])
    assert sch["body"] == c["body"]["m"]


@pytest.mark.parametrize("shape", (bc.SHAPES[2], bc.SHAPES[3], bc.SHAPES3[0]))
def test_certificate_on_shapes(shape):
    c = bc.shape_case(*shape, dim=3 if shape in bc.SHAPES3 else 2)
    sch = bc.ref_solve(c)
    a = (c["x"], c["v"], c["t"], c["status"])
    clr = c["opts"]["clearance"]
    live = np.flatnonzero((sch["status"] <= 1) & (sch["arrive"] >= 1))
    assert live.size
    for r in live:
        k = btr.sched_check(*a, sch, c["obst"], c["body"], min(int(sch["arrive"][r]), 4096), clr)
        assert k["collides"][r] == 0 and k["min_sep"][r] >= clr, (shape, r)


# ---- the scene of the table ------------------------------------------------------------------------------------------------------------
def test_the_tables_scene_orders_the_body_between_the_two_points():
    """The numbers of DESIGN.md §7x's table, asserted as relations."""
    for vel in ((0.0, 0.3), (0.3, 0.3), (-0.2, 0.3)):
        rows = bc.table_scene(vel)["rows"]
        pauses = {k: int(s["pauses"][0]) for k, (s, _) in rows.items()}
        sep = {k: float(ck["min_sep"][0]) for k, (_, ck) in rows.items()}
        hit = {k: int(ck["collides"][0]) for k, (_, ck) in rows.items()}
        print(vel, pauses, sep, hit)
        assert all(int(s["status"][0]) == 1 for s, _ in rows.values())
        assert pauses["inscribed"] <= pauses["body"] <= pauses["circumscribed"]
        assert hit["inscribed"] == 1 and hit["disc"] == 1 and hit["body"] == 0 and sep["body"] >= bc.BASE["clearance"]
        assert sep["inscribed"] < bc.BASE["clearance"] and sep["disc"] < bc.BASE["clearance"]
    rows = bc.table_scene()["rows"]
    assert [int(rows[k][0]["pauses"][0]) for k in ("body", "inscribed", "disc", "circumscribed")] == [14, 12, 13, 17]
    assert [round(float(rows[k][1]["min_sep"][0]), 4) for k in ("body", "inscribed", "disc", "circumscribed")] == [0.2672, 0.1235, 0.1953, 0.4827]


def test_parked_beside_passes_with_the_body_and_not_with_the_circumscribed_point():
    c = bc.parked_beside()
    a = (c["x"], c["v"], c["t"], c["status"])
    assert int(bc.ref_solve(c)["status"][0]) == 0
    assert int(rr.solve(*a, c["obst"], 0.0, dict(bc.BASE, clearance=bc.BASE["clearance"] + bc.R_OUT))["status"][0]) == 3


def test_a_ball_that_hits_the_rear_ball_alone():
    c = bc.rear_only()
    a = (c["x"], c["v"], c["t"], c["status"], c["obst"])
    tail = (c["dt"], c["steps"], c["t0"], c["t_begin"], c["clearance"])
    got = bc.ref_check(c)
    assert got["collides"][0] == 1 and got["min_ball"][0] == 1 and got["first_hit"][0] == 10
    pt = obst_ref.check(*a, *tail)
    assert pt["collides"][0] == 0 and pt["min_sep"][0] > c["clearance"]
    front = btr.check(*a, body_ref.make(2, bc.TWO["off"][:1], bc.TWO["rho"][:1]), *tail)
    assert front["collides"][0] == 0
    # the defective variant: rho not subtracted
    bad = bc.ref_check(c, variant="no_rho")
    assert abs((bad["min_sep"][0] - got["min_sep"][0]) - 0.1) < 1e-12 and bad["min_ball"][0] == 1


def test_a_turn_at_a_knot_blocks_the_play_cell_alone():
    tk = bc.turn_knot()
    c, a = tk["case"], tk["a"]
    keep = {}
    sch = bc.ref_solve(c, keep=keep)
    T = keep[0]
    assert (T["Q"][a, 2:] != T["Q"][a + 1, 2:]).any()
    assert not T["play"][a].any() and T["pause"][a].all() and T["pause"][a + 1].all() and int(sch["status"][0]) == 3
    # the defective variant: the play cell with the heading of slot a at both ends
    keep_h = {}
    hold = bc.ref_solve(c, variant="play_hold", keep=keep_h)
    assert keep_h[0]["play"][a].all() and int(hold["status"][0]) == 0


def test_defective_variants_change_their_cases():
    # the heading of segment i + 1: the half circle turns at every knot
    c = bc.check_shape_case(1, 64, 64, 1, 2)
    ref, bad = bc.ref_check(c), bc.ref_check(c, variant="heading_next")
    assert not _bits(ref["min_sep"], bad["min_sep"])
    s0 = btr.states(c["x"], c["v"], c["t"], c["status"], c["dt"], 8)
    s1 = btr.states(c["x"], c["v"], c["t"], c["status"], c["dt"], 8, variant="heading_next")
    assert _bits(s0[..., :2], s1[..., :2]) and not _bits(s0[..., 2:], s1[..., 2:])
    # the pause cell at its first sample only: the fast disc of retime_cases' tunnel goes through a waiting body between samples
    c = bc.special_cases()["tunnel"]
    ref, bad = bc.ref_solve(c), bc.ref_solve(c, variant="pause_sample")
    assert not all(np.array_equal(ref[k], bad[k]) for k in SKEYS)
    a = (c["x"], c["v"], c["t"], c["status"])
    k = btr.sched_check(*a, bad, c["obst"], c["body"], int(bad["arrive"][0]), c["opts"]["clearance"])
    assert k["collides"][0] == 1
    for v in btr.VARIANTS:
        assert v in inspect.getsource(btr)


# ---- the timed poses -----------------------------------------------------------------------------------------------------------------
def test_states_pin_the_heading_rule():
    for dim in (2, 3):
        x, v, t, st = oc.batch(dim, 11, 64)
        dt = 0.5
        S = btr.states(x, v, t, st, dt, 40, t0=0.125)
        assert S.shape == (11, 41, dim + 2)
        for r in range(11):
            if st[r] != 0:
                assert np.isnan(S[r]).all()
                continue
            xs, vs, ts = x[r].astype(F64), v[r].astype(F64), t[r].astype(F64)
            for k in (0, 7, 40):
                tau = F64(0.125) + F64(k) * F64(dt)
                p, i, c, s = btr.pose(xs, vs, ts, tau)
                assert _bits(S[r, k], np.concatenate([p, [c, s]]))
                assert i == (63 if tau >= ts[-1] else int(np.searchsorted(ts, tau, side="right")) - 1)
                assert (c, s) == body_ref.chord_heading(xs[:, :2], i) and abs(c * c + s * s - 1.0) < 1e-15
        k = tc.NAMES.index("point")
        assert (S[k, :, dim] == 1.0).all() and (S[k, :, dim + 1] == 0.0).all()
    # 3-D: on the corner's vertical first leg the heading is the first horizontal chord's ahead, +x
    k = tc.NAMES.index("corner")
    assert x[k, 1, 2] > x[k, 0, 2] and x[k, 1, 0] == x[k, 0, 0] and S[k, 0, 3] == 1.0 and S[k, 0, 4] == 0.0
    # along a schedule: the pose of own(k)
    c, sch, _, _ = _solved("batch")
    a = (c["x"], c["v"], c["t"], c["status"])
    R = btr.states(*a, 0.0, 30, sched=sch)
    for r in range(c["x"].shape[0]):
        if sch["status"][r] >= 2:
            assert np.isnan(R[r]).all()
        else:
            assert _bits(R[r], btr.sched_poses(*a[:3], sch, r, 0, 31))
