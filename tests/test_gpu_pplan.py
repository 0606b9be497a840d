"""The pose planner on the GPU (csrc/pplan.hip, gpis_pplan_*) against the numpy / heapq reference (tests/pplan_ref.py), computed
on the device's own dist grid and compared without tolerance: cost, policy, c, counts and info at every tile edge and every H,
for all three move tables; c against gpis_body_clearance; schedules and streams; pose paths; the projection into a Planner and
its consumers; lifetimes; every error code; and the closed loop on the Z corridor."""
import ctypes as C

import numpy as np
import pytest

import body_ref
import mppi_ref
import pplan_cases as pc
import pplan_ref as pr
from test_gpu_body import device_body
from test_gpu_mppi import _b, _dev, _same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U32 = np.uint32
_ENV = {}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _field(sc, df=None):
    """(DistanceField of the scene's f grid, its own dist flat)."""
    import gpismap_amd
    df = df if df is not None else gpismap_amd.DistanceField()
    df.from_grid(_dev(np.ascontiguousarray(sc["f"], F32).ravel()).data_ptr(), sc["shape"], sc["origin"], sc["step"], 0.0)
    return df, df.get()[0].ravel()


def _check(pp, pb, ref_cost=None):
    """The handle's cost, policy, c and info against the reference problem's; returns (cost, policy) of the reference."""
    rc = pr.solve_sweep(pb) if ref_cost is None else ref_cost
    rp = pr.policy(pb, rc)
    cost, pol, c = pp.get()
    assert cost.shape == pb.n3 and pol.dtype == np.uint8 and c.shape == pb.n3
    assert _bits(c, pb.c), np.argwhere(c.view(U32) != pb.c.view(U32))[:4]
    assert _bits(cost.ravel(), rc), np.argwhere(cost.ravel().view(U32) != rc.view(U32))[:4]
    assert np.array_equal(pol.ravel(), rp), np.argwhere(pol.ravel() != rp)[:4]
    inf, fin = pp.info(), np.isfinite(rc)
    assert (inf["valid"], inf["nx"], inf["ny"], inf["H"]) == (1, pb.shape[0], pb.shape[1], pb.H) and inf["step"] == pb.step
    assert (inf["goals"], inf["goals_kept"]) == (pb.goals_given, pb.goals_kept)
    assert (inf["free"], inf["reachable"]) == (int(pb.free.sum()), int(fin.sum()))
    assert F32(inf["max_cost"]) == (rc[fin].max() if fin.any() else F32(0)) and inf["rounds"] >= 1
    assert inf["tile_launches"] >= (1 if pb.goals_kept else 0) and inf["solve_ms"] >= inf["setup_ms"] >= 0
    return rc, rp


def _gap_env():
    """(scene, field, dist, Footprint, solved PosePlanner, problem, cost, policy) of the gap case, forward table, H = 16."""
    if "gap" not in _ENV:
        import gpismap_amd
        sc = pc.gap_scene()
        df, dist = _field(sc)
        fp = device_body(pc.slim())
        _, pb = pc.gap_problem("forward", 16, dist=dist)
        g = np.array([[sc["goal"][0], sc["goal"][1], 0], [sc["goal"][0], sc["goal"][1], 0], [-9.0, 0.0, -1],
                      [sc["origin"][0] + 1.2, sc["origin"][1] + 0.3, -1]], F32)
        pp = gpismap_amd.PosePlanner().solve(df, fp, g, H=16, moves="forward", **pc.GAP_OPTS)
        rc, rp = _check(pp, pb)
        _ENV["gap"] = (sc, df, dist, fp, pp, pb, rc, rp)
    return _ENV["gap"]


def _scene_env(name):
    """(scene, field, dist, Footprint, solved PosePlanner, problem, cost, policy, projection) of the door / Z problem."""
    if name not in _ENV:
        import gpismap_amd
        sc = pc.door_scene() if name == "door" else pc.z_scene()
        df, dist = _field(sc)
        assert _bits(dist, sc["dist"])                                   # the device's field is the reference's
        _, pb, rc, rp, pj = pc.solved(name)
        fp = gpismap_amd.Footprint.box(pc.ROBOT["length"], pc.ROBOT["width"], pc.ROBOT["discs"])
        pp = df.plan_poses(fp, [sc["goal"]], H=16, pose_planner=gpismap_amd.PosePlanner(), clearance=0.0, margin=0.0, turn=0.05)
        _ENV[name] = (sc, df, dist, fp, pp, pb, rc, rp, pj)
    return _ENV[name]


# ---- cost, policy, c, counts, info ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_every_shape_and_move_table(shape):
    import gpismap_amd
    nx, ny, H, m = shape
    sc = pc.shape_scene(nx, ny)
    df, dist = _field(sc)
    B = pc.footprint(m)
    fp = device_body(B)
    goals = pc.shape_goals(nx, ny, H)
    pp = gpismap_amd.PosePlanner()
    for moves, margin in (("any", 0.0), ("forward", 0.2), ("both", 0.2)):
        assert pp.solve(df, fp, goals, H=H, moves=moves, clearance=0.01, margin=margin, turn=0.07) is pp
        pb = pc.problem(sc, B, H, goals, moves, dist=dist, clearance=0.01, margin=margin, turn=0.07)
        rc, _ = _check(pp, pb)
        assert pb.goals_dropped >= 1 and pb.goals_kept >= 2
    # goals without headings: [g, 2] rows stand for h = -1
    pp.solve(df, fp, goals[:1, :2], H=H, clearance=0.01, margin=0.0, turn=0.07)
    _check(pp, pc.problem(sc, B, H, goals[:1], "any", dist=dist, clearance=0.01, margin=0.0, turn=0.07))


@pytest.mark.parametrize("name", ["door", "z"])
def test_both_scenes(name):
    sc, df, dist, fp, pp, pb, rc, rp, pj = _scene_env(name)
    _check(pp, pb, rc)
    s = pc.lattice_index(sc, sc["start"])
    got = pp.get()[0].reshape(16, -1)[:, s].min()
    assert np.isfinite(got) and got == pj["cost2"][s]
    if name == "z":
        assert np.isinf(pp.get()[0].reshape(16, -1)[:, pc.lattice_index(sc, sc["middle"])]).all()
    assert pp.info()["rounds"] > 3


def test_c_is_the_float_of_gpis_body_clearance():
    sc, df, dist, fp, pp, pb, rc, rp = _gap_env()
    H, ny, nx = pb.n3
    X = (F32(sc["origin"][0]) + np.arange(nx, dtype=F32) * F32(sc["step"])).astype(F64)
    Y = (F32(sc["origin"][1]) + np.arange(ny, dtype=F32) * F32(sc["step"])).astype(F64)
    tab = pr.heading_table(H)
    S = np.zeros((H, ny, nx, 4), F64)
    S[..., 0], S[..., 1] = X[None, None, :], Y[None, :, None]
    S[..., 2], S[..., 3] = tab[:, 0][:, None, None], tab[:, 1][:, None, None]
    D = fp.clearance(df, S.reshape(-1, 4))["D"].reshape(pb.n3)
    assert np.array_equal(np.isnan(D), np.isnan(pb.D)) and np.array_equal(D[~np.isnan(D)].view(np.uint64), pb.D[~np.isnan(D)].view(np.uint64))
    o = pc.GAP_OPTS
    with np.errstate(invalid="ignore"):
        d = D.astype(F32)
        free = d >= F32(o["clearance"])
        t = np.maximum(F32(0), F32(o["margin"]) - (d - F32(o["clearance"]))) / F32(o["margin"])
        c = np.where(free, F32(1) + F32(o["gain"]) * (t * t), F32(0)).astype(F32)
    assert _bits(pp.get()[2], c) and (c[np.isnan(D)] == 0).all() and np.isnan(D).any()


def test_result_does_not_depend_on_schedule_or_stream():
    import gpismap_amd
    import torch
    sc, df, dist, fp, pp0, pb, rc, rp = _gap_env()
    g = np.array([[sc["goal"][0], sc["goal"][1], 0]], F32)
    pp = gpismap_amd.PosePlanner()
    st = torch.cuda.Stream()
    rounds = {}
    for sched, stream in (((1, 1), 0), ((3, 2), 0), ((0, 0), 0), ((0, 0), st.cuda_stream), ((2, 3), st.cuda_stream)):
        pp.set_schedule(*sched)
        pp.solve(df, fp, g, H=16, moves="forward", stream=stream, **pc.GAP_OPTS)
        cost, pol, c = pp.get()
        assert _bits(cost.ravel(), rc) and np.array_equal(pol.ravel(), rp) and _bits(c, pb.c), (sched, stream)
        rounds[(sched, stream)] = pp.info()["rounds"]
    assert rounds[((1, 1), 0)] > rounds[((0, 0), 0)]                 # one sweep per round: the cap was met and the tiles re-ran
    with pytest.raises(gpismap_amd.GpisError):
        pp.set_schedule(-1, 0)


# ---- pose paths ----------------------------------------------------------------------------------------------------------------
def _starts(sc, pb, rc, m, seed=5):
    """m starts over the scene and a little beyond it, headings from -1 .. H - 1; the first few are fixed: the scene's start
    without a heading, a point outside, a NaN, a point inside the wall, a free state that cannot reach the goal."""
    rng = np.random.default_rng(seed)
    o, nx, ny = sc["origin"], sc["shape"][0], sc["shape"][1]
    S = np.zeros((m, 3), F32)
    S[:, 0] = rng.uniform(o[0] - 0.2, o[0] + 0.1 * (nx - 1) + 0.2, m)
    S[:, 1] = rng.uniform(o[1] - 0.2, o[1] + 0.1 * (ny - 1) + 0.2, m)
    S[:, 2] = rng.integers(-1, pb.H, m)
    un = np.argwhere(pb.free & np.isinf(rc.reshape(pb.n3)))[0]
    fixed = [(sc["start"][0], sc["start"][1], -1), (-9.0, 0.0, -1), (np.nan, 0.0, 2), (o[0] + 1.2, o[1] + 0.3, -1),
             (o[0] + 0.1 * un[2], o[1] + 0.1 * un[1], un[0])]
    S[:min(m, 5)] = fixed[:min(m, 5)]
    return S


def _paths_equal(got, ref):
    P, Hd, sc_, st = got
    off, pts, hd, rsc, rst = ref
    assert np.array_equal(st, rst) and len(P) == rst.size
    assert np.array_equal(np.isnan(sc_), np.isnan(rsc)) and _bits(np.nan_to_num(sc_, nan=-1.0), np.nan_to_num(rsc, nan=-1.0))
    for k in range(rst.size):
        assert _bits(P[k], pts[off[k]:off[k + 1]]) and np.array_equal(Hd[k], hd[off[k]:off[k + 1]]), k


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_pose_paths(m):
    sc, df, dist, fp, pp, pb, rc, rp = _gap_env()
    S = _starts(sc, pb, rc, m)
    ref = pr.paths(pb, rc, rp, S, rc.size)
    got = pp.paths(S)
    _paths_equal(got, ref)
    off1 = pp.last_off.copy()
    assert np.array_equal(off1, ref[0])
    pp.paths(S)
    assert np.array_equal(pp.last_off, off1)                         # the same offsets on every run
    if m >= 65:
        assert set(ref[4].tolist()) == {0, 1, 2, 3}
        k = int(np.flatnonzero(ref[4] == 0)[0])
        pr.check_path_invariants(pb, rc, got[0][k], got[1][k])
        # cut-offs: a limit below the longest path gives status 4 with the points so far; at the length itself the path arrives
        longest = int(np.diff(ref[0]).max())
        for cap in (2, longest - 1, longest):
            _paths_equal(pp.paths(S, max_points=cap), pr.paths(pb, rc, rp, S, cap))
        assert (pr.paths(pb, rc, rp, S, longest - 1)[4] == 4).any() and not (pr.paths(pb, rc, rp, S, longest)[4] == 4).any()


# ---- the projection ------------------------------------------------------------------------------------------------------------
def test_project_against_the_reference_and_its_consumers():
    import gpismap_amd
    sc, df, dist, fp, pp, pb, rc, rp, pj = _scene_env("z")
    pl = pp.project()
    assert isinstance(pl, gpismap_amd.Planner)
    cost2, pol2 = pl.get()
    assert _bits(cost2.ravel(), pj["cost2"]) and np.array_equal(pol2.ravel(), pj["policy2"])
    assert np.array_equal(pp.heading2.ravel(), pj["heading2"])
    i, j = pl.info(), pp.info()
    assert (i["valid"], i["dim"], i["nx"], i["ny"], i["nz"]) == (1, 2, 81, 61, 1) and i["step"] == F32(0.1)
    assert (i["free"], i["reachable"]) == (pj["free"], pj["reachable"]) and F32(i["max_cost"]) == pj["max_cost"]
    assert all(i[k] == j[k] for k in ("goals", "goals_kept", "rounds", "tile_launches", "solve_ms"))
    # Planner.paths walks the projection as the reference's greedy walk does
    nx = sc["shape"][0]
    starts = np.array([sc["start"], (7.5, 5.5), (0.7, 0.8), sc["middle"], (3.5, 1.0)], F32)     # .., unreachable, inside the block
    P, scost, st = pl.paths(starts)
    assert list(st) == [0, 0, 0, 3, 2]
    for k in range(3):
        p = pc.lattice_index(sc, starts[k])
        w = np.array(pr.greedy_walk(pj, sc["shape"], (p % nx, p // nx)), np.int64)
        assert _bits(P[k], pb.world(w)) and scost[k] == pj["cost2"][p]
    # the smoother takes the projected handle
    t = pl.trajectories(N=32)
    t.optimize(df, clearance=0.0)
    assert t.get()["x"].shape == (5, 32, 2)
    # a second projection into the same handle, after another solve, replaces the first
    sd, dfd, _, fpd, ppd, pbd, _, _, pjd = _scene_env("door")
    assert ppd.project(pl) is pl
    assert _bits(pl.get()[0].ravel(), pjd["cost2"]) and np.array_equal(pl.get()[1].ravel(), pjd["policy2"])


def test_controller_step_with_the_projection_equals_the_reference_step():
    import gpismap_amd
    sc, df, dist, fp, pp, pb, rc, rp, pj = _scene_env("z")
    pl = pp.project()
    B = pc.robot()
    o = mppi_ref.default_opts(2, sc["step"])
    o.update(pc.LOOP["opts"], clearance=0.0)
    K, T, seed = 257, 20, 3
    ctl = gpismap_amd.Controller()
    ctl.init(2, K, T, seed=seed)
    pose = mppi_ref.pose_of_state(np.array([sc["start"][0], sc["start"][1], 1.0, 0.0]), 2)
    before = ctl.get()
    u0, info = df.control(ctl, pose, planner=pl, footprint=fp, **o)
    g = ctl.get()
    args = (dist, sc["shape"], sc["origin"], sc["step"], pose, before["U"], seed, 1)
    r = body_ref.roll(*args, K, o, pj["cost2"], None, body=B)
    _same_bits(g["J"], r["J"], "J")
    assert np.array_equal(g["hits"], r["hits"]) and _b(info["Jmin"]) == _b(r["Jmin"]) and info["best"] == r["best"]
    dq = np.abs(g["q"].astype(np.int64) - r["q"].astype(np.int64))
    assert dq.max() <= 1                                             # the weights' one exp: at most 1 in 2^32
    f = body_ref.finish(r, g["q"], *args, o, pj["cost2"], None, body=B)
    _same_bits(g["U"], f["U"], "the new sequence")
    _same_bits(u0, f["u0"], "u0")
    _same_bits(g["nominal_states"], f["nominal_states"], "nominal states")
    assert r["branches"]["term_cost"] > 0


def test_projected_handle_outlives_everything():
    import gpismap_amd
    sc = pc.gap_scene()
    df, dist = _field(sc)
    fp = device_body(pc.slim())
    _, pb = pc.gap_problem("any", 16, dist=dist)
    g = np.array([[sc["goal"][0], sc["goal"][1], 0]], F32)
    pp = gpismap_amd.PosePlanner().solve(df, fp, g, H=16, **pc.GAP_OPTS)
    rc = pr.solve_sweep(pb)
    pj = pr.project(pb, rc)
    pl = pp.project()
    # the pose plan outlives its field and its footprint
    fp.close()
    df.close()
    assert _bits(pp.get()[0].ravel(), rc)
    P, Hd, scost, st = pp.paths([sc["start"]])
    assert st[0] == 0
    pr.check_path_invariants(pb, rc, P[0], Hd[0])
    # the projection outlives the pose planner
    pp.close()
    assert _bits(pl.get()[0].ravel(), pj["cost2"]) and np.array_equal(pl.get()[1].ravel(), pj["policy2"])
    P2, _, st2 = pl.paths([sc["start"]])
    assert st2[0] == 0 and len(P2[0]) > 3 and pl.info()["reachable"] == pj["reachable"]


# ---- lifetime and reuse --------------------------------------------------------------------------------------------------------
def test_one_handle_through_changing_shapes_and_headings():
    import gpismap_amd
    pp, pl = gpismap_amd.PosePlanner(), gpismap_amd.Planner()
    for nx, ny, H, m in (pc.SHAPES[1], pc.SHAPES[5], pc.SHAPES[0], pc.SHAPES[4], pc.SHAPES[2]):       # grow, shrink, grow
        sc = pc.shape_scene(nx, ny)
        df, dist = _field(sc)
        B = pc.footprint(m)
        goals = pc.shape_goals(nx, ny, H)
        pp.solve(df, device_body(B), goals, H=H, moves="both", clearance=0.01, margin=0.2, turn=0.07)
        pb = pc.problem(sc, B, H, goals, "both", dist=dist, clearance=0.01, margin=0.2, turn=0.07)
        rc, rp = _check(pp, pb)
        pj = pr.project(pb, rc)
        assert pp.project(pl) is pl
        assert _bits(pl.get()[0].ravel(), pj["cost2"]) and np.array_equal(pl.get()[1].ravel(), pj["policy2"])
        assert pl.info()["nx"] == nx and pl.info()["free"] == pj["free"]
        S = np.concatenate([goals, [[sc["origin"][0] + 0.1 * (nx - 2), sc["origin"][1] + 0.1 * (ny - 2), -1]]]).astype(F32)
        P, Hd, scost, st = pp.paths(S)
        ref = pr.paths(pb, rc, rp, S, rc.size)
        assert np.array_equal(st, ref[4]) and np.array_equal(pp.last_off, ref[0])


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_code_and_the_result_survives():
    import gpismap_amd
    sc, df, dist, fp, pp0, pb, rc, rp = _gap_env()
    L = gpismap_amd.lib()
    pp = gpismap_amd.PosePlanner()
    tab, mv = pr.heading_table(16), pr.heading_moves(16, "forward")
    goals = np.array([[sc["goal"][0], sc["goal"][1], 0]], F32)

    def solve(p=pp, f=df, b=fp, tab=tab, mv=mv, H=16, goals=goals, n=None, **kw):
        o = gpismap_amd.pplan_opts(sc["step"], 16, **dict(pc.GAP_OPTS, **kw))
        tab, mv, goals = np.ascontiguousarray(tab, F64), np.ascontiguousarray(mv, np.uint16), np.ascontiguousarray(goals, F32)
        return L.gpis_pplan_solve(p.h if p else None, f.h if f else None, b.h if b else None, tab.ctypes.data_as(C.POINTER(C.c_double)),
                                  mv.ctypes.data_as(C.POINTER(C.c_ushort)), H, goals.ctypes.data_as(C.POINTER(C.c_float)),
                                  goals.shape[0] if n is None else n, C.byref(o), None)

    assert solve() == 0

    def still_there(what):
        cost, pol, c = pp.get()
        assert _bits(cost.ravel(), rc) and np.array_equal(pol.ravel(), rp), what

    ARG, STATE, LIMIT = -1, -3, -4
    sc3 = dict(f=np.ones(27, F32) * np.where(np.arange(27) == 13, -1, 1), shape=(3, 3, 3), origin=(0.0, 0.0, 0.0), step=0.1)
    df3, _ = _field(sc3)
    bad_tab, zero_tab, bad_mv = tab.copy(), tab.copy(), mv.copy()
    bad_tab[3, 1], zero_tab[5], bad_mv[2] = np.nan, (0.0, 0.0), mv[2] | 16
    for what, rc_, kw in (("no handle", ARG, dict(p=None)), ("no field", ARG, dict(f=None)), ("no footprint", ARG, dict(b=None)),
                          ("no goals", ARG, dict(n=0)), ("a 3-D field", ARG, dict(f=df3)), ("H = 12", ARG, dict(H=12)), ("H = 128", ARG, dict(H=128)),
                          ("a NaN heading", ARG, dict(tab=bad_tab)), ("a zero heading", ARG, dict(tab=zero_tab)),
                          ("the stay bit", ARG, dict(mv=bad_mv)), ("a NaN clearance", ARG, dict(clearance=np.nan)),
                          ("an infinite margin", ARG, dict(margin=np.inf)), ("a negative gain", ARG, dict(gain=-1.0)), ("gain > 1e4", ARG, dict(gain=2e4)),
                          ("a NaN turn", ARG, dict(turn=np.nan)), ("turn < step / 64", ARG, dict(turn=0.001)), ("turn > 1e4 step", ARG, dict(turn=1.1e3)),
                          ("max_rounds < 0", ARG, dict(max_rounds=-1)), ("goal heading 0.5", ARG, dict(goals=[[1.0, 1.0, 0.5]])),
                          ("goal heading 16", ARG, dict(goals=[[1.0, 1.0, 16]])), ("goal heading -2", ARG, dict(goals=[[1.0, 1.0, -2]])),
                          ("goal heading NaN", ARG, dict(goals=[[1.0, 1.0, np.nan]])),
                          ("an empty footprint", STATE, dict(b=gpismap_amd.Footprint(2).set(np.zeros((0, 2)), [])),),
                          ("a 3-D footprint", STATE, dict(b=gpismap_amd.Footprint(3).set([(0.0, 0.0, 0.0)], [0.1]))),
                          ("a field without a result", STATE, dict(f=gpismap_amd.DistanceField()))):
        assert solve(**kw) == rc_, what
        still_there(what)
    # nx ny H > 2^28
    big = dict(f=np.ones(2049 * 2049, F32), shape=(2049, 2049), origin=(0.0, 0.0), step=0.1)
    big["f"][5] = -1.0
    dfb, _ = _field(big)
    assert solve(f=dfb, H=64, tab=pr.heading_table(64), mv=pr.heading_moves(64)) == LIMIT
    assert solve(f=dfb, H=32, tab=pr.heading_table(32), mv=pr.heading_moves(32), goals=[[1.0, 1.0, 40]]) == ARG
    still_there("too many states")
    # paths: arguments, state, limit
    x = np.array([[sc["start"][0], sc["start"][1], -1]], F32)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))
    assert L.gpis_pplan_paths(pp.h, None, 1, 8, None) == ARG and L.gpis_pplan_paths(pp.h, xp, 0, 8, None) == ARG
    assert L.gpis_pplan_paths(pp.h, xp, 1, 1, None) == ARG and L.gpis_pplan_paths(pp.h, xp, (1 << 24) + 1, 8, None) == LIMIT
    bad = np.array([[1.0, 1.0, 16]], F32)
    assert L.gpis_pplan_paths(pp.h, bad.ctypes.data_as(C.POINTER(C.c_float)), 1, 8, None) == ARG
    assert L.gpis_pplan_path_counts(pp.h, None, None) == STATE
    assert L.gpis_pplan_get_paths(pp.h, None, None, None, None, None) == STATE
    assert L.gpis_pplan_paths(pp.h, xp, 1, 4096, None) == 0 and L.gpis_pplan_path_counts(pp.h, None, None) == 0
    fresh = gpismap_amd.PosePlanner()
    assert L.gpis_pplan_paths(fresh.h, xp, 1, 8, None) == STATE and L.gpis_pplan_get(fresh.h, None, None, None) == STATE
    assert L.gpis_pplan_project(fresh.h, gpismap_amd.Planner().h, None) == STATE and L.gpis_pplan_project(pp.h, None, None) == ARG
    assert fresh.device_ptrs() == (0, 0, 0) and all(pp.device_ptrs()) and fresh.info()["valid"] == 0
    with pytest.raises(gpismap_amd.GpisError):
        fresh.get()
    # max_rounds exceeded: GPIS_ERR_LIMIT and no result
    pp.set_schedule(1, 1)
    assert solve(max_rounds=2) == LIMIT
    assert pp.info()["valid"] == 0 and L.gpis_pplan_get(pp.h, None, None, None) == STATE
    pp.set_schedule(0, 0)
    assert solve() == 0
    still_there("after the round cap")


# ---- the closed loop -----------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_z_corridor_on_the_device():
    """The CPU scenario of tests/test_pplan_ref.py through Controller, with its acceptance: behaviour, not bits (a q may differ by
    one from the reference's own run)."""
    import gpismap_amd
    sc, df, dist, fp, pp, pb, rc, rp, pj = _scene_env("z")
    projected = pp.project()
    point = df.plan([sc["goal"]], planner=gpismap_amd.Planner(), clearance=pc.R_DISC, margin=0.0)
    assert _bits(point.get()[0].ravel(), pc.point_cost(sc, pc.R_DISC))

    def loop(planner):
        ctl = gpismap_amd.Controller()
        ctl.init(2, pc.LOOP["K"], pc.LOOP["T"], seed=pc.LOOP["seed"])

        def step_fn(pose, o):
            u0, _ = df.control(ctl, pose, planner=planner, footprint=fp, **o)
            ctl.shift()
            return u0

        return pc.closed_loop(sc, None, pc.robot(), step_fn=step_fn)

    good, bad = loop(projected), loop(point)
    for name, r in (("projected pose plan", good), ("point plan, disc radius", bad)):
        print("%s: %s steps, least body clearance %.3f, %d driven states with the body in the wall" % (name, r["steps"], np.nanmin(r["D"]), r["hits"]))
    assert good["steps"] is not None and good["steps"] <= 140 and good["hits"] == 0 and np.nanmin(good["D"]) > 0
    assert bad["steps"] is None
