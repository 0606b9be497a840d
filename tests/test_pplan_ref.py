"""CPU tests of the pose planner's contract (tests/pplan_ref.py; gpis_pplan_*): the exported surface, the host
helpers against literal tables, the reference against itself (array sweeps against a heapq Dijkstra on the reversed graph, path
and projection invariants), the outcomes of the door and Z-corridor scenes, every named branch, and every defective variant
rejected by a named case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_ref
import pplan_cases as pc
import pplan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
NAMES = {"gpis_pplan_" + n for n in ("default_opts", "create", "destroy", "solve", "info", "get", "device", "paths", "path_counts", "get_paths",
                                     "project", "set_schedule")}
_memo = {}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _gap(moves="forward", H=16, variant=None, **kw):
    """(scene, problem, cost by sweeps) of the gap case, computed once per argument set."""
    key = (moves, H, variant, tuple(sorted(kw.items())))
    if key not in _memo:
        sc, pb = pc.gap_problem(moves, H, variant, **kw)
        _memo[key] = (sc, pb, pr.solve_sweep(pb))
    return _memo[key]


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import gpismap_amd
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(gpis_pplan[0-9a-z_]*)\s*\(", hdr)) == NAMES
    L = C.CDLL(gpismap_amd.LIB_PATH)        # loads without a GPU
    for n in sorted(NAMES):
        assert hasattr(L, n), n
    vp, z = C.c_void_p, (C.c_double * 16)()
    L.gpis_pplan_info.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    L.gpis_pplan_get.argtypes = [vp, vp, vp, vp]
    L.gpis_pplan_device.argtypes = [vp, vp, vp, vp]
    L.gpis_pplan_paths.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.gpis_pplan_path_counts.argtypes = [vp, vp, vp]
    L.gpis_pplan_get_paths.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gpis_pplan_project.argtypes = [vp, vp, vp]
    L.gpis_pplan_set_schedule.argtypes = [vp, C.c_int, C.c_int]
    L.gpis_pplan_solve.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.gpis_pplan_default_opts.argtypes = [C.c_float, C.c_int, vp]
    # a pose planner lives on a device, so without a handle the entries answer GPIS_ERR_ARG
    assert L.gpis_pplan_info(None, z, 14) == -1 and L.gpis_pplan_get(None, None, None, None) == -1
    assert L.gpis_pplan_device(None, None, None, None) == -1 and L.gpis_pplan_paths(None, z, 1, 8, None) == -1
    assert L.gpis_pplan_path_counts(None, None, None) == -1 and L.gpis_pplan_get_paths(None, None, None, None, None, None) == -1
    assert L.gpis_pplan_project(None, None, None) == -1 and L.gpis_pplan_set_schedule(None, 0, 0) == -1
    assert L.gpis_pplan_solve(None, None, None, z, z, 16, z, 1, None, None) == -1
    o = gpismap_amd.gpis_pplan_opts()
    assert L.gpis_pplan_default_opts(0.1, 16, C.byref(o)) == 0
    assert (o.clearance, o.margin, o.gain, o.turn, o.max_rounds) == (0.0, F32(4) * F32(0.1), 4.0, F32(0.1), 0)
    for step, H in ((0.1, 12), (0.0, 16), (float("nan"), 16), (0.1, 128)):
        assert L.gpis_pplan_default_opts(step, H, C.byref(o)) == -1
    assert L.gpis_pplan_default_opts(0.1, 16, None) == -1
    for meth in ("solve", "info", "get", "paths", "project", "device_ptrs", "set_schedule", "close"):
        assert callable(getattr(gpismap_amd.PosePlanner, meth)), meth
    assert callable(gpismap_amd.DistanceField.plan_poses) and callable(gpismap_amd.pplan_opts)
    assert gpismap_amd.pplan_opts(0.25, 8, turn=0.5).turn == 0.5
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.pplan_opts(0.25, 8, connectivity=1)


def test_heading_helpers_against_literal_tables():
    import gpismap_amd
    r = np.sqrt(0.5)
    t8 = gpismap_amd.heading_table(8)
    assert t8.dtype == np.float64 and t8.shape == (8, 2)
    assert np.array_equal(t8[[0, 2, 4, 6]], [(1, 0), (0, 1), (-1, 0), (0, -1)])                 # exact at the quarter turns
    assert np.allclose(t8[[1, 3, 5, 7]], [(r, r), (-r, r), (-r, -r), (r, -r)], rtol=0, atol=1e-15)
    t16 = gpismap_amd.heading_table(16)
    assert np.array_equal(t16[[0, 4, 8, 12]], [(1, 0), (0, 1), (-1, 0), (0, -1)])
    assert np.allclose(t16[:, 0], np.cos(np.arange(16) * np.pi / 8), rtol=0, atol=1e-15)
    assert np.allclose(t16[:, 1], np.sin(np.arange(16) * np.pi / 8), rtol=0, atol=1e-15)
    # bit k - 9 of the translation code k: 9 (-1,-1) 10 (0,-1) 11 (1,-1) 12 (-1,0) 14 (1,0) 15 (-1,1) 16 (0,1) 17 (1,1)
    E, NE, N, NW, W, SW, S, SE = (1 << 5), (1 << 8), (1 << 7), (1 << 6), (1 << 3), (1 << 0), (1 << 1), (1 << 2)
    fwd8 = [E, NE, N, NW, W, SW, S, SE]
    both8 = [E | W, NE | SW, N | S, NW | SE] * 2
    fwd16 = [E, E | NE, NE, NE | N, N, N | NW, NW, NW | W, W, W | SW, SW, SW | S, S, S | SE, SE, SE | E]
    both16 = [E | W, E | NE | W | SW, NE | SW, NE | N | SW | S, N | S, N | NW | S | SE, NW | SE, NW | W | SE | E] * 2
    for H, fwd, both in ((8, fwd8, both8), (16, fwd16, both16)):
        for mod in (gpismap_amd, pr):
            assert np.array_equal(mod.heading_moves(H, "forward"), np.array(fwd, np.uint16))
            assert np.array_equal(mod.heading_moves(H, "both"), np.array(both, np.uint16))
            assert np.array_equal(mod.heading_moves(H, "any"), np.full(H, 0x1ef, np.uint16))
            assert mod.heading_moves(H).dtype == np.uint16
    for H in pr.HS:
        assert np.array_equal(gpismap_amd.heading_table(H).view(np.uint64), pr.heading_table(H).view(np.uint64))
        for mode in ("any", "forward", "both"):
            assert np.array_equal(gpismap_amd.heading_moves(H, mode), pr.heading_moves(H, mode))
    for bad in (4, 12, 128):
        with pytest.raises(gpismap_amd.GpisError):
            gpismap_amd.heading_table(bad)
        with pytest.raises(ValueError):
            pr.heading_moves(bad)
    with pytest.raises(gpismap_amd.GpisError):
        gpismap_amd.heading_moves(8, "sideways")


def test_the_reference_rejects_bad_arguments():
    sc = pc.gap_scene()
    ok = dict(body=pc.slim(), H=8, goals=[[1.0, 1.0, -1]])
    pc.problem(sc, **ok)
    for kw in (dict(goals=[[1.0, 1.0, 0.5]]), dict(goals=[[1.0, 1.0, 8]]), dict(goals=[[1.0, 1.0, -2]]), dict(goals=[[1.0, 1.0, np.nan]]),
               dict(turn=0.1 / 65), dict(turn=1.1e3), dict(gain=2e4), dict(margin=-0.1), dict(clearance=np.inf), dict(moves=np.full(8, 16, np.uint16)),
               dict(moves=np.full(8, 512, np.uint16))):
        with pytest.raises(ValueError):
            pc.problem(sc, **dict(ok, **kw))
    for body in (body_ref.make(2, [], []), body_ref.make(3, [(0.0, 0.0, 0.0)], [0.1])):
        with pytest.raises(RuntimeError):
            pc.problem(sc, **dict(ok, body=body))
    with pytest.raises(ValueError):
        pr.Problem(sc["dist"], sc["shape"], sc["origin"], sc["step"], pc.slim(), np.zeros((8, 2)), pr.heading_moves(8), [[1.0, 1.0, -1]])
    with pytest.raises(ValueError):
        pr.Problem(sc["dist"], sc["shape"], sc["origin"], sc["step"], pc.slim(), pr.heading_table(8)[:6], pr.heading_moves(8)[:6], [[1.0, 1.0, -1]])


# ---- the reference against itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_sweeps_equal_dijkstra_on_the_reversed_graph(shape):
    nx, ny, H, m = shape
    sc = pc.shape_scene(nx, ny)
    for moves, margin in (("any", 0.0), ("forward", 0.2), ("both", 0.2)):
        pb = pc.problem(sc, pc.footprint(m), H, pc.shape_goals(nx, ny, H), moves, clearance=0.01, margin=margin, turn=0.07)
        a, b = pr.solve_sweep(pb), pr.solve_dijkstra(pb)
        assert _bits(a, b)
        assert pb.goals_given == 4 and pb.goals_dropped >= 1
        if min(nx, ny) >= 8:
            assert pb.goals_kept >= 2 and np.isfinite(a).sum() > pb.goals_kept


@pytest.mark.parametrize("moves", ["any", "forward", "both"])
def test_gap_case_sweeps_dijkstra_paths_and_projection(moves):
    sc, pb, cost = _gap(moves)
    assert _bits(cost, pr.solve_dijkstra(pb))
    pol = pr.policy(pb, cost)
    fin = np.isfinite(cost)
    assert ((pol == pr.NONE) == ~(fin & pb.free.ravel())).all() and ((pol == pr.STAY) == pb.goal.ravel()).all()
    # paths from every fifth reachable state: legal moves, strictly cheaper, ending at a goal
    S = np.flatnonzero(fin)[::5]
    H, ny, nx = pb.n3
    h, r = np.divmod(S, ny * nx)
    starts = np.concatenate([pb.world(np.stack([r % nx, r // nx], axis=1)), h[:, None].astype(F32)], axis=1)
    off, pts, hd, sc_, st = pr.paths(pb, cost, pol, starts, H * ny * nx)
    assert (st == 0).all() and _bits(sc_, cost[S])
    for k in range(S.size):
        P, Hd = pts[off[k]:off[k + 1]], hd[off[k]:off[k + 1]]
        pr.check_path_invariants(pb, cost, P, Hd)
        assert Hd[0] == h[k] and pb.goal[Hd[-1], int(round((P[-1, 1] - sc["origin"][1]) / 0.1)), int(round((P[-1, 0] - sc["origin"][0]) / 0.1))]
    # the projection: a cheaper neighbour everywhere (asserted inside), and the greedy walk ends at cost 0
    pj = pr.project(pb, cost)
    c3 = cost.reshape(pb.n3)
    assert _bits(pj["cost2"], c3.min(axis=0).ravel())
    reach = np.flatnonzero(np.isfinite(pj["cost2"]))
    assert (pj["heading2"][reach] < H).all() and (pj["heading2"][~np.isfinite(pj["cost2"])] == pr.NONE).all()
    assert _bits(c3.reshape(H, -1)[pj["heading2"][reach], reach], pj["cost2"][reach])
    for p in reach[::7]:
        w = pr.greedy_walk(pj, sc["shape"], (int(p % nx), int(p // nx)))
        assert pj["cost2"][w[-1][1] * nx + w[-1][0]] == 0
    assert pj["free"] == int(pb.free.any(axis=0).sum()) and pj["reachable"] == reach.size


@pytest.mark.parametrize("name", ["door", "z"])
@pytest.mark.parametrize("H,moves", [(8, "any"), (16, "any"), (16, "forward"), (16, "both")])
def test_scene_projection_is_walkable(name, H, moves):
    sc, pb, cost, pol, pj = pc.solved(name, H, moves)              # (project() asserts the cheaper neighbour)
    nx = sc["shape"][0]
    s = pc.lattice_index(sc, sc["start"])
    w = pr.greedy_walk(pj, sc["shape"], (s % nx, s // nx))
    assert pj["cost2"][w[-1][1] * nx + w[-1][0]] == 0 and len(w) > 20
    if (H, moves) == (16, "any"):
        assert _bits(cost, pr.solve_sweep(pb))


# ---- the two scenes' outcomes --------------------------------------------------------------------------------------------------
def test_door_pose_plan_finds_the_door_the_circumscribed_point_does_not():
    sc, pb, cost, pol, pj = pc.solved("door")
    s = pc.lattice_index(sc, sc["start"])
    assert np.isinf(pc.point_cost(sc, pc.R_OUT)[s])
    inner = pc.point_cost(sc, pc.R_IN)[s]
    assert np.isfinite(pj["cost2"][s]) and pj["cost2"][s] > inner > 0          # the body pays for turning into the door
    # the pose path from the start crosses the wall's column inside the door, lengthwise
    off, pts, hd, sc_, st = pr.paths(pb, cost, pol, [[sc["start"][0], sc["start"][1], -1]], cost.size)
    assert st[0] == 0
    pr.check_path_invariants(pb, cost, pts, hd)
    at_wall = np.abs(pts[:, 0] - 4.0) < 0.05
    assert at_wall.any() and (np.abs(pts[at_wall, 1] - 3.0) < 0.35).all()
    tab = pr.heading_table(16)
    assert (np.abs(tab[hd[at_wall], 0]) > 0.9).all()


def test_z_corridor_is_closed_to_the_body_and_open_to_the_disc():
    sc, pb, cost, pol, pj = pc.solved("z")
    s, mid = pc.lattice_index(sc, sc["start"]), pc.lattice_index(sc, sc["middle"])
    point = pc.point_cost(sc, pc.R_DISC)
    assert np.isfinite(point[mid]) and point[mid] < point[s]                   # the disc routes through the corridor
    assert np.isinf(cost.reshape(pb.n3)[:, mid // 81, mid % 81]).all()          # the middle: unreachable at every heading
    assert pb.free.reshape(16, -1)[:, mid].any()                               # (free at some heading: it is the bends that close it)
    assert np.isfinite(pj["cost2"][s]) and pj["cost2"][s] > point[s]
    # the pose path goes round: it rises above the block
    off, pts, hd, sc_, st = pr.paths(pb, cost, pol, [[sc["start"][0], sc["start"][1], -1]], cost.size)
    assert st[0] == 0 and pts[:, 1].max() > 4.5
    pr.check_path_invariants(pb, cost, pts, hd)


def test_z_closed_loop_reaches_the_goal_with_the_projection_only():
    """The reference controller with the box footprint on the Z corridor, 140 steps allowed: offered the pose plan's projected
    cost-to-go it arrives without a body hit; offered the disc-radius point plan's it is still in the corridor's mouth."""
    sc, pb, cost, pol, pj = pc.solved("z")
    good = pc.closed_loop(sc, pj["cost2"], pc.robot())
    assert good["steps"] is not None and good["steps"] <= 140 and good["hits"] == 0 and np.nanmin(good["D"]) > 0
    bad = pc.closed_loop(sc, pc.point_cost(sc, pc.R_DISC), pc.robot())
    assert bad["steps"] is None


# ---- branches ------------------------------------------------------------------------------------------------------------------
def _edge(pb, code):
    return next((e, w) for k, o, e, w in pb.edges if k == code)


def test_branch_body_half_off_the_lattice():
    sc, pb, cost = _gap()
    nan = np.isnan(pb.D)
    assert nan.any() and not pb.free[nan].any() and np.isinf(cost.reshape(pb.n3)[nan]).all()
    half = nan.any(axis=0) & pb.free.any(axis=0)          # points where the heading decides whether the body is on the lattice
    assert half.sum() > 10


def test_branch_turn_blocked_by_one_neighbour_layer():
    sc, pb, cost = _gap()
    up, dn = _edge(pb, pr.TURN_UP)[0], _edge(pb, pr.TURN_DOWN)[0]
    assert (pb.free & ~up & dn).any() and (pb.free & up & ~dn).any() and (pb.free & ~up & ~dn).any()


def test_branch_diagonal_refused_by_the_subset_rule_in_one_layer_only():
    sc, pb, cost = _gap("any")
    hit = 0
    for k, (dx, dy) in pr.TRANSLATIONS:
        if dx and dy:
            e = _edge(pb, k)[0]
            ends = pb.free & pr._shift(pb.free, (dx, dy, 0), False)       # both ends free: only the subset rule can refuse it
            hit += int(((ends & ~e).any(axis=0) & e.any(axis=0)).sum())
    assert hit > 0


def test_branch_wrap_around_between_the_last_heading_and_the_first():
    sc, pb, cost = _gap()
    pol = pr.policy(pb, cost).reshape(pb.n3)
    c3 = cost.reshape(pb.n3)
    a, b = pol[pb.H - 1] == pr.TURN_UP, pol[0] == pr.TURN_DOWN
    assert a.any() and b.any()
    w = _edge(pb, pr.TURN_UP)[1]
    assert _bits(c3[pb.H - 1][a], (c3[0] + w[pb.H - 1])[a])


def test_branch_forward_table_has_moves_without_a_reverse():
    sc, pb, cost = _gap("forward")
    one_way = 0
    for k, (dx, dy) in pr.TRANSLATIONS:
        e, back = _edge(pb, k)[0], _edge(pb, 26 - k)[0]
        one_way += int((e & ~pr._shift(back, (dx, dy, 0), False)).sum())
    assert one_way > 100
    sc, pa, _ = _gap("any")
    for k, (dx, dy) in pr.TRANSLATIONS:
        assert not (_edge(pa, k)[0] & ~pr._shift(_edge(pa, 26 - k)[0], (dx, dy, 0), False)).any()


def test_branch_goals_every_heading_some_blocked_and_dropped():
    sc, pb, cost = _gap(goal_h=-1, in_gap=True)
    # two given goals in the middle of the gap with h = -1: each keeps the free headings only; two goals are dropped
    per_goal = pb.goals_kept // 2
    assert pb.goals_given == 4 and pb.goals_dropped == 2 and 0 < per_goal < pb.H and pb.goals_kept == 2 * per_goal
    assert int(pb.goal.sum()) == per_goal and (cost[pb.goal.ravel()] == 0).all()
    sc, p0, c0 = _gap()
    assert p0.goals_kept == 2 and int(p0.goal.sum()) == 1 and p0.goals_dropped == 2


def test_branch_margin_zero_and_positive():
    sc, pb, cost = _gap()
    assert (pb.c[pb.free] >= 1).all() and (pb.c[pb.free] > 1).any() and (pb.c[~pb.free] == 0).all()
    sc, p0, c0 = _gap(margin=0.0)
    assert (p0.c[p0.free] == 1).all() and np.array_equal(p0.free, pb.free) and not _bits(c0, cost)


def test_branch_start_without_a_heading_and_every_status():
    sc, pb, cost = _gap()
    pol = pr.policy(pb, cost)
    c3 = cost.reshape(pb.n3)
    o, nx = sc["origin"], sc["shape"][0]
    p = pc.lattice_index(sc, sc["start"])
    col = c3[:, p // nx, p % nx]
    freecol = pb.free[:, p // nx, p % nx]
    hbest = int(np.flatnonzero(freecol & (col == col[freecol].min()))[0])
    unreach = np.argwhere(pb.free & np.isinf(c3))[0]
    starts = [[sc["start"][0], sc["start"][1], -1], [sc["start"][0], sc["start"][1], hbest], [-9.0, 0.0, -1], [np.nan, 0.0, 2],
              [o[0] + 1.2, o[1] + 0.3, -1], [o[0] + 1.2, o[1] + 0.3, 3], [o[0] + 0.1 * unreach[2], o[1] + 0.1 * unreach[1], unreach[0]]]
    off, pts, hd, scost, st = pr.paths(pb, cost, pol, starts, cost.size)
    assert list(st) == [0, 0, 1, 1, 2, 2, 3]
    assert hd[off[0]] == hbest and _bits(pts[off[0]:off[1]], pts[off[1]:off[2]]) and np.array_equal(hd[off[0]:off[1]], hd[off[1]:off[2]])
    assert np.isnan(scost[2:4]).all() and np.isinf(scost[4:]).all() and scost[0] == col[hbest]
    n0 = int(off[1] - off[0])
    assert n0 > 4
    off2, pts2, hd2, _, st2 = pr.paths(pb, cost, pol, starts[:2], n0 - 1)
    assert list(st2) == [4, 4] and list(np.diff(off2)) == [n0 - 1, n0 - 1] and _bits(pts2[:n0 - 1], pts[:n0 - 1])
    off3, _, _, _, st3 = pr.paths(pb, cost, pol, starts[:1], n0)
    assert st3[0] == 0 and off3[1] == n0
    with pytest.raises(ValueError):
        pr.paths(pb, cost, pol, [[1.0, 1.0, 0.5]], 10)


def test_branch_policy_ties():
    sc, pb, cost = _gap()
    br = {}
    pr.policy(pb, cost, br)
    assert br["tie_cost"] > 0 and br["tie_code"] > 0


# ---- defective variants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [v for v in pr.VARIANTS if v != "ties_code"])
def test_gap_case_rejects_the_variant(variant):
    """The gap case with the forward-only table, a goal at one heading, a margin and the asymmetric body tells every variant's
    cost from the contract's."""
    sc, pb, cost = _gap()
    _, pv, cv = _gap(variant=variant)
    assert not _bits(cv, cost), variant
    if variant in ("opposite_bit", "along"):              # these two need directed moves: the full table hides them
        _, pa, ca = _gap("any")
        assert _bits(_gap("any", variant=variant)[2], ca)
    if variant == "nan_free":
        assert pv.free.sum() > pb.free.sum()
    if variant == "cast_first":
        assert np.array_equal(pv.free, pb.free) and not _bits(pv.c, pb.c)


def test_gap_case_rejects_policy_ties_by_code_only():
    sc, pb, cost = _gap()
    _, pv, cv = _gap(variant="ties_code")
    assert _bits(cv, cost)
    assert (pr.policy(pv, cv) != pr.policy(pb, cost)).sum() > 0
