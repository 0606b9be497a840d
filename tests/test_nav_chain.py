"""The chained round of tests/nav_chain.py reaches what it is there for, asserted on the references alone before the device sees
anything: conditions the scene, the pose and the balls were chosen to meet, not measurements.  The device test
(tests/test_gpu_nav_chain.py) asserts the same conditions again on the device's data through conditions()."""
import time

import numpy as np
import pytest

import nav_chain as nc
import plan_ref
import pplan_cases as pc

_ROUND = {}


def _round(dim):
    if dim not in _ROUND:
        t0 = time.process_time()
        r = nc.run(dim)
        _ROUND[dim] = (r, time.process_time() - t0)
    return _ROUND[dim]


# ---- the conditions, per stage: the device test calls these on its own data ----------------------------------------------------
def check_frame(r):
    st = r["frame"]["status"]
    assert (st == 0).any() and (st != 0).any(), np.bincount(st)


def check_cover(r):
    c, cv = r["cfg"], r["cover"]
    seen, rd = np.asarray(cv["seen"]).ravel() != 0, cv["restricted"]
    assert seen.any() and not seen.all()
    assert cv["frontiers"]["label"].size >= 1
    # a point on the unseen_dist plateau next to a point that kept its true distance
    nz = c["shape"][2] if c["dim"] == 3 else 1
    g = rd.reshape(nz, c["shape"][1], c["shape"][0])
    s3 = seen.reshape(g.shape)
    plateau = (g == np.float32(cv["unseen_dist"])) & ~s3
    true = s3 & (g != np.float32(cv["unseen_dist"]))
    pairs = sum(int((np.take(plateau, range(0, g.shape[a] - 1), axis=a) & np.take(true, range(1, g.shape[a]), axis=a)).sum()) +
                int((np.take(true, range(0, g.shape[a] - 1), axis=a) & np.take(plateau, range(1, g.shape[a]), axis=a)).sum()) for a in range(3))
    assert pairs > 0


def check_plan(r):
    p = r["plan"]
    assert p["status"][0] == 0 and np.isfinite(p["start_cost"][0])
    assert (p["status"] != 0).any(), p["status"]
    assert np.isinf(p["cost"]).any() and np.isfinite(p["cost"]).any()


def check_pplan(r):
    c, p, q = r["cfg"], r["plan"], r["pplan"]
    assert q["status"][0] == 0 and np.isfinite(q["start_cost"][0])
    s = pc.lattice_index(c, nc.start_point(c))
    at_start = q["cost"].reshape(c["H"], -1)[:, s].min()
    assert at_start == q["start_cost"][0] and at_start > p["cost"][s], (at_start, p["cost"][s])
    # the projection's heading along the start's pose path
    pts = q["points"][q["off"][0]:q["off"][1]]
    h2 = q["projection"]["heading2"].ravel()[[pc.lattice_index(c, x) for x in pts]]
    assert np.unique(h2).size >= 2, h2


def check_traj(r):
    t = r["traj"]
    st = t["result"]["status"]
    assert (st == 0).any() and (st != 0).any(), st
    col = t["clearance"]["collides"]
    assert (col == 1).any() and (col == 0).any(), col


def check_timing(r):
    t = r["timing"]
    assert t["timing"]["status"][0] == 0 and np.unique(t["timing"]["limiter"][0]).size >= 2
    assert t["check"]["collides"][0] == 1 and (t["check"]["collides"][1:] == 0).any(), t["check"]["collides"]
    assert t["obst"]["n"] == 3 and t["check"]["min_obstacle"][0] == 0


def check_control(r):
    assert len(r["control"]["steps"]) == 2
    for s in r["control"]["steps"]:
        f, br = s["finish"], s["roll"]["branches"]
        assert 0 < f["ndyn"] < nc.K, f["ndyn"]
        assert br["dyn_col"] > 0 and br["col"] > 0 and br["second_ball_nearer"] > 0 and br["term_cost"] > 0, br
        assert s["body_only"] > 0
        assert 1.0 < f["neff"] < nc.K, f["neff"]


def check_localise(r):
    l = r["localise"]
    assert 1.0 < l["filter"]["neff"] < nc.PARTICLES, l["filter"]["neff"]
    o = nc.track_field_ref.opts(r["cfg"]["dim"], **r["cfg"]["track"])
    assert l["track"]["inliers"] >= o.min_inliers and l["track"]["status"] in (0, 1), (l["track"]["inliers"], l["track"]["status"])
    assert l["grid"].shape[0] >= nc.POSES


CHECKS = dict(frame=check_frame, cover=check_cover, plan=check_plan, pplan=check_pplan, traj=check_traj, timing=check_timing,
              control=check_control, localise=check_localise)


def conditions(r, name):
    """The conditions of stage `name` on the round r (the stages up to it present); no-op for a stage without any."""
    if name in CHECKS:
        CHECKS[name](r)


# ---- tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_round_reaches_every_branch_it_is_there_for(dim):
    r, cpu = _round(dim)
    assert set(r) == set(nc.stages_of(dim)) | {"cfg"}
    for name in nc.stages_of(dim):
        conditions(r, name)
    print("dim %d: %.2f s of CPU" % (dim, cpu))
    assert cpu < 20.0, cpu


@pytest.mark.parametrize("dim", [2, 3])
def test_the_lattice_and_the_shapes_are_the_ones_the_round_is_specified_with(dim):
    c = nc.config(dim)
    if dim == 2:
        assert c["shape"][0] <= 81 and c["shape"][1] <= 61 and c["H"] == 16 and c["body"]["m"] == 5 and c["thetas"] is nc.hc.TH90
        assert np.array_equal(c["body"]["b"], pc.robot()["b"])
    else:
        assert c["shape"] == nc.hc.SMALL3["shape"] and c["body"]["m"] == 3 and c["cam"][4] <= 64 and c["cam"][5] <= 48
    assert (nc.K, nc.T, nc.N, nc.PARTICLES, nc.POSES) == (257, 33, 33, 257, 300)
    r, _ = _round(dim)
    assert r["plan"]["starts"].shape[0] == 6 and r["traj"]["result"]["x"].shape[:2] == (6, nc.N)
    assert r["timing"]["controls"]["U"].shape[1] == nc.T and r["control"]["steps"][0]["roll"]["J"].size == nc.K
    assert r["view"]["poses"].shape[0] == 8 * r["cover"]["reps"].shape[0]


@pytest.mark.parametrize("dim", [2, 3])
def test_sweep_and_dijkstra_agree_on_the_restricted_field(dim):
    """As tests/test_plan_ref.py holds the two solvers to one another, here on a field with a plateau and an inf wall."""
    r, _ = _round(dim)
    sweep = plan_ref.solve_sweep(r["plan"]["pb"])
    assert np.array_equal(sweep.view(np.uint32), r["plan"]["cost"].view(np.uint32))
    for k in np.flatnonzero(r["plan"]["status"] == 0):
        plan_ref.check_path_invariants(r["plan"]["pb"], r["plan"]["cost"], r["plan"]["points"][r["plan"]["off"][k]:r["plan"]["off"][k + 1]])


def test_hooks_replace_what_a_stage_hands_on():
    """run() hands the next stage what a hook returned: the mechanism the device test relies on."""
    seen = {}

    def frame(r, out):
        return dict(out, meas=np.full_like(out["meas"], 0.5))

    def cover(r, out):
        seen["meas"] = r["frame"]["meas"].copy()
        seen["n"] = int(out["seen"].sum())

    r = nc.run(2, stages=("field", "frame", "cover"), hooks=dict(frame=frame, cover=cover))
    assert np.all(seen["meas"] == np.float32(0.5)) and seen["n"] != int(_round(2)[0]["cover"]["seen"].sum())
    assert "view" not in r and r["cover"]["seen"].sum() == seen["n"]
