"""Smoothing for the robot's footprint on the GPU (traj_opt_kernel<DIM, true> of csrc/traj.hip, gpis_smooth_*,
gpis_smooth_from_pose_paths) against the numpy reference (tests/traj_body_ref.py) on the device's own dist, bit for
bit and NaN for NaN: the waypoints, status, iterations, the four float and two integer results and the fused body result."""
import ctypes as C
import functools

import numpy as np
import pytest

import body_ref
import traj_body_cases as tbc
import traj_body_ref as tb
import traj_cases
import traj_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
U32 = np.uint32
KEYS = ("x", "status", "iterations", "length", "smooth", "obstacle", "min_dist", "nonfinite", "collides")
BODY = (("D_min", "D_min"), ("waypoint", "waypoint"), ("ball", "ball"), ("collides", "body_collides"))
ARG, STATE = -1, -3


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U32) if a.dtype == F32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _equal(got, body, ref, what=""):
    for k in KEYS:
        u, v = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k, u.dtype, v.dtype)
        assert np.array_equal(_bits(u), _bits(v)), (what, k, np.flatnonzero((_bits(u) != _bits(v)).reshape(u.shape[0], -1).any(axis=1))[:8])
    for kg, kr in BODY:
        u, v = np.ascontiguousarray(body[kg]), np.ascontiguousarray(ref[kr])
        assert u.dtype == v.dtype and np.array_equal(_bits(u), _bits(v)), (what, kg, u[:8], v[:8])


@functools.lru_cache(maxsize=None)
def _env():
    """name -> (field description, DistanceField, the device's own dist)."""
    import gpismap_amd
    out = {}
    for name, f in tbc.fields().items():
        df = gpismap_amd.DistanceField()
        df.from_grid(_dev(np.ascontiguousarray(f["f"], F32).ravel()).data_ptr(), f["shape"], f["origin"], f["step"], 0.0)
        out[name] = (f, df, df.get()[0].ravel())
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in tbc.all_cases({k: v[2] for k, v in _env().items()})}


def _footprint(B):
    import gpismap_amd
    return gpismap_amd.Footprint(B["dim"]).set(B["b"], B["rho"])


def _opts(f, B, **kw):
    import gpismap_amd
    o, wt = gpismap_amd.traj_body_opts(len(f["shape"]), F32(f["step"]), B["m"], **kw)
    return {k: getattr(o, k) for k in traj_ref.OPT_NAMES}, wt


def _ref(c, x=None):
    f, df, dist = _env()[c["scene"]]
    o, _ = _opts(f, c["body"], **c["opts"])
    return tb.optimize(dist, f["shape"], f["origin"], f["step"], c["body"], c["x"] if x is None else x, None, o, c["w_turn"])


def _run(c, tj, x=None):
    f, df, dist = _env()[c["scene"]]
    df.smooth(c["x"] if x is None else x, trajectories=tj, footprint=_footprint(c["body"]), w_turn=float(c["w_turn"]), **c["opts"])
    return tj.get(), tj.body_result()


def _names():
    sizes = [(d, N, b, w) for d in (2, 3) for i, N in enumerate(tbc.NS) for b in (("one", "two", "sixteen", "asym", "zero2") if N == 64 else
                                                                                   (("one", "two", "sixteen", "asym")[i % 4],)) for w in (0, 1)]
    return ["hand%d_N%d_%s_w%d" % s for s in sizes] + ["hand2_iters0", "hand3_iters0", "repeated_w0", "repeated_w1", "leaving", "door_N32", "door_N64",
                                                       "door_N128", "door_mix"]


@pytest.mark.parametrize("name", _names())
def test_case_against_the_reference(name):
    """Every waypoint count around the wavefront edges, 1 / 2 / 16 balls and the asymmetric body, w_turn 0 and 1, iters = 0, zero
    chords, trajectories that leave the lattice, the door with the defaults, a batch whose members stop at different
    iterations and hold a status-2 member."""
    import gpismap_amd
    assert sorted(_names()) == sorted(_cases())
    c = _cases()[name]
    got, body = _run(c, gpismap_amd.Trajectories())
    ref = _ref(c)
    _equal(got, body, ref, name)
    if name == "door_mix":
        assert len(set(ref["iterations"].tolist())) >= 4 and ref["status"][3] == 2 and np.isnan(body["D_min"][3]) and body["waypoint"][3] == -1
    if name == "leaving":
        assert np.isnan(body["D_min"][1]) and body["collides"].tolist() == [1, 1] and got["status"][1] != 2
    if name.startswith("door_N"):
        assert body["D_min"][0] >= 0 and body["collides"][0] == 0
    if name.endswith("iters0"):
        assert np.all(got["iterations"] == 0) and np.array_equal(got["x"].view(U32), c["x"].view(U32))


def test_large_batch_and_position_independence():
    import gpismap_amd
    f, df, dist = _env()["balls2"]
    c = tbc.batch_case(dist)
    tj = gpismap_amd.Trajectories()
    got, body = _run(c, tj)
    ref = _ref(c)
    _equal(got, body, ref, "batch")
    assert got["status"][17] == 2 and got["x"].shape[0] == 600
    # trajectory 5 alone, and at the first, a middle and the last place of a batch of seven
    one, bone = _run(c, tj, c["x"][5:6])
    for k in KEYS:
        assert np.array_equal(_bits(one[k]), _bits(got[k][5:6])), k
    for kg, _ in BODY:
        assert np.array_equal(_bits(bone[kg]), _bits(body[kg][5:6])), kg
    for pos in (0, 3, 6):
        idx = [17, 40, 41, 42, 43, 44, 45]
        idx[pos] = 5
        g7, b7 = _run(c, tj, c["x"][idx])
        for k in KEYS:
            assert np.array_equal(_bits(g7[k]), _bits(got[k][idx])), (pos, k)
        for kg, _ in BODY:
            assert np.array_equal(_bits(b7[kg]), _bits(body[kg][idx])), (pos, kg)


@pytest.mark.parametrize("dim", [2, 3])
def test_zero_footprint_equals_the_point_path_on_the_device(dim):
    import gpismap_amd
    f, df, dist = _env()["balls%d" % dim]
    x, o, _ = traj_cases.hand_made(traj_cases.scene(dim), dist, 65)
    tj = gpismap_amd.Trajectories()
    base = df.smooth(x, trajectories=tj, iters=12, **o).get()
    with pytest.raises(gpismap_amd.GpisError):
        tj.body_result()                                                          # the point path leaves no body result
    zero = _footprint(body_ref.point(dim))
    for wt in (0.0, 1.0):
        got = df.smooth(x, trajectories=tj, footprint=zero, w_turn=wt, iters=12, **o).get()
        for k in KEYS:
            assert np.array_equal(_bits(got[k]), _bits(base[k])), (wt, k)
        b = tj.body_result()
        ref = tj.body_clearance(zero, df, clearance=float(F32(o["clearance"])))
        for k in ref:
            assert np.array_equal(_bits(b[k]), _bits(ref[k])), k
    # one call of the point path after a body call on the same handle: the bits are unchanged
    again = df.smooth(x, trajectories=tj, iters=12, **o).get()
    for k in KEYS:
        assert np.array_equal(_bits(again[k]), _bits(base[k])), k


def test_body_result_is_a_result():
    """time / controls / body_clearance / device_ptrs work on a body result as on any other, and body_clearance on it returns
    the fused body result."""
    import gpismap_amd
    f, df, dist = _env()["door"]
    c = _cases()["door_mix"]
    tj = gpismap_amd.Trajectories()
    got, body = _run(c, tj)
    fp = _footprint(c["body"])
    chk = tj.body_clearance(fp, df, clearance=0.0)
    for k in chk:
        assert np.array_equal(_bits(chk[k]), _bits(body[k])), k
    tm = tj.time(df)
    assert tm["status"].tolist() == [0, 0, 0, 2] and np.all(tm["duration"][:3] > 0)
    U, h0, p0, cl = tj.controls(0.25, 16)
    assert U.shape == (4, 16, 2) and np.isfinite(U).all() and np.array_equal(p0[0].astype(F32), got["x"][0, 0])
    assert all(tj.device_ptrs())
    after, bafter = tj.get(), tj.body_result()
    assert all(np.array_equal(_bits(after[k]), _bits(got[k])) for k in KEYS) and all(np.array_equal(_bits(bafter[k]), _bits(body[k])) for k in body)


def test_from_pose_paths_with_turns_in_place():
    """Pose paths that end in a turn in place, a path that only turns (five points, no length), the goal itself and a start
    without a path, resampled on the device against the reference's rule; then smoothed for the planner's footprint."""
    import gpismap_amd
    sc, B, goals, starts = tbc.turn_scene()
    df = gpismap_amd.DistanceField()
    df.from_grid(_dev(np.ascontiguousarray(sc["f"], F32).ravel()).data_ptr(), sc["shape"], sc["origin"], sc["step"], 0.0)
    dist = df.get()[0].ravel()
    fp = _footprint(B)
    pp = gpismap_amd.PosePlanner().solve(df, fp, goals, H=tbc.TURN_H, moves=tbc.TURN_MOVES, **tbc.TURN_OPTS)
    paths, heads, scost, st = pp.paths(starts)
    off = pp.last_off.copy()
    pts = np.concatenate(paths) if off[-1] else np.zeros((0, 2), F32)
    tbc.check_turn_paths(off, pts, st)
    tj = gpismap_amd.Trajectories()
    for N in (3, 5, 64, 65):
        x, ist = tb.resample(off, pts, st, N)
        assert pp.trajectories(N, trajectories=tj) is tj
        got = tj.optimize(df, iters=0).get()
        assert np.array_equal(got["x"].view(U32), x.view(U32)) and np.array_equal(got["status"] == 2, ist == 2), N
        assert np.all(got["x"][tbc.TURN_ONLY] == pts[off[tbc.TURN_ONLY]])
        o, wt = _opts(sc, B, iters=4)
        ref = tb.optimize(dist, sc["shape"], sc["origin"], sc["step"], B, x, ist, o, wt)
        assert df.smooth(pp, N=N, trajectories=tj, footprint=fp, iters=4) is tj
        _equal(tj.get(), tj.body_result(), ref, ("pose paths", N))


def test_argument_errors_leave_the_result_alone():
    import gpismap_amd
    L = gpismap_amd.lib()
    f, df, dist = _env()["balls2"]
    f3, df3, _ = _env()["balls3"]
    c = _cases()["hand2_N4_two_w1"]
    tj = gpismap_amd.Trajectories()
    got, body = _run(c, tj)
    fp, fp3 = _footprint(c["body"]), _footprint(tbc.bodies(3)["two"])
    empty = gpismap_amd.Footprint(2).set(np.zeros((0, 2)), np.zeros(0))
    o, _ = gpismap_amd.traj_body_opts(2, f["step"], 2)
    bad = gpismap_amd.traj_body_opts(2, f["step"], 2)[0]
    bad.margin = 0.0

    def call(t=tj, d=df, b=fp, op=o, wt=1.0):
        h = lambda v: v.h if v is not None else None
        return L.gpis_smooth_body_optimize(h(t), h(d), h(b), C.byref(op) if op is not None else None, C.c_float(wt), None)

    for name, kw, rc in (("no_traj", dict(t=None), ARG), ("no_field", dict(d=None), ARG), ("no_body", dict(b=None), ARG), ("empty", dict(b=empty), ARG),
                         ("neg_turn", dict(wt=-1.0), ARG), ("nan_turn", dict(wt=float("nan")), ARG), ("inf_turn", dict(wt=float("inf")), ARG),
                         ("body_dim", dict(b=fp3), ARG), ("field_dim", dict(d=df3, b=fp3), ARG), ("opts", dict(op=bad), ARG),
                         ("no_result", dict(d=gpismap_amd.DistanceField()), STATE), ("no_input", dict(t=gpismap_amd.Trajectories()), STATE)):
        assert call(**kw) == rc, name
        after, bafter = tj.get(), tj.body_result()
        assert all(np.array_equal(_bits(after[k]), _bits(got[k])) for k in KEYS) and all(np.array_equal(_bits(bafter[k]), _bits(body[k])) for k in body), name
    assert call(op=None) == 0                                                      # NULL options: the defaults for the footprint's m
    ref = _ref(dict(c, opts={}))
    _equal(tj.get(), tj.body_result(), ref, "default options")
    assert L.gpis_smooth_body_get(None, None, None, None, None) == ARG and L.gpis_smooth_from_pose_paths(tj.h, None, 8) == ARG
    pp = gpismap_amd.PosePlanner()
    assert L.gpis_smooth_from_pose_paths(tj.h, pp.h, 8) == STATE and L.gpis_smooth_from_pose_paths(tj.h, pp.h, 2) == ARG
    with pytest.raises(gpismap_amd.GpisError):
        tj.optimize(df, w_turn=1.0)
