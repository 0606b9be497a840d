"""The moving-obstacle detector on the GPU (csrc/detect.hip, gpis_detect_*) against the numpy reference (tests/detect_ref.py) on
the device's own dist: every device value is a minimum, a maximum or an integer sum and the host half is plain double in one
order, so every array is compared for equal bytes.  Fields come from from_grid on the analytic grids of tests/detect_cases.py."""
import numpy as np
import pytest

import detect_cases as dc
import detect_ref as dr

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -3, -4
_CACHE = {}


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _field(name):
    """(DistanceField, (its own dist flat, shape, origin, step)) of a named grid of detect_cases, built once."""
    import gpismap_amd
    if name not in _CACHE:
        grid, lat = dict(room2=(dc.room2_grid, dc.ROOM2), edge=(dc.edge_grid, dc.EDGE), room3=(dc.room3_grid, dc.ROOM3))[name]
        df = gpismap_amd.DistanceField()
        df.from_grid(_dev(grid()).data_ptr(), lat["shape"], lat["origin"], lat["step"], 0.0)
        _CACHE[name] = (df, (df.get()[0].ravel(), lat["shape"], lat["origin"], lat["step"]))
    return _CACHE[name]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(det, got, ref, what=""):
    """Every array of the device's result against the reference's: bytes."""
    s, rs = det.samples(), ref["samples"]
    assert _same(s["label"], ref["label"]), (what, np.flatnonzero(s["label"] != ref["label"])[:8])
    assert _same(s["d"], rs["d"]) and _same(s["x"], rs["x"]) and _same(s["foreign"], rs["foreign"].astype(np.uint8)), what
    c, rt = det.components(), ref["tab"]
    for k in ("label", "count", "flag", "box", "centre", "r2"):
        assert _same(c[k], rt[k]), (what, k, c[k][:4], rt[k][:4])
    rb = ref["balls"]
    for k in ("centre", "velocity", "radius", "count", "label", "id", "age", "missed", "box"):
        assert _same(got[k], rb[k]), (what, k, got[k][:4], rb[k][:4])
    for k in ("samples", "foreign", "components", "noise", "too_large", "dropped"):
        assert got[k] == rb[k], (what, k, got[k], rb[k])
    i = det.info()
    assert i["valid"] == 1 and i["balls"] == rb["id"].size and i["grid"] == rs["g"] and i["tracks"] == rb["id"].size


def _both2(name, frame, pose, t=1.0, det=None, rdet=None, cover=None, seen=None, stream=None, **kw):
    """One scan through the device and the reference on the device's dist.  Returns (device result, reference result, detector)."""
    import gpismap_amd
    df, (dist, shape, origin, step) = _field(name)
    det = det if det is not None else gpismap_amd.Detector()
    rdet = rdet if rdet is not None else dr.Detector()
    th, r, off = frame
    got = df.detect_scan(th, r, pose, off, t, detector=det, cover=cover, stream=stream, **kw)
    ref = rdet.detect(dist, shape, origin, step, 2, frame, pose, t, dr.opts(2, step, **kw), seen)
    _compare(det, got, ref, (name, len(th), kw))
    return got, ref, det


def _both3(W, H, stride, mask, det=None, rdet=None, **kw):
    import gpismap_amd
    df, (dist, shape, origin, step) = _field("room3")
    det = det if det is not None else gpismap_amd.Detector()
    rdet = rdet if rdet is not None else dr.Detector()
    depth, cam = dc.depth3(W, H, stride, mask), dc.cam6(W, H)
    got = df.detect_depth(depth, dc.POSE3, cam, 1.0, detector=det, stride=stride, **kw)
    ref = rdet.detect(dist, shape, origin, step, 3, (depth, cam), dc.POSE3, 1.0, dr.opts(3, step, stride=stride, **kw))
    _compare(det, got, ref, (W, H, stride, kw))
    return got, ref, det


def _status(fn):
    import gpismap_amd
    with pytest.raises(gpismap_amd.GpisError) as e:
        fn()
    return int(str(e.value).rsplit(" ", 1)[1])


# ---- 2-D frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.BEAMS)
def test_scan_frames_bit_equal(n):
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    got, ref, det = _both2("room2", frame, dc.POSE2, min_points=1)
    img = ref["label"]
    assert img[0] >= 0 and img[n - 1] >= 0 and (n == 1 or img[0] != img[n - 1]), "the last beam and beam 0 stay two components"
    if n > 64:
        assert img[63] >= 0 and img[63] == img[64]
    if n > 2048:
        assert img[2047] >= 0 and img[2047] == img[2048]
    assert got["components"] >= (1 if n == 1 else 2) and det.info()["rounds"] >= 1
    _both2("room2", frame, dc.POSE2)                             # (the defaults: min_points 3)


# ---- 3-D frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.SIZES3)
@pytest.mark.parametrize("stride", (1, 2))
def test_depth_frames_bit_equal(W, H, stride):
    gw, gh = W // stride, H // stride
    got, _, det = _both3(W, H, stride, dc.blobs(gw, gh), min_points=1, max_radius=10.0)
    assert got["components"] == 2 and det.info()["grid_w"] == gw and det.info()["grid_h"] == gh
    got, _, _ = _both3(W, H, stride, dc.serpentine(gw, gh), min_points=1, max_radius=10.0)
    assert got["components"] == 1
    _both3(W, H, stride, dc.serpentine(gw, gh))


def test_serpentine_rounds_and_schedules():
    import gpismap_amd
    W, H = 80, 60
    mask = dc.serpentine(W, H)
    outs = []
    for every in (1, 4, 64):
        det = gpismap_amd.Detector().set_schedule(check_every=every)
        got, _, _ = _both3(W, H, 1, mask, det=det, min_points=1, max_radius=10.0)
        rounds = det.info()["rounds"]
        print("serpentine %dx%d check_every %d: %d rounds" % (W, H, every, rounds))
        assert rounds % every == 0 and rounds >= every
        if every < 64:
            assert rounds > every, "several read-backs"
        outs.append((det.samples()["label"], got["centre"], got["radius"]))
    for o in outs[1:]:
        assert all(_same(a, b) for a, b in zip(o, outs[0]))
    # max_rounds = 1 cannot converge on it: GPIS_ERR_LIMIT, and no result is held
    df, _ = _field("room3")
    det = gpismap_amd.Detector()
    _both3(8, 8, 1, dc.blobs(8, 8), det=det, min_points=1)
    assert _status(lambda: df.detect_depth(dc.depth3(W, H, 1, mask), dc.POSE3, dc.cam6(W, H), 2.0, detector=det, stride=1,
                                           max_rounds=1)) == ERR_LIMIT
    assert det.info()["valid"] == 0 and _status(det.result) == ERR_STATE and _status(det.samples) == ERR_STATE
    assert det.info()["tracks_held"] == 1 and det.info()["t_prev"] == 1.0, "the tracks stay"


# ---- link and threshold edges ---------------------------------------------------------------------------------------------------
def test_link_and_threshold_edges():
    import gpismap_amd
    df, (dist, shape, origin, step) = _field("edge")
    th, r = dc.edge_scan()
    md = float(dist[16 * 33 + 16])                             # the device's d at (1, 1)
    kw = dict(link=dc.EDGE_LINK, min_dist=md, min_points=1, max_radius=10.0)
    got, ref, det = _both2("edge", (th, r, (0.0, 0.0)), dc.EDGE_POSE, **kw)
    s = det.samples()
    assert s["d"][0] == F32(md) and s["foreign"][0] == 1, "d == min_dist is foreign"
    assert s["label"][:2].tolist() == [0, 0], "exactly `link` apart: one component"
    assert s["label"][3:5].tolist() == [3, 4], "one ulp beyond: two"
    assert np.isnan(s["d"][7]) and s["foreign"][7] == 0 and s["label"][7] == -1, "off the lattice"
    assert np.array_equal(s["x"][6], np.array([3.0, 1.0], F32)) and s["foreign"][6] == 1, "on the lattice's last point"
    # with a mask that lacks that last byte the sample is not foreign
    seen = np.ones(int(np.prod(shape)), np.uint8)
    seen[-1] = 0
    cv = gpismap_amd.Coverage().reset(df).set(seen)
    _both2("edge", (th, r, (0.0, 0.0)), dc.EDGE_POSE, cover=cv, seen=seen, **kw)
    assert det.samples()["label"][6] == 6


def test_link_length_between_double_and_float32():
    df, (dist, shape, origin, step) = _field("room2")
    n = 257
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    _, ref, _ = _both2("room2", frame, dc.POSE2, min_points=1)
    s, img = ref["samples"], ref["label"]
    for k in range(n - 1):
        if img[k] >= 0 and img[k] == img[k + 1]:
            s64 = float(dr.link_s(s["x"][k:k + 1], s["x"][k + 1:k + 2])[0])
            s32 = float(dr.link_s(s["x"][k:k + 1], s["x"][k + 1:k + 2], "link32")[0])
            if s64 != s32:
                _both2("room2", frame, dc.POSE2, min_points=1, link=float(np.sqrt(0.5 * (s64 + s32))))
                return
    raise AssertionError("no pair separates the two measures")


# ---- selection ------------------------------------------------------------------------------------------------------------------
def test_selection_cap_noise_and_size():
    th, r, pose = dc.singles_scan(300)
    got, _, _ = _both2("edge", (th, r, (0.0, 0.0)), pose, min_points=1)
    assert got["components"] == 300 and got["count"].size == 256 and got["dropped"] == 44
    assert np.array_equal(got["label"], np.arange(0, 512, 2))
    th, r, pose = dc.singles_scan(300, tail=9)
    got, _, _ = _both2("edge", (th, r, (0.0, 0.0)), pose, min_points=1, link=1.0)
    assert got["components"] == 301 and got["label"][-1] == 600 and got["count"][-1] == 9 and got["dropped"] == 45
    n = 257
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    base, ref, _ = _both2("room2", frame, dc.POSE2, min_points=1)
    cnt, rad = ref["tab"]["count"], np.sqrt(ref["tab"]["r2"])
    cut = int(np.sort(cnt)[len(cnt) // 2]) + 1
    got, _, _ = _both2("room2", frame, dc.POSE2, min_points=cut)
    assert got["noise"] == int((cnt < cut).sum()) > 0 and got["count"].size == int((cnt >= cut).sum()) > 0
    mid = float(0.5 * (rad.min() + rad.max()))
    got, _, det = _both2("room2", frame, dc.POSE2, min_points=1, max_radius=mid)
    assert got["too_large"] == int((rad > mid).sum()) > 0 and np.array_equal(det.components()["flag"] == 2, rad > mid)


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_coverage_mask():
    import gpismap_amd
    df, (dist, shape, origin, step) = _field("room2")
    frame = dc.scan2(256, dc.POSE2, [((-1.5, 0.5), 0.2), ((1.5, 0.5), 0.2)]) + (dc.OFF2,)
    ax = dc.lattice_axes(shape, origin, step)
    seen = np.broadcast_to(ax[0][None, :] > 0, tuple(shape)[::-1]).astype(np.uint8).ravel()
    cv = gpismap_amd.Coverage().reset(df)
    free, _, _ = _both2("room2", frame, dc.POSE2)
    half, _, _ = _both2("room2", frame, dc.POSE2, cover=cv.set(seen), seen=seen)
    assert free["count"].size == 2 and half["count"].size == 1 and half["centre"][0, 0] > 0, "the disc in the unseen half is not reported"
    full, _, _ = _both2("room2", frame, dc.POSE2, cover=cv.set(np.ones_like(seen)), seen=np.ones_like(seen))
    assert all(_same(full[k], free[k]) for k in ("centre", "radius", "count", "label", "box"))
    # a mask of another lattice, and one that was never reset
    other = gpismap_amd.Coverage().reset(_field("edge")[0])
    det = gpismap_amd.Detector()
    _both2("room2", frame, dc.POSE2, det=det)
    th, r, off = frame
    for bad in (other, gpismap_amd.Coverage()):
        assert _status(lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, cover=bad)) == ERR_STATE
        assert det.info()["valid"] == 1 and det.result()["count"].size == 2 and det.info()["t_prev"] == 1.0


# ---- tracks ---------------------------------------------------------------------------------------------------------------------
def test_tracks_bit_equal_over_frames():
    import gpismap_amd
    df, _ = _field("room2")
    det, rdet = gpismap_amd.Detector(), dr.Detector()
    fr = []
    for k, t in enumerate(dc.TRACK_T):
        frame = dc.scan2(720, dc.POSE2, dc.track_discs(k)) + (dc.OFF2,)
        got, _, _ = _both2("room2", frame, dc.POSE2, t=t, det=det, rdet=rdet, **dc.TRACK_OPTS)
        fr.append(got)
    assert fr[0]["id"].size == 3 and (fr[0]["age"] == 0).all() and not fr[0]["velocity"].any()
    assert fr[2]["id"].size == 3 and fr[2]["missed"][-1] == 1 and fr[2]["label"][-1] == -1, "coasting, after the detected ones"
    assert fr[3]["id"].size == 3 and fr[2]["id"][-1] not in fr[3]["id"], "dropped after max_missed"
    assert (fr[3]["age"] == 0).sum() == 1 and fr[6]["age"].max() == 6
    # t must increase: refused with the tracks intact
    th, r, off = dc.scan2(720, dc.POSE2, dc.track_discs(6)) + (dc.OFF2,)
    before = det.result()
    for t in (dc.TRACK_T[-1], 0.0, float("nan")):
        assert _status(lambda: df.detect_scan(th, r, dc.POSE2, off, t, detector=det, **dc.TRACK_OPTS)) == ERR_ARG
    after = det.result()
    assert all(_same(before[k], after[k]) for k in ("centre", "velocity", "id", "age")) and det.info()["t_prev"] == dc.TRACK_T[-1]
    got, _, _ = _both2("room2", (th, r, off), dc.POSE2, t=4.0, det=det, rdet=rdet, **dc.TRACK_OPTS)
    assert got["age"].max() == 7
    det.reset_tracks()
    rdet.reset_tracks()
    got, _, _ = _both2("room2", (th, r, off), dc.POSE2, t=0.25, det=det, rdet=rdet, **dc.TRACK_OPTS)
    assert (got["age"] == 0).all()


# ---- handles --------------------------------------------------------------------------------------------------------------------
def test_one_detector_through_changing_frames_streams_and_refusals():
    import gpismap_amd
    import torch
    det, rdet = gpismap_amd.Detector(), dr.Detector()             # (ids go on counting over reset_tracks, in both)
    own = torch.cuda.Stream(device=0)
    t = 0.0
    for k, n in enumerate((2049, 63, 256, 1, 2048, 65)):
        t += 0.5
        frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
        _both2("room2", frame, dc.POSE2, t=t, det=det, rdet=rdet, stream=own.cuda_stream if k % 2 else None, min_points=1,
               max_missed=0, gate=0.0, max_speed=0.0)
        det.reset_tracks()
        rdet.reset_tracks()
    got, _, _ = _both3(33, 17, 1, dc.blobs(33, 17), det=det, rdet=rdet, min_points=1)     # (the same handle on a 3-D field)
    det.reset_tracks()
    rdet.reset_tracks()
    df, _ = _field("room2")
    n = 64
    th, r, off = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    good, _, _ = _both2("room2", (th, r, off), dc.POSE2, t=1.0, det=det, rdet=rdet, min_points=1)
    nanpose = dc.POSE2.copy()
    nanpose[3] = np.inf
    refusals = [
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, link=-1.0)),
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, min_dist=float("nan"))),
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, alpha=0.0)),
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, alpha=1.5)),
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, 2.0, detector=det, min_points=0)),
        (ERR_ARG, lambda: df.detect_scan(th, r, nanpose, off, 2.0, detector=det)),
        (ERR_ARG, lambda: df.detect_scan(th, r, dc.POSE2, off, float("inf"), detector=det)),
        (ERR_ARG, lambda: _field("room3")[0].detect_scan(th, r, dc.POSE2, off, 2.0, detector=det)),
        (ERR_ARG, lambda: _field("room3")[0].detect_depth(dc.depth3(8, 8, 1, dc.blobs(8, 8)), dc.POSE3, dc.cam6(8, 8), 2.0, detector=det,
                                                          stride=0)),
        (ERR_STATE, lambda: gpismap_amd.DistanceField().detect_scan(th, r, dc.POSE2, off, 2.0, detector=det)),
    ]
    for want, call in refusals:
        assert _status(call) == want
        now = det.result()
        assert det.info()["valid"] == 1 and all(_same(now[k], good[k]) for k in ("centre", "radius", "id", "label")), "still readable"
        assert np.array_equal(det.samples()["label"] >= 0, det.samples()["foreign"] == 1)
    # more than 2^26 beams or pixels: GPIS_ERR_LIMIT before anything is read -- the arrays are short, and a NaN angle in them
    # does not turn the code into GPIS_ERR_ARG; the previous result and the tracks stay
    import ctypes as C
    L = gpismap_amd.lib()
    fp, dpt = C.POINTER(C.c_float), C.POINTER(C.c_double)
    off32, pose2, pose3 = np.asarray(off, F32), np.ascontiguousarray(dc.POSE2, F64), np.ascontiguousarray(dc.POSE3, F64)
    th_nan = th.copy()
    th_nan[2] = np.nan
    held = det.info()
    for angles in (th, th_nan):
        assert L.gpis2_detect_scan_field(None, df.h, det.h, None, angles.ctypes.data_as(fp), r.ctypes.data_as(fp), (1 << 26) + 1,
                                         off32.ctypes.data_as(fp), pose2.ctypes.data_as(dpt), 2.0, None, None) == ERR_LIMIT
    small = np.full(64, 1.5, F32)
    cam = gpismap_amd._cam((64.0, 64.0, 4096.0, 4096.0, 8193, 8192))               # 8193 * 8192 = 2^26 + 2^13 pixels
    assert L.gpis3_detect_depth_field(None, _field("room3")[0].h, det.h, None, C.byref(cam), small.ctypes.data_as(fp),
                                      pose3.ctypes.data_as(dpt), 2.0, None, None) == ERR_LIMIT
    now, ni = det.result(), det.info()
    assert all(_same(now[k], good[k]) for k in ("centre", "velocity", "radius", "id", "age", "missed", "label", "count", "box"))
    assert all(ni[k] == held[k] for k in ("valid", "dim", "grid", "samples", "foreign", "components", "balls", "tracks", "tracks_held", "t_prev"))
    assert ni["valid"] == 1 and ni["tracks_held"] == 1 and ni["t_prev"] == 1.0
    assert np.array_equal(det.samples()["label"] >= 0, det.samples()["foreign"] == 1)
    fresh = gpismap_amd.Detector()
    assert _status(fresh.result) == ERR_STATE and _status(fresh.samples) == ERR_STATE and _status(fresh.components) == ERR_STATE
    # an empty frame is a result with no balls, and to_obstacles then empties the set
    ob = gpismap_amd.Obstacles(2, dc.ROOM2["step"], clearance=0.3)
    assert det.to_obstacles(ob) is ob and ob.info()["n"] == good["id"].size and ob.info()["epoch"] == 1.0
    g = ob.get()
    assert _same(g["centre"], good["centre"]) and _same(g["velocity"], good["velocity"]) and _same(g["radius"], good["radius"])
    assert g["opts"]["clearance"] == 0.3, "the set's options stay"
    for rr in (np.zeros(n, F32), dc.room2_ranges(th, dc.POSE2).astype(F32)):     # no valid sample; none foreign
        got, _, _ = _both2("room2", (th, rr, off), dc.POSE2, t=det.info()["t_prev"] + 1.0, det=det, rdet=rdet, max_missed=0)
        assert got["id"].size == 0 and got["components"] == 0
        df.detect_scan(th, rr, dc.POSE2, off, det.info()["t_prev"] + 1.0, detector=det, obstacles=ob, max_missed=0)
        assert ob.info()["n"] == 0


# ---- closed loop ----------------------------------------------------------------------------------------------------------------
def test_closed_loop_detect_hand_over_steer_on_the_device():
    """tests/test_detect_ref.py's closed loop through the device: DistanceField.render_scan, the true disc's returns, detect_scan,
    to_obstacles, Controller.step.  Every detection has the reference's bits on the same inputs and every controller step is the
    reference's step from the device's state with the device's weights (a q within 1 of the reference's, everything
    after it exact).  Where no q differed anywhere, the loop is the reference's: the same step count and least separation."""
    import gpismap_amd
    import mppi_cases as mc
    import obst_cases as oc
    import obst_ref
    import render_field_ref
    from test_detect_ref import loop_ball
    from test_gpu_mppi import env
    from test_mppi_ref import LOOP2
    sc, df, dist, pl, cost = env(2)
    cfg, ball, unaware_sep = loop_ball()
    assert unaware_sep < -0.39
    o = mc.opts(2, **LOOP2["opts"])
    ctl = gpismap_amd.Controller(**LOOP2["opts"])
    ctl.init(2, LOOP2["K"], LOOP2["T"], seed=LOOP2["seed"])
    det, rdet = gpismap_amd.Detector(), dr.Detector()
    ob = gpismap_amd.Obstacles(2, sc["step"], **oc.LOOP_OBST)
    pad = float(F64(F32(dc.LOOP_PAD_STEPS) * F32(sc["step"])))
    do = dr.opts(2, sc["step"], pad=pad, **dc.LOOP_DETECT)
    th = dc.thetas_of(dc.LOOP_BEAMS)
    count = dict(tick=0, q_off=0, detections=0, render_off=0)

    def step_fn(pose, t):
        static = df.render_scan(th, pose, dc.LOOP_OFF)[0]
        count["render_off"] += not _same(static, render_field_ref.render_scan(dist, sc["shape"], sc["origin"], sc["step"], th,
                                                                              pose.astype(F32), dc.LOOP_OFF)[0].astype(F32))
        _, r = dc.loop_frame(static, pose, ball, t)
        got = df.detect_scan(th, r, pose, dc.LOOP_OFF, t, detector=det, obstacles=ob, pad=pad, **dc.LOOP_DETECT)
        ref = rdet.detect(dist, sc["shape"], sc["origin"], sc["step"], 2, (th, r, dc.LOOP_OFF), pose, t, do)
        _compare(det, got, ref, "closed loop t %.1f" % t)
        S = dc.detected_set(ref["balls"], t, sc["step"])
        g = ob.get()
        assert ob.info()["n"] == got["radius"].size and (S is None or (_same(g["centre"], S["c"]) and _same(g["velocity"], S["v"])
                                                                        and _same(g["radius"], S["r"]) and g["epoch"] == t))
        count["detections"] += int(S is not None)
        before = ctl.get()
        u0, _ = df.control(ctl, pose, planner=pl, obstacles=ob, t=t)
        count["tick"] += 1
        args = (dist, sc["shape"], sc["origin"], sc["step"], pose, before["U"], LOOP2["seed"], count["tick"])
        rr = obst_ref.roll(*args, LOOP2["K"], o, cost, None, obst=S, t_now=t)
        q = ctl.get()["q"]
        dq = np.abs(q.astype(np.int64) - rr["q"].astype(np.int64))
        assert dq.max() <= 1, "t %.1f: q differs by up to %d" % (t, dq.max())
        count["q_off"] += int(np.count_nonzero(dq))
        f = obst_ref.finish(rr, q, *args, o, cost, None, obst=S, t_now=t)
        assert _same(np.asarray(u0, F64), np.asarray(f["u0"], F64)), "u0 at t %.1f" % t
        ctl.shift()
        return u0

    r = oc.closed_loop(LOOP2, step_fn=step_fn, track=ball)
    print("device loop: %s steps, least separation %.6f from the true disc, %d detections, %d weights off by one, %d scans not the reference renderer's (reference: %d steps, %.6f)"
          % (r["steps"], r["sep"], count["detections"], count["q_off"], count["render_off"], dc.LOOP_STEPS, dc.LOOP_MIN_SEP))
    assert r["steps"] is not None and r["steps"] <= LOOP2["budget"] and r["e"] <= 2 * sc["step"] and r["sep"] > 0
    assert count["detections"] > 20
    if count["q_off"] == 0 and count["render_off"] == 0:      # (the static ranges too were the reference renderer's bits)
        assert r["steps"] == dc.LOOP_STEPS and r["sep"] == dc.LOOP_MIN_SEP
