"""The detector's reference (tests/detect_ref.py) on the CPU: every case of tests/detect_cases.py reaches the branch it is there
for, every defective variant is rejected by at least one case, and the exact properties of the contract hold.  The fields are the
analytic grids themselves (the reference takes any dist); tests/test_gpu_detect.py runs the same frames on the device's dist."""
import math

import numpy as np
import pytest

import detect_cases as dc
import detect_ref as dr

F32 = np.float32
F64 = np.float64


def _room2():
    return dc.room2_grid(), dc.ROOM2["shape"], dc.ROOM2["origin"], dc.ROOM2["step"]


def _edge():
    return dc.edge_grid(), dc.EDGE["shape"], dc.EDGE["origin"], dc.EDGE["step"]


def _room3():
    return dc.room3_grid(), dc.ROOM3["shape"], dc.ROOM3["origin"], dc.ROOM3["step"]


def run2(field, frame, pose, t=1.0, variant=None, seen=None, det=None, **kw):
    dist, shape, origin, step = field
    o = dr.opts(2, step, **kw)
    det = det if det is not None else dr.Detector(variant)
    return det.detect(dist, shape, origin, step, 2, frame, pose, t, o, seen), o


def run3(W, H, stride, mask, variant=None, **kw):
    dist, shape, origin, step = _room3()
    o = dr.opts(3, step, stride=stride, **kw)
    return dr.Detector(variant).detect(dist, shape, origin, step, 3, (dc.depth3(W, H, stride, mask), dc.cam6(W, H)), dc.POSE3, 1.0, o), o


def same_result(a, b):
    if not np.array_equal(a["label"], b["label"]):
        return False
    for k in ("centre", "velocity", "radius", "id", "age", "count", "label"):
        x, y = a["balls"][k], b["balls"][k]
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def flood_partition(dim, s, o):
    """An independent flood fill over the links: label image with each class named by its smallest member."""
    g, f, x = s["g"], s["foreign"], s["x"]
    p, q = dr.neighbour_pairs(dim, g, s["gw"], s["gh"])
    adj = {}
    for a, b in zip(p.tolist(), q.tolist()):
        if f[a] and f[b] and dr.link_s(x[a:a + 1], x[b:b + 1])[0] <= o["link"] * o["link"]:
            adj.setdefault(a, []).append(b)
            adj.setdefault(b, []).append(a)
    img = np.full(g, -1, np.int32)
    for a in np.nonzero(f)[0].tolist():
        if img[a] >= 0:
            continue
        img[a] = a
        stack = [a]
        while stack:
            u = stack.pop()
            for w in adj.get(u, ()):
                if img[w] < 0:
                    img[w] = a
                    stack.append(w)
    return img


def check_properties(dim, res, o):
    """r2 covers every sample of its component in the contract's own arithmetic; the partition is the flood fill's."""
    s, img, tab = res["samples"], res["label"], res["tab"]
    assert np.array_equal(img, flood_partition(dim, s, o))
    assert np.array_equal(img >= 0, s["foreign"]) and not (s["foreign"] & ~s["valid"]).any()
    for c, lab in enumerate(tab["label"].tolist()):
        xs = s["x"][img == lab]
        ss = np.zeros(xs.shape[0], F64)
        for a in range(dim):
            e = xs[:, a].astype(F64) - tab["centre"][c, a]
            ss = ss + e * e
        assert (ss <= tab["r2"][c]).all() and (ss == tab["r2"][c]).any()
        assert lab == np.nonzero(img == lab)[0].min() and tab["count"][c] == xs.shape[0]
    b = res["balls"]
    assert np.array_equal(np.sort(b["label"][b["label"] >= 0]), b["label"][b["label"] >= 0])
    assert len(set(b["id"].tolist())) == b["id"].size


@pytest.mark.parametrize("n", dc.BEAMS)
def test_frames_2d_reach_their_branches(n):
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n))
    res, o = run2(_room2(), frame + (dc.OFF2,), dc.POSE2, min_points=1)
    img = res["label"]
    check_properties(2, res, o)
    assert img[n - 1] >= 0 and img[0] >= 0, "the disc across the wrap is seen by the last beam and by beam 0"
    if n > 1:
        assert img[0] != img[n - 1], "no wrap: they stay two"
    if n > 2:
        wr, _ = run2(_room2(), frame + (dc.OFF2,), dc.POSE2, variant="wrap", min_points=1)
        assert not same_result(res, wr) and wr["balls"]["components"] == res["balls"]["components"] - 1
    if n > 64:
        assert img[63] >= 0 and img[63] == img[64]
    if n > 2048:
        assert img[2047] >= 0 and img[2047] == img[2048]
    assert res["balls"]["components"] >= (1 if n == 1 else 2)
    # the walls are the field's own: no wall sample is foreign
    d = res["samples"]["d"]
    assert (np.abs(d[~res["samples"]["foreign"] & res["samples"]["valid"]]) < o["min_dist"]).all()


def test_link_and_threshold_edges():
    th, r = dc.edge_scan()
    field = _edge()
    md = float(field[0][16 * 33 + 16])                       # d at (1, 1): the lattice value there
    assert md == 1.0
    res, o = run2(field, (th, r, (0.0, 0.0)), dc.EDGE_POSE, link=dc.EDGE_LINK, min_dist=md, min_points=1, max_radius=10.0)
    s, img = res["samples"], res["label"]
    assert np.array_equal(s["x"][[0, 1, 3, 4, 6]], np.array([[1, 1], [1.25, 1], [1, 1], [np.nextafter(F32(1.25), F32(2)), 1], [3, 1]], F32))
    assert s["d"][0] == F32(md) and s["foreign"][0], "d == min_dist is foreign"
    assert img.tolist() == [0, 0, -1, 3, 4, -1, 6, -1]
    assert np.isnan(s["d"][7]) and s["valid"][7] and not s["foreign"][7], "off the lattice: not foreign"
    assert not s["valid"][2] and np.isnan(s["d"][2])
    assert s["foreign"][6] and np.isfinite(s["d"][6]), "exactly on the lattice's last point"
    check_properties(2, res, o)
    gt, _ = run2(field, (th, r, (0.0, 0.0)), dc.EDGE_POSE, variant="gt", link=dc.EDGE_LINK, min_dist=md, min_points=1, max_radius=10.0)
    assert not same_result(res, gt) and gt["label"][0] == -1
    # the mask's nearest point of (3, 1) is the last byte
    seen = np.ones(33 * 17, np.uint8)
    seen[-1] = 0
    ms, _ = run2(field, (th, r, (0.0, 0.0)), dc.EDGE_POSE, seen=seen, link=dc.EDGE_LINK, min_dist=md, min_points=1, max_radius=10.0)
    assert ms["label"].tolist() == [0, 0, -1, 3, 4, -1, -1, -1]


def link32_case():
    """A link length that separates the double and the float32 measure of one pair of neighbouring samples of the 257-beam frame."""
    n = 257
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    res, _ = run2(_room2(), frame, dc.POSE2, min_points=1)
    s, img = res["samples"], res["label"]
    for k in range(n - 1):
        if img[k] >= 0 and img[k] == img[k + 1]:
            a, b = s["x"][k:k + 1], s["x"][k + 1:k + 2]
            s64, s32 = float(dr.link_s(a, b)[0]), float(dr.link_s(a, b, "link32")[0])
            if s64 != s32:
                return frame, math.sqrt(0.5 * (s64 + s32)), k
    raise AssertionError("no pair separates the two measures")


def test_link_in_float32_is_rejected():
    frame, link, k = link32_case()
    a, _ = run2(_room2(), frame, dc.POSE2, min_points=1, link=link)
    b, _ = run2(_room2(), frame, dc.POSE2, variant="link32", min_points=1, link=link)
    assert (a["label"][k] == a["label"][k + 1]) != (b["label"][k] == b["label"][k + 1])
    assert not same_result(a, b)


@pytest.mark.parametrize("W,H", dc.SIZES3)
@pytest.mark.parametrize("stride", (1, 2))
def test_frames_3d_reach_their_branches(W, H, stride):
    gw, gh = W // stride, H // stride
    res, o = run3(W, H, stride, dc.serpentine(gw, gh), min_points=1, max_radius=10.0)
    check_properties(3, res, o)
    assert res["balls"]["components"] == 1 and res["balls"]["foreign"] == int(dc.serpentine(gw, gh).sum())
    assert res["samples"]["g"] == gw * gh and res["balls"]["samples"] == gw * gh
    bl, o = run3(W, H, stride, dc.blobs(gw, gh), min_points=1, max_radius=10.0)
    check_properties(3, bl, o)
    assert bl["balls"]["components"] == 2
    n4, _ = run3(W, H, stride, dc.blobs(gw, gh), variant="n4", min_points=1, max_radius=10.0)
    assert n4["balls"]["components"] == 3 and not same_result(bl, n4)


def test_selection_cap_noise_and_size():
    field = _edge()
    th, r, pose = dc.singles_scan(300)
    res, o = run2(field, (th, r, (0.0, 0.0)), pose, min_points=1)
    b = res["balls"]
    assert b["components"] == 300 and b["count"].size == 256 and b["dropped"] == 44 and (b["count"] == 1).all()
    assert np.array_equal(b["label"], np.arange(0, 512, 2)), "ties by the lower label"
    hi, _ = run2(field, (th, r, (0.0, 0.0)), pose, variant="tie_high", min_points=1)
    assert not same_result(res, hi) and hi["balls"]["label"][0] == 88
    # a larger component at the highest labels is kept before the one-sample ones
    th, r, pose = dc.singles_scan(300, tail=9)
    res, o = run2(field, (th, r, (0.0, 0.0)), pose, min_points=1, link=1.0)
    b = res["balls"]
    assert b["components"] == 301 and b["label"][-1] == 600 and b["count"][-1] == 9 and b["dropped"] == 45
    assert np.array_equal(b["label"][:-1], np.arange(0, 510, 2))
    # min_points and max_radius each remove what they should
    n = 257
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    base, _ = run2(_room2(), frame, dc.POSE2, min_points=1)
    cnt = base["tab"]["count"]
    cut = int(np.sort(cnt)[len(cnt) // 2]) + 1
    mp, _ = run2(_room2(), frame, dc.POSE2, min_points=cut)
    assert mp["balls"]["noise"] == int((cnt < cut).sum()) > 0 and mp["balls"]["count"].size == int((cnt >= cut).sum()) > 0
    rad = np.sqrt(base["tab"]["r2"])
    mid = float(0.5 * (rad.min() + rad.max()))
    mr, _ = run2(_room2(), frame, dc.POSE2, min_points=1, max_radius=mid)
    assert mr["balls"]["too_large"] == int((rad > mid).sum()) > 0 and mr["balls"]["count"].size == int((rad <= mid).sum()) > 0
    assert (mr["tab"]["flag"] == np.where(rad > mid, dr.LARGE, dr.BALL)).all()


def test_centre_is_the_box_midpoint_not_the_mean():
    n = 257
    frame = dc.scan2(n, dc.POSE2, dc.frame2(n)) + (dc.OFF2,)
    a, _ = run2(_room2(), frame, dc.POSE2)
    b, _ = run2(_room2(), frame, dc.POSE2, variant="mean")
    assert a["balls"]["count"].size >= 2 and not same_result(a, b)
    t = a["tab"]
    assert np.array_equal(t["centre"], 0.5 * (t["box"][:, 0].astype(F64) + t["box"][:, 1].astype(F64)))


def test_coverage_mask_hides_the_unseen_half():
    n = 256
    disc = ((-1.5, 0.5), 0.2)
    frame = dc.scan2(n, dc.POSE2, [disc, ((1.5, 0.5), 0.2)]) + (dc.OFF2,)
    shape = dc.ROOM2["shape"]
    ax = dc.lattice_axes(shape, dc.ROOM2["origin"], dc.ROOM2["step"])
    seen = np.broadcast_to(ax[0][None, :] > 0, shape[::-1]).astype(np.uint8).ravel()
    free, _ = run2(_room2(), frame, dc.POSE2)
    half, _ = run2(_room2(), frame, dc.POSE2, seen=seen)
    full, _ = run2(_room2(), frame, dc.POSE2, seen=np.ones_like(seen))
    assert free["balls"]["count"].size == 2 and half["balls"]["count"].size == 1 and half["balls"]["centre"][0, 0] > 0
    assert same_result(free, full)


def track_frames(det=None, variant=None, field=None):
    """The five frames (and two more without the vanished disc) through one detector.  Returns the results."""
    det = det if det is not None else dr.Detector(variant)
    out = []
    for k, t in enumerate(dc.TRACK_T):
        frame = dc.scan2(720, dc.POSE2, dc.track_discs(k)) + (dc.OFF2,)
        res, _ = run2(field or _room2(), frame, dc.POSE2, t=t, det=det, **dc.TRACK_OPTS)
        out.append(res["balls"])
    return out


def test_tracks_ids_ages_coasting_and_velocities():
    fr = track_frames()
    ids = [dict(zip(f["id"].tolist(), range(f["id"].size))) for f in fr]
    # frame 0: three new balls, v = 0, age 0
    assert fr[0]["id"].size == 3 and (fr[0]["age"] == 0).all() and not fr[0]["velocity"].any()
    mov = int(fr[0]["id"][np.argmin(np.abs(fr[0]["centre"][:, 1] - 1.0) + np.abs(fr[0]["centre"][:, 0] + 1.3))])
    gone = int(fr[0]["id"][np.argmax(fr[0]["centre"][:, 0])])
    for k in range(1, 7):
        assert fr[k]["age"][ids[k][mov]] == k and fr[k]["missed"][ids[k][mov]] == 0
    # age 0 takes v_raw whole, later the filter settles on the disc's 0.4 along x
    v1 = fr[1]["velocity"][ids[1][mov]]
    c0, c1 = fr[0]["centre"][ids[0][mov]], fr[1]["centre"][ids[1][mov]]
    assert np.array_equal(v1, (c1 - c0) / (dc.TRACK_T[1] - dc.TRACK_T[0]))
    v6 = fr[6]["velocity"][ids[6][mov]]
    print("velocity of the moving disc after 6 updates: %s (true 0.4, 0)" % v6)
    assert abs(v6[0] - 0.4) < 0.1 and abs(v6[1]) < 0.1
    # the disc that disappears after frame 1 coasts for max_missed = 1 call, after the detected ones, and is dropped then
    assert gone in ids[1] and fr[2]["missed"][ids[2][gone]] == 1 and fr[2]["label"][ids[2][gone]] == -1 and ids[2][gone] == fr[2]["id"].size - 1
    assert gone not in ids[3]
    # the disc that appears at frame 3 gets a fresh id
    new = set(ids[3]) - set(ids[2])
    assert len(new) == 1 and fr[3]["age"][ids[3][new.pop()]] == 0
    nf = track_frames(variant="no_filter")
    assert any(a["velocity"].tobytes() != b["velocity"].tobytes() for a, b in zip(fr, nf))


def test_association_is_a_matching_and_time_must_increase():
    rng = np.random.default_rng(5)
    o = dr.opts(2, 0.1, gate=0.5, max_missed=3)
    tr = dict(balls=[], t_prev=0.0, held=False, next_id=0)
    t = 0.0
    for it in range(12):
        t += 0.25
        n = int(rng.integers(0, 9))
        det = [dict(c=rng.uniform(-1, 1, 2), r=0.1, comp=j) for j in range(n)]
        old = {b["id"]: b for b in tr["balls"]} if tr["held"] else {}
        out = dr.associate(2, det, t, o, tr)
        got = [b["id"] for b in out]
        assert len(set(got)) == len(got), "each ball is matched once"
        for b in out[:n]:
            if b["age"] > 0:
                p = old[b["id"]]
                d = math.dist(b["c"], [p["c"][a] + p["v"][a] * 0.25 for a in range(2)])
                assert d <= o["gate"] + o["max_speed"] * 0.25
        assert [b["comp"] for b in out[:n]] == list(range(n)) and all(b["comp"] == -1 for b in out[n:])
        assert [b["id"] for b in out[n:]] == sorted(b["id"] for b in out[n:])
    det = dr.Detector()
    frame = dc.scan2(64, dc.POSE2, dc.frame2(64)) + (dc.OFF2,)
    run2(_room2(), frame, dc.POSE2, t=1.0, det=det)
    with pytest.raises(ValueError):
        run2(_room2(), frame, dc.POSE2, t=1.0, det=det)
    det.reset_tracks()
    run2(_room2(), frame, dc.POSE2, t=0.5, det=det)


def test_defaults_are_the_stated_ones():
    o = dr.opts(3, 0.1)
    assert o["min_dist"] == float(F32(2) * F32(0.1)) and o["link"] == float(F32(3) * F32(0.1)) and o["stride"] == 2
    assert dr.opts(2, 0.1)["stride"] == 1 and o["pad"] == float(F32(0.1)) and o["gate"] == float(F32(4) * F32(0.1))
    k = dr.key(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-30, 2.0, np.inf], F32))
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(dr.unkey(k).view(np.uint32), np.array(
        [-np.inf, -1.0, -0.0, 0.0, 1e-30, 2.0, np.inf], F32).view(np.uint32))


def loop_ball():
    import obst_cases as oc
    from test_mppi_ref import LOOP2
    unaware = oc.closed_loop(LOOP2)
    ball = oc.crossing_ball(LOOP2, unaware["states"], 0.3, 0.4)
    return LOOP2, ball, oc.least_separation(LOOP2, unaware["states"], ball)


def test_closed_loop_detects_and_avoids_the_crossing_disc():
    """obst_cases' 2-D closed loop with the crossing disc known only through its returns in the scan: detect, hand over, steer.
    Without the set the controller collides (-0.40).  Recorded: pad 0 steps, least separation 1.389 from the true disc, 76 steps;
    velocity error of the filtered track (age >= 8) against the disc's true (0.205, -0.219): at most 0.196, 0.047 on average."""
    import mppi_cases as mc
    cfg, ball, unaware_sep = loop_ball()
    assert unaware_sep < -0.39
    log = []
    r = dc.ref_loop(cfg, ball, dc.LOOP_PAD_STEPS, log)
    late = np.array([b["velocity"][0] for _, b in log if b["radius"].size and b["age"][0] >= 8])
    err = np.abs(late - ball["v"][0])
    print("pad %d steps: %s steps, least separation %.6f from the true disc, %.3f from the goal; %d detections; velocity error at age >= 8: "
          "max %.3f mean %.3f" % (dc.LOOP_PAD_STEPS, r["steps"], r["sep"], r["e"], sum(1 for _, b in log if b["radius"].size), err.max(),
                                  err.mean()))
    assert r["steps"] == dc.LOOP_STEPS and r["e"] <= 2 * mc.scene(2)["step"]
    assert r["sep"] > 0 and r["sep"] == dc.LOOP_MIN_SEP
    assert dc.LOOP_PAD_STEPS == 0, "the smallest pad: there is none below"
    assert sum(1 for _, b in log if b["radius"].size) > 20
