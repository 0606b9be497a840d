"""Inputs shared by tests/test_detect_ref.py (CPU: the reference against its defective variants, on analytic distance grids) and
tests/test_gpu_detect.py (the device against the reference, on the device's own dist of the same grids): rooms without
furniture, scans and depth frames of them, and discs / patches added to the measurements that the field does not hold."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64

# ---- a 2-D room: free inside |x| < 3, |y| < 2.2 -----------------------------------------------------------------------------
ROOM2 = dict(shape=(69, 53), origin=(-3.4, -2.6), step=0.1, half=(3.0, 2.2))
BEAMS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)     # the wavefront, 256-wide scans, a compaction chunk of 2048 +- 1
OFF2 = (0.05, -0.02)


def lattice_axes(shape, origin, step):
    return [(F32(origin[a]) + np.arange(shape[a], dtype=F32) * F32(step)).astype(F32) for a in range(len(shape))]


def room2_grid():
    """f (flat, x fastest): the distance to the nearest wall, positive inside the room."""
    ax = lattice_axes(ROOM2["shape"], ROOM2["origin"], ROOM2["step"])
    X, Y = np.meshgrid(ax[0].astype(F64), ax[1].astype(F64), indexing="xy")
    return np.minimum(ROOM2["half"][0] - np.abs(X), ROOM2["half"][1] - np.abs(Y)).astype(F32).ravel()


def pose2(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([x, y, c, s, -s, c], F64)


def thetas_of(n):
    return (-math.pi + 2.0 * math.pi * np.arange(n, dtype=F64) / n).astype(F32)


def sensor2(pose, off=OFF2):
    """(position [2], yaw) of the sensor in the world."""
    p = np.asarray(pose, F64)
    return np.array([p[0] + p[2] * off[0] + p[4] * off[1], p[1] + p[3] * off[0] + p[5] * off[1]]), math.atan2(p[3], p[2])


def room2_ranges(thetas, pose, off=OFF2):
    """The ranges of the empty room from the pose (float64)."""
    p, yaw = sensor2(pose, off)
    a = np.asarray(thetas, F32).astype(F64) + yaw
    r = np.full(a.size, np.inf)
    for ax, d in ((0, np.cos(a)), (1, np.sin(a))):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (ROOM2["half"][ax] - p[ax]) / d, np.where(d < 0, (-ROOM2["half"][ax] - p[ax]) / d, np.inf))
        r = np.minimum(r, t)
    return r


def disc_ranges(thetas, pose, centre, radius, off=OFF2):
    """The range at which each beam meets the disc (inf: it does not): a ray-circle intersection."""
    p, yaw = sensor2(pose, off)
    a = np.asarray(thetas, F32).astype(F64) + yaw
    q = np.asarray(centre, F64) - p
    b = q[0] * np.cos(a) + q[1] * np.sin(a)
    disc = b * b - (q @ q - radius * radius)
    with np.errstate(invalid="ignore"):
        r = b - np.sqrt(disc)
    return np.where((disc >= 0) & (r > 0), r, np.inf)


def scan2(n, pose, discs, static=None):
    """(thetas [n] f32, ranges [n] f32) of the room with the discs ((centre, radius), ...) in it."""
    th = thetas_of(n)
    r = room2_ranges(th, pose) if static is None else np.asarray(static, F64).copy()
    for c, rad in discs:
        r = np.minimum(r, disc_ranges(th, pose, c, rad))
    return th, r.astype(F32)


POSE2 = pose2(0.3, -0.2, 0.4)


def disc_at_beam(n, k, pose=POSE2, rng=1.4, radius=0.15):
    """A disc whose centre lies on the direction between beams floor(k) and floor(k) + 1 of an n-beam scan (k may be fractional)."""
    p, yaw = sensor2(pose)
    a = -math.pi + 2.0 * math.pi * k / n + yaw
    return (p + rng * np.array([math.cos(a), math.sin(a)]), radius)


def frame2(n):
    """The discs of the n-beam frame: one across the last beam and beam 0 (they must stay two components), one across beams
    63 | 64 and one across 2047 | 2048 where the scan has them, one a quarter of the way round."""
    discs = [disc_at_beam(n, n - 0.5 if n > 1 else 0.0), disc_at_beam(n, n / 4.0 + 0.5)]
    if n > 64:
        discs.append(disc_at_beam(n, 63.5))
    if n > 2048:
        discs.append(disc_at_beam(n, 2047.5))
    return discs


# ---- exact edges: f = x on a dyadic lattice, every sample on the row y = 1 (the lattice's last) ----------------------------------
EDGE = dict(shape=(33, 17), origin=(-1.0, -1.0), step=0.125)
EDGE_POSE = np.array([0.0, 1.0, 1.0, 0.0, 0.0, 1.0], F64)
EDGE_LINK = 0.25


def edge_grid():
    ax = lattice_axes(EDGE["shape"], EDGE["origin"], EDGE["step"])
    X, _ = np.meshgrid(ax[0], ax[1], indexing="xy")
    return X.astype(F32).ravel()


def edge_scan():
    """Beams along +x from (0, 1) with no sensor offset, so a sample is (r, 1) exactly: 0, 1 exactly `link` apart (one component);
    3, 4 one ulp beyond (two); 6 exactly on the lattice's last point (3, 1); 7 off the lattice (d NaN); 2 and 5 not valid."""
    up = np.nextafter(F32(1.25), F32(2))
    return np.zeros(8, F32), np.array([1.0, 1.25, 0.0, 1.0, up, 0.0, 3.0, 3.5], F32)


def singles_scan(n_single=300, tail=0):
    """Every second beam valid on the edge field from (1.5, 0): isolated one-sample components, then `tail` valid beams in a row."""
    n = 2 * n_single + tail
    th = thetas_of(n)
    r = np.zeros(n, F32)
    r[0:2 * n_single:2] = 0.5
    r[2 * n_single:] = 0.5
    return th, r, np.array([1.5, 0.0, 1.0, 0.0, 0.0, 1.0], F64)


# ---- a 3-D room: free below the wall z = 2.5, seen by a camera at the origin looking along +z -------------------------------
ROOM3 = dict(shape=(33, 33, 31), origin=(-1.6, -1.6, 0.0), step=0.1, wall=2.5)
POSE3 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], F64)
SIZES3 = ((8, 8), (33, 17), (80, 60))


def room3_grid():
    ax = lattice_axes(ROOM3["shape"], ROOM3["origin"], ROOM3["step"])
    n = ROOM3["shape"]
    Z = np.broadcast_to(ax[2][:, None, None], (n[2], n[1], n[0]))
    return (F32(ROOM3["wall"]) - Z).astype(F32).ravel()


def cam6(W, H):
    return (64.0, 64.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H)


def serpentine(gw, gh):
    """A one-pixel-wide path over the grid [gw, gh]: every second column, joined alternately at the top and the bottom."""
    m = np.zeros((gw, gh), bool)
    m[0::2, :] = True
    for k, c in enumerate(range(1, gw - 1, 2)):
        m[c, 0 if k % 2 else gh - 1] = True
    return m


def blobs(gw, gh):
    """Patches that touch only across a diagonal (one component under 8 neighbours, two under 4), and a separate one."""
    m = np.zeros((gw, gh), bool)
    a, b = max(1, gw // 4), max(1, gh // 4)
    m[0:a, 0:b] = True
    m[a:2 * a, b:2 * b] = True
    m[gw - 1, gh - 1] = True
    return m


def depth3(W, H, stride, mask, near=1.5):
    """depth [W * H] column-major: the wall, and `near` at the strided pixels where mask [W // stride, H // stride] is set."""
    d = np.full((W, H), ROOM3["wall"], F32)
    gw, gh = W // stride, H // stride
    sub = d[:gw * stride:stride, :gh * stride:stride]
    sub[mask] = near
    return d.ravel()


# ---- five frames of tracks ----------------------------------------------------------------------------------------------------
TRACK_T = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5)
TRACK_OPTS = dict(min_points=2, max_missed=1)


def track_discs(k):
    """The discs of frame k: one moving, one at rest, one that appears at frame 3, one that disappears after frame 1."""
    t = TRACK_T[k]
    discs = [((-1.5 + 0.4 * t, 1.0), 0.15), ((1.5, -1.2), 0.2)]
    if k >= 3:
        discs.append(((-1.0, -1.3), 0.15))
    if k <= 1:
        discs.append(((2.0, 1.2), 0.15))
    return discs


# ---- closed loop: detect, hand over, steer -------------------------------------------------------------------------------------
LOOP_BEAMS = 360
LOOP_OFF = (0.0, 0.0)
LOOP_DETECT = dict(min_points=2)


def loop_frame(static, pose, ball, t):
    """(thetas, ranges f32) of one step: the field's own rendered ranges (NaN: a miss), the least of them and the true disc's."""
    import obst_ref
    th = thetas_of(LOOP_BEAMS)
    c = obst_ref.at(ball, t)[0]
    r = np.fmin(np.asarray(static, F64), disc_ranges(th, pose, c, float(ball["r"][0]), LOOP_OFF))
    return th, np.where(np.isfinite(r), r, 0.0).astype(F32)


def detected_set(balls, t, step):
    """The set the controller takes from a detection (None: no ball), with the closed loops' cost options."""
    import obst_cases
    import obst_ref
    if balls["radius"].size == 0:
        return None
    return obst_ref.make(2, balls["centre"], balls["velocity"], balls["radius"], epoch=t, step=step, **obst_cases.LOOP_OBST)


def ref_loop(cfg, ball, pad_steps, log=None):
    """obst_cases.closed_loop with the disc `ball` known only through the detector's reference: at every step the field's rendered
    scan with the true disc in it, detect, hand over, obst_ref's controller.  Returns closed_loop's dict (sep: from the true disc)."""
    import detect_ref
    import mppi_cases as mc
    import obst_cases
    import obst_ref
    import render_field_ref
    sc = mc.scene(2)
    o = mc.opts(2, **cfg["opts"])
    cost, goal = (sc["cost"], None) if cfg["terminal"] == "plan" else (None, sc["goal_point"])
    ctl = obst_ref.Controller(2, cfg["K"], cfg["T"], cfg["seed"])
    det = detect_ref.Detector()
    do = detect_ref.opts(2, sc["step"], pad=float(F64(F32(pad_steps) * F32(sc["step"]))), **LOOP_DETECT)
    th = thetas_of(LOOP_BEAMS)

    def step_fn(pose, t):
        static = render_field_ref.render_scan(sc["dist"], sc["shape"], sc["origin"], sc["step"], th, pose.astype(F32), LOOP_OFF)[0]
        _, r = loop_frame(static, pose, ball, t)
        res = det.detect(sc["dist"], sc["shape"], sc["origin"], sc["step"], 2, (th, r, LOOP_OFF), pose, t, do)["balls"]
        if log is not None:
            log.append((t, res))
        u0, _ = ctl.step(sc["dist"], sc["shape"], sc["origin"], sc["step"], pose, o, cost=cost, goal=goal,
                         obst=detected_set(res, t, sc["step"]), t_now=t)
        ctl.shift()
        return u0

    return obst_cases.closed_loop(cfg, step_fn=step_fn, track=ball)


# Measured with ref_loop on the CPU (tests/test_detect_ref.py asserts them): the smallest pad in whole lattice steps for which the
# least separation from the TRUE disc (speed 0.3, radius 0.4, through the unaware robot's state of step 30) stays positive, that
# separation and the step count.  The controller keeps its own clearance (0.25) and band (1.0) around the detected ball, which is
# why no pad is needed here although the box-midpoint ball of the near arc misses the disc's far side.
LOOP_PAD_STEPS = 0
LOOP_MIN_SEP = 1.3887159073824389
LOOP_STEPS = 76
