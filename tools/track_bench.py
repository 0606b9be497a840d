"""Tracking benchmark (gpis3_track_depth / gpis2_track_scan).  Workloads:
  - synthetic_s1 / synthetic_s2: the bench map (synthetic 640x480 depth, F = 5 frames, identity pose); a 640x480 depth image
    rendered from a pose 1.5 cm / 1 degree off the identity, tracked from a further 2 cm / 2 degrees at stride 1 and 2;
  - bigbird: frames 2, 17 and 30 held out of a map of their four nearest frames, each tracked at 640x480 (stride 2) from its
    pose moved by 2 cm / 2 degrees;
  - gazebo: scans 6, 14 and 22 tracked against the map of the scans before them from their pose moved by 10 cm / 2 degrees.
Per workload it prints one JSON line with
  - call_ms: wall time of the calls (median of --repeats; each call returns with its work finished),
  - pass_ms: the host wall time of their passes (transform, test(), terms, reduction, the sums read back) and call_ms / pass_ms,
  - iterations, passes, points per pass, statuses and pose errors,
  - today_ms: the same result the way a user gets it without the call: the numpy reference (tests/track_ref.py) on the host
    with the map's test() once per pass, and whether it gives the same bits.
The time of the tracker's own kernels (the track_* kernels) comes from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o track -- python tools/track_bench.py --repeats 3 --no-today
  python profiles/summarize_rocpd.py DIR/track_results.db
(profiles/track_kernel_stats.txt)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVEL = -0.2
F32 = np.float32
U32 = np.uint32


def rot(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def perturb3(P, dt, deg, axis=(0.4, -1.0, 0.7), tdir=(1.0, -0.8, 0.9)):
    d = np.asarray(tdir, np.float64)
    t = np.asarray(P[:3], np.float64) + dt * d / np.linalg.norm(d)
    R = rot(axis, math.radians(deg)) @ np.asarray(P[3:], np.float64).reshape(3, 3).T
    return np.concatenate([t, R.T.ravel()]).astype(F32)


def perturb2(P, dt, deg, tdir=(1.0, -0.9)):
    d = np.asarray(tdir, np.float64)
    t = np.asarray(P[:2], np.float64) + dt * d / np.linalg.norm(d)
    th = math.atan2(float(P[3]), float(P[2])) + math.radians(deg)
    return np.array([t[0], t[1], math.cos(th), math.sin(th), -math.sin(th), math.cos(th)], F32)


def err3(P, Q):
    Rp, Rq = (np.asarray(X[3:], np.float64).reshape(3, 3).T for X in (P, Q))
    c = (np.trace(Rp.T @ Rq) - 1) / 2
    return (float(np.linalg.norm(np.asarray(P[:3], np.float64) - np.asarray(Q[:3], np.float64))),
            math.degrees(math.acos(min(1.0, max(-1.0, c)))))


def err2(P, Q):
    dth = math.atan2(float(P[3]), float(P[2])) - math.atan2(float(Q[3]), float(Q[2]))
    dth = (dth + math.pi) % (2 * math.pi) - math.pi
    return float(np.hypot(float(P[0]) - float(Q[0]), float(P[1]) - float(Q[1]))), abs(math.degrees(dth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["synthetic_s1", "synthetic_s2", "bigbird", "gazebo"])
    ap.add_argument("--no-today", action="store_true", help="skip the host-side path (profiler runs)")
    args = ap.parse_args()

    import gpismap_amd
    import replay
    import track_ref

    L = gpismap_amd.lib()
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def track3(gm, t, depth, pose0, cam6, **kw):
        """the C call alone: arguments built before the clock starts, the results read after it stops"""
        d = np.ascontiguousarray(depth, F32)
        p = np.ascontiguousarray(pose0, F32)
        cam = gpismap_amd._cam(cam6)
        o = gpismap_amd.track_opts(3, **kw)
        out = np.zeros(12, F32)

        def fn():
            assert L.gpis3_track_depth(gm.h, t.h, C.byref(cam), P(d), P(p), C.byref(o), P(out), None) == 0
            return out.copy(), t
        return fn

    def track2(g2, t, fr, pose0):
        th, rg, p = (np.ascontiguousarray(a, F32) for a in (fr["thetas"], fr["ranges"], pose0))
        o = gpismap_amd.track_opts(2)
        out = np.zeros(6, F32)

        def fn():
            assert L.gpis2_track_scan(g2.h, t.h, P(th), P(rg), th.size, P(p), C.byref(o), P(out), None) == 0
            return out.copy(), t
        return fn

    def run(name, calls, truths, errf, today):
        ms, per = [], []
        for c in calls:                         # (warm-up: buffers grow on the first call)
            c()
        for _ in range(args.repeats):
            tot = 0.0
            per = []
            for c in calls:
                t0 = time.perf_counter()
                pose, t = c()
                tot += (time.perf_counter() - t0) * 1e3
                per.append((pose, t.result()))
            ms.append(tot)
        info = [i for _, i in per]
        sums = {k: float(sum(i[k] for i in info)) for k in ("iterations", "passes", "points", "pass_ms", "evals")}
        res = {"workload": name, "calls": len(calls), "repeats": args.repeats, "call_ms": float(np.median(ms)), "call_ms_all": ms,
               **sums}
        res["call_ms_per_call"] = res["call_ms"] / len(calls)
        res["call_over_passes"] = float(ms[-1] / max(sums["pass_ms"], 1e-9))     # (pass_ms is that of the last repeat)
        res["points_per_pass"] = sums["points"] / len(calls)
        res["ms_per_pass"] = sums["pass_ms"] / max(sums["passes"], 1)
        res["status"] = [i["status"] for i in info]
        res["iterations_each"] = [i["iterations"] for i in info]
        res["inliers"] = [i["inliers"] for i in info]
        res["errors_m_deg"] = [list(errf(p, q)) for (p, _), q in zip(per, truths)]
        if today is not None and not args.no_today:
            t0 = time.perf_counter()
            refs = today()
            res["today_ms"] = (time.perf_counter() - t0) * 1e3
            same = True
            for (pose, i), r in zip(per, refs):
                same = same and np.array_equal(pose.view(U32), r["pose"].view(U32)) and i["status"] == r["status"] \
                    and i["iterations"] == r["iterations"] and np.array_equal(i["H"].view(np.uint64), r["H"].view(np.uint64)) \
                    and np.array_equal(i["resid"].view(U32), r["resid"].view(U32))
            res["today_same_bits"] = bool(same)
        print(json.dumps(res), flush=True)

    syn = [w for w in args.workloads if w.startswith("synthetic")]
    if syn:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        cam = (568.0, 568.0, 310.0, 224.0, 640, 480)
        truth = perturb3(replay.IDENTITY_POSE, 0.015, 1.0, axis=(1.0, 2.0, -1.0), tdir=(0.6, -1.0, 0.5))
        depth = gm.render_depth(truth, cam6=cam)[0]
        start = perturb3(truth, 0.02, 2.0)
        for w in syn:
            stride = 1 if w.endswith("s1") else 2
            t = gpismap_amd.Tracker()

            def today(stride=stride):
                return [track_ref.track_depth(lambda x, res: gm.test(x, res), depth, cam, start,
                                              track_ref.Opts(3, level=LEVEL, stride=stride))]
            run("synthetic_640x480_stride%d" % stride, [track3(gm, t, depth, start, cam, stride=stride)], [truth], err3, today)

    if "bigbird" in args.workloads:
        frames = replay.load_bigbird()
        c = np.array([f["pose"][:3] for f in frames], np.float64)
        calls, truths, refs = [], [], []
        maps = []
        for k in (2, 17, 30):
            d = np.linalg.norm(c - c[k], axis=1)
            d[k] = np.inf
            ids = sorted(np.argsort(d)[:4].tolist())
            gb = gpismap_amd.GPisMap3(frames[ids[0]]["cam"])
            for i in ids:
                gb.set_camera(frames[i]["cam"])
                gb.update(frames[i]["depth"], frames[i]["pose"])
            gb.sync()
            maps.append(gb)
            start = perturb3(frames[k]["pose"], 0.02, 2.0)
            calls.append(track3(gb, gpismap_amd.Tracker(), frames[k]["depth"], start, frames[k]["cam"]))
            truths.append(frames[k]["pose"])
            refs.append((gb, frames[k], start))

        def today_bb():
            return [track_ref.track_depth(lambda x, res, g=g: g.test(x, res), fr["depth"], fr["cam"], s, track_ref.Opts(3, level=LEVEL))
                    for g, fr, s in refs]
        run("bigbird_640x480_held_out", calls, truths, err3, today_bb)

    if "gazebo" in args.workloads:
        fr2 = replay.load_gazebo()
        calls, truths, refs = [], [], []
        for k in (6, 14, 22):
            g2 = gpismap_amd.GPisMap()
            for i in range(k):
                g2.update(fr2[i]["thetas"], fr2[i]["ranges"], fr2[i]["pose"])
            g2.sync()
            start = perturb2(fr2[k]["pose"], 0.1, 2.0)
            calls.append(track2(g2, gpismap_amd.Tracker(), fr2[k], start))
            truths.append(fr2[k]["pose"])
            refs.append((g2, fr2[k], start))

        def today_gz():
            return [track_ref.track_scan(lambda x, res, g=g: g.test(x, res), fr["thetas"], fr["ranges"], s, (0.08, 0.0),
                                         track_ref.Opts(2, level=LEVEL)) for g, fr, s in refs]
        run("gazebo_270_beams", calls, truths, err2, today_gz)


if __name__ == "__main__":
    main()
