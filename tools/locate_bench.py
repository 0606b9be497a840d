"""Pose-scoring benchmark (gpis3_locate_depth_field / gpis2_locate_scan_field) on tools/track_field_bench.py's inputs:
  - gazebo: scan 14 (270 beams) against the field (demo grid at 0.1 m) of the map of the scans before it, --poses2 (100 000)
    poses of a grid around the recorded pose;
  - synthetic: the bench map (synthetic 640x480 depth, 5 frames) and its field at (256, 192, 64), a 640x480 depth rendered
    1.5 cm / 1 degree off the identity at stride 8 (4 800 grid samples), --poses3 (10 000) poses of a grid around it;
  - gazebo_locate: locate-and-refine on scans 6, 14 and 22 from a grid of 0.5 m / 10 degrees that does not contain the recorded
    pose, against the field of the scans before each.
Per workload it prints one JSON line (and appends it to --out) with
  - field_ms: the map-level distance_field call that builds the field (median of --repeats),
  - call_ms: the scoring call, arguments built before the clock starts (median of --repeats; it returns with its work done),
    samples = poses x points, samples_per_s,
  - loop_ms_per_pose / loop_ms_extrapolated: the route it replaces, a loop of track_*_field(max_iters=0) calls, timed on the
    first --loop-poses poses and scaled to the batch (said so in the record), and whether its costs agree with the scorer's
    inlier counts,
  - ref_ms: the numpy reference (tests/locate_ref.py) on the first --ref-poses poses, scaled to the batch, and whether it gives
    the same bits there.
The time of the scoring kernel itself comes from a separate profiler run (no timing there):
  rocprofv3 --kernel-trace --stats -d DIR -o locate -- python tools/locate_bench.py --repeats 1 --out ''
  python profiles/summarize_rocpd.py DIR/locate_results.db
(profiles/locate_kernel_stats.txt)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from track_bench import err2, perturb3  # noqa: E402

F32 = np.float32
SYN = dict(origin=(-0.60, -0.45, 0.85), step=0.3 / 64, shape=(256, 192, 64))
BOX2 = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
OFF2 = (0.08, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--poses2", type=int, default=100000)
    ap.add_argument("--poses3", type=int, default=10000)
    ap.add_argument("--loop-poses", type=int, default=500, help="poses of the per-pose tracker loop (scaled to the batch)")
    ap.add_argument("--ref-poses", type=int, default=200, help="poses of the numpy reference (scaled to the batch)")
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synthetic", "gazebo_locate"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
    import locate_ref
    import replay

    L = gpismap_amd.lib()
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out_f = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def median_ms(fn):
        fn()                                              # (warm-up: buffers grow on the first call)
        return [timed(fn)[0] for _ in range(args.repeats)]

    def lat(df):
        i = df.info()
        return i["shape"], i["origin"], i["step"]

    def record(name, dim, build, call, loc, poses, loop_one, ref):
        fms = [timed(build)[0] for _ in range(args.repeats)]
        cms = median_ms(call)
        cost, inl, order = loc.get()
        info = loc.info()
        samples = info["poses"] * info["points"]
        rec = {"workload": name, "repeats": args.repeats, "poses": info["poses"], "points": info["points"], "samples": samples,
               "field_ms": float(np.median(fms)), "field_ms_all": fms, "call_ms": float(np.median(cms)), "call_ms_all": cms,
               "info_ms": info["ms"], "samples_per_s": samples / (float(np.median(cms)) * 1e-3),
               "best": int(order[0]), "best_cost": float(cost[order[0]]), "best_inliers": int(inl[order[0]])}
        nl = min(args.loop_poses, poses.shape[0])
        loop_one(poses[0])
        t0 = time.perf_counter()
        loop_inl = [loop_one(poses[k]) for k in range(nl)]
        lms = (time.perf_counter() - t0) * 1e3
        rec.update(loop_poses=nl, loop_ms=lms, loop_ms_per_pose=lms / nl, loop_ms_extrapolated=lms / nl * poses.shape[0],
                   loop_note="timed on the first %d poses and scaled to %d" % (nl, poses.shape[0]),
                   loop_inliers_agree=bool(np.array_equal(np.asarray(loop_inl), inl[:nl])))
        rec["loop_over_call"] = rec["loop_ms_extrapolated"] / rec["call_ms"]
        nr = min(args.ref_poses, poses.shape[0])
        rms, (rc, rn, _) = timed(lambda: ref(poses[:nr]))
        rec.update(ref_poses=nr, ref_ms=rms, ref_ms_extrapolated=rms / nr * poses.shape[0],
                   ref_bits_agree=bool(np.array_equal(rc.view(np.uint64), cost[:nr].view(np.uint64)) and np.array_equal(rn, inl[:nr])))
        rec["ref_over_call"] = rec["ref_ms_extrapolated"] / rec["call_ms"]
        emit(rec)

    fr2 = replay.load_gazebo() if any(w.startswith("gazebo") for w in args.workloads) else None

    def gazebo_field(k):
        g2 = gpismap_amd.GPisMap()
        for i in range(k):
            g2.update(fr2[i]["thetas"], fr2[i]["ranges"], fr2[i]["pose"])
        g2.sync()
        df = gpismap_amd.DistanceField()
        g2.distance_field(field=df, **BOX2)
        return g2, df

    def xyth(p):
        return float(p[0]), float(p[1]), math.atan2(float(p[3]), float(p[2]))

    if "gazebo" in args.workloads:
        g2, df = gazebo_field(14)
        fr = fr2[14]
        x, y, th = xyth(fr["pose"])
        na = 40
        nxy = int(math.ceil(math.sqrt(args.poses2 / na)))
        poses = gpismap_amd.pose_grid2(x + np.linspace(-2.0, 2.0, nxy), y + np.linspace(-2.0, 2.0, nxy),
                                       th + np.radians(np.linspace(-20.0, 20.0, na)))[:args.poses2]
        poses = np.ascontiguousarray(poses)
        tht, rg = np.ascontiguousarray(fr["thetas"], F32), np.ascontiguousarray(fr["ranges"], F32)
        loc, trk = gpismap_amd.Locator(), gpismap_amd.Tracker()
        o = gpismap_amd.locate_opts(2, top_k=16)

        def call():
            assert L.gpis2_locate_scan_field(g2.h, df.h, loc.h, P(tht), P(rg), tht.size, None, P(poses), poses.shape[0], C.byref(o), None) == 0

        def loop_one(p):
            return g2.track_scan_field(df, tht, rg, p, tracker=trk, max_iters=0)[1]["inliers"]
        shape, origin, step = lat(df)
        dist = df.get()[0].ravel()
        record("gazebo_270_beams_x_%d_poses" % poses.shape[0], 2, lambda: g2.distance_field(field=df, **BOX2), call, loc, poses, loop_one,
               lambda q: locate_ref.score_scan(dist, shape, origin, step, tht, rg, q, OFF2))

    if "synthetic" in args.workloads:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df = gpismap_amd.DistanceField()
        gm.distance_field(field=df, **SYN)
        truth = perturb3(replay.IDENTITY_POSE, 0.015, 1.0, axis=(1.0, 2.0, -1.0), tdir=(0.6, -1.0, 0.5))
        depth = np.ascontiguousarray(gm.render_depth(truth, cam6=SYN_CAM)[0], F32)
        nr = 10
        no = int(math.ceil((args.poses3 / nr) ** (1.0 / 3.0)))
        a = np.linspace(-0.05, 0.05, no)
        off = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
        rv = [(0.0, 0.0, 0.0)] + [(0.02 * math.cos(t), 0.02 * math.sin(t), 0.01) for t in np.linspace(0, 2 * math.pi, nr - 1, endpoint=False)]
        poses = np.ascontiguousarray(gpismap_amd.pose_grid3(truth, off, rv)[:args.poses3])
        loc, trk = gpismap_amd.Locator(), gpismap_amd.Tracker()
        o = gpismap_amd.locate_opts(3, stride=8, top_k=16)
        cam = gpismap_amd._cam(SYN_CAM)

        def call():
            assert L.gpis3_locate_depth_field(gm.h, df.h, loc.h, C.byref(cam), P(depth), P(poses), poses.shape[0], C.byref(o), None) == 0

        def loop_one(p):
            return gm.track_depth_field(df, depth, p, cam6=SYN_CAM, tracker=trk, max_iters=0, stride=8)[1]["inliers"]
        shape, origin, step = lat(df)
        dist = df.get()[0].ravel()
        record("synthetic_640x480_stride8_x_%d_poses" % poses.shape[0], 3, lambda: gm.distance_field(field=df, **SYN), call, loc, poses,
               loop_one, lambda q: locate_ref.score_depth(dist, shape, origin, step, depth, SYN_CAM, q, stride=8))

    if "gazebo_locate" in args.workloads:
        for k in (6, 14, 22):
            g2, df = gazebo_field(k)
            fr = fr2[k]
            x, y, th = xyth(fr["pose"])
            # a grid of 0.5 m / 10 degrees shifted off the recorded pose by 0.2 m / 4 degrees
            poses = gpismap_amd.pose_grid2(x + 0.2 + np.arange(-3, 4) * 0.5, y - 0.2 + np.arange(-3, 4) * 0.5,
                                           th + math.radians(4.0) + np.radians(np.arange(-18, 18) * 10.0))
            g2.locate_scan_field(df, fr["thetas"], fr["ranges"], poses)
            ms, (pose, info) = timed(lambda: g2.locate_scan_field(df, fr["thetas"], fr["ranges"], poses))
            b = info["best"]
            first = poses[info["order"][0]]
            emit({"workload": "gazebo_locate_scan_%d" % k, "poses": int(poses.shape[0]), "refine": int(len(info["tracks"])),
                  "call_ms": ms, "first_error_m_deg": list(err2(first, fr["pose"])), "error_m_deg": list(err2(pose, fr["pose"])),
                  "status": int(info["tracks"][b]["status"]), "iterations": [int(t["iterations"]) for t in info["tracks"]],
                  "best_candidate": int(b), "refined_cost": [float(v) for v in info["refined_cost"]],
                  "refined_inliers": [int(v) for v in info["refined_inliers"]], "first_cost": float(info["cost"][info["order"][0]])})
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
