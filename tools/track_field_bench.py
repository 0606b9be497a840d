"""Field-tracking benchmark (gpis3_track_depth_field / gpis2_track_scan_field) on tools/track_bench.py's inputs:
  - synthetic_s1 / synthetic_s2: the bench map (synthetic 640x480 depth, F = 5 frames, identity pose) and its field on the
    lattice of tests/test_gpu_dfield.py's SYN (129x97x33 at 0.3/32 m); 640x480 depth rendered 1.5 cm / 1 degree off the
    identity, tracked from a further 2 cm / 2 degrees at stride 1 and 2;
  - bigbird: frames 2, 17 and 30 held out of a map of their four nearest frames, the field on the demo box at 2.5 mm, each frame
    tracked at 640x480 (stride 2) from its pose moved by 2 cm / 2 degrees;
  - gazebo: scans 6, 14 and 22 against the field (demo grid at 0.1 m) of the map of the scans before them, from their pose moved
    by 10 cm / 2 degrees and by 30 cm / 5 degrees.
Per workload it prints one JSON line (and appends it to --out) with
  - field_ms: the map-level distance_field call that builds the field (median of --repeats),
  - call_ms / passes / ms_per_pass / pass_ms: the field-tracking calls (median of --repeats; each returns with its work done),
  - map_call_ms / map_passes / map_ms_per_pass: the map tracker (gpis3_track_depth / gpis2_track_scan) on the same input in
    the same process, and the pose errors of both,
  - frames_per_field: --frames calls from different starts against one field, and what a frame costs with the field's build
    shared out: (field_ms + frames x call) / frames, next to the map tracker's call.
The time of the field tracker's own kernels comes from a separate profiler run (no timing there):
  rocprofv3 --kernel-trace --stats -d DIR -o track_field -- python tools/track_field_bench.py --repeats 1 --out ''
  python profiles/summarize_rocpd.py DIR/track_field_results.db
(profiles/track_field_kernel_stats.txt)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from track_bench import err2, err3, perturb2, perturb3  # noqa: E402

F32 = np.float32
SYN = dict(origin=(-0.60, -0.45, 0.85), step=0.3 / 32, shape=(129, 97, 33))
BOX3 = dict(origin=(-0.07, -0.10, 0.0), step=0.0025, shape=(81, 97, 113))
BOX2 = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10, help="calls against one field for the shared-cost record")
    ap.add_argument("--workloads", nargs="+", default=["synthetic_s1", "synthetic_s2", "bigbird", "gazebo"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_field_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
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

    def call3(gm, df, t, depth, pose0, cam6, field, **kw):
        """the C call alone: arguments built before the clock starts"""
        d, p = np.ascontiguousarray(depth, F32), np.ascontiguousarray(pose0, F32)
        cam = gpismap_amd._cam(cam6)
        o = gpismap_amd.track_opts(3, **kw)
        out = np.zeros(12, F32)

        def fn():
            if field:
                assert L.gpis3_track_depth_field(gm.h, df.h, t.h, C.byref(cam), P(d), P(p), C.byref(o), P(out), None) == 0
            else:
                assert L.gpis3_track_depth(gm.h, t.h, C.byref(cam), P(d), P(p), C.byref(o), P(out), None) == 0
            return out.copy()
        return fn

    def call2(g2, df, t, fr, pose0, field):
        th, rg, p = (np.ascontiguousarray(a, F32) for a in (fr["thetas"], fr["ranges"], pose0))
        o = gpismap_amd.track_opts(2)
        out = np.zeros(6, F32)

        def fn():
            if field:
                assert L.gpis2_track_scan_field(g2.h, df.h, t.h, P(th), P(rg), th.size, None, P(p), C.byref(o), P(out), None) == 0
            else:
                assert L.gpis2_track_scan(g2.h, t.h, P(th), P(rg), th.size, P(p), C.byref(o), P(out), None) == 0
            return out.copy()
        return fn

    def measure(calls, trackers):
        """median over the repeats of the summed wall time of the calls; the last repeat's poses and infos"""
        for c in calls:                                   # (warm-up: buffers grow on the first call)
            c()
        ms, poses, infos = [], [], []
        for _ in range(args.repeats):
            tot, poses = 0.0, []
            for c in calls:
                dt, p = timed(c)
                tot += dt
                poses.append(p)
            infos = [t.info() for t in trackers]
            ms.append(tot)
        return float(np.median(ms)), ms, poses, infos

    def run(name, builds, field_calls, map_calls, ftrackers, mtrackers, truths, errf, multi):
        """builds: functions that (re)build the fields of the workload; multi: (field build, calls against that one field)"""
        fms = []
        for _ in range(args.repeats):
            fms.append(sum(timed(b)[0] for b in builds))
        cms, call_all, fposes, finfo = measure(field_calls, ftrackers)
        mms, _, mposes, minfo = measure(map_calls, mtrackers)
        sm = lambda infos, k: float(sum(i[k] for i in infos))
        rec = {"workload": name, "calls": len(field_calls), "repeats": args.repeats,
               "field_ms": float(np.median(fms)), "field_ms_all": fms,
               "call_ms": cms, "call_ms_all": call_all, "call_ms_per_call": cms / len(field_calls),
               "iterations": sm(finfo, "iterations"), "passes": sm(finfo, "passes"), "points": sm(finfo, "points"),
               "pass_ms": sm(finfo, "pass_ms"), "evals": sm(finfo, "evals")}
        rec["ms_per_pass"] = rec["pass_ms"] / max(rec["passes"], 1)
        rec["points_per_pass"] = rec["points"] / len(field_calls)
        rec["status"] = [int(i["status"]) for i in finfo]
        rec["iterations_each"] = [int(i["iterations"]) for i in finfo]
        rec["inliers"] = [int(i["inliers"]) for i in finfo]
        rec["errors_m_deg"] = [list(errf(p, q)) for p, q in zip(fposes, truths)]
        rec["map_call_ms"] = mms
        rec["map_call_ms_per_call"] = mms / len(map_calls)
        rec["map_passes"] = sm(minfo, "passes")
        rec["map_ms_per_pass"] = sm(minfo, "pass_ms") / max(rec["map_passes"], 1)
        rec["map_status"] = [int(i["status"]) for i in minfo]
        rec["map_errors_m_deg"] = [list(errf(p, q)) for p, q in zip(mposes, truths)]
        rec["field_plus_call_over_map_call"] = (rec["field_ms"] + cms) / mms
        build, mcalls = multi
        bms = timed(build)[0]
        for c in mcalls:
            c()
        tot = 0.0
        for c in mcalls:
            tot += timed(c)[0]
        rec["frames_per_field"] = {"frames": len(mcalls), "field_ms": bms, "calls_ms": tot,
                                   "ms_per_frame_shared": (bms + tot) / len(mcalls),
                                   "map_call_ms_per_frame": rec["map_call_ms_per_call"]}
        emit(rec)

    syn = [w for w in args.workloads if w.startswith("synthetic")]
    if syn:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df = gpismap_amd.DistanceField()
        gm.distance_field(field=df, **SYN)
        truth = perturb3(replay.IDENTITY_POSE, 0.015, 1.0, axis=(1.0, 2.0, -1.0), tdir=(0.6, -1.0, 0.5))
        depth = gm.render_depth(truth, cam6=SYN_CAM)[0]
        start = perturb3(truth, 0.02, 2.0)
        starts = [perturb3(truth, 0.02, 2.0, axis=(np.cos(a), np.sin(a), 0.5), tdir=(np.sin(a), 0.7, np.cos(a)))
                  for a in np.linspace(0, 2 * np.pi, args.frames, endpoint=False)]
        for w in syn:
            stride = 1 if w.endswith("s1") else 2
            tf, tm = gpismap_amd.Tracker(), gpismap_amd.Tracker()
            run("synthetic_640x480_stride%d" % stride, [lambda: gm.distance_field(field=df, **SYN)],
                [call3(gm, df, tf, depth, start, SYN_CAM, True, stride=stride)],
                [call3(gm, df, tm, depth, start, SYN_CAM, False, stride=stride)], [tf], [tm], [truth], err3,
                (lambda: gm.distance_field(field=df, **SYN),
                 [call3(gm, df, tf, depth, s, SYN_CAM, True, stride=stride) for s in starts]))

    if "bigbird" in args.workloads:
        frames = replay.load_bigbird()
        c = np.array([f["pose"][:3] for f in frames], np.float64)
        builds, fcalls, mcalls, tfs, tms, truths = [], [], [], [], [], []
        keep = []
        for k in (2, 17, 30):
            d = np.linalg.norm(c - c[k], axis=1)
            d[k] = np.inf
            ids = sorted(np.argsort(d)[:4].tolist())
            gb = gpismap_amd.GPisMap3(frames[ids[0]]["cam"])
            for i in ids:
                gb.set_camera(frames[i]["cam"])
                gb.update(frames[i]["depth"], frames[i]["pose"])
            gb.sync()
            df = gpismap_amd.DistanceField()
            gb.distance_field(field=df, **BOX3)
            keep.append((gb, df))
            builds.append(lambda gb=gb, df=df: gb.distance_field(field=df, **BOX3))
            start = perturb3(frames[k]["pose"], 0.02, 2.0)
            tf, tm = gpismap_amd.Tracker(), gpismap_amd.Tracker()
            fcalls.append(call3(gb, df, tf, frames[k]["depth"], start, frames[k]["cam"], True))
            mcalls.append(call3(gb, df, tm, frames[k]["depth"], start, frames[k]["cam"], False))
            tfs.append(tf)
            tms.append(tm)
            truths.append(frames[k]["pose"])
        gb, df = keep[0]
        fr = frames[2]
        starts = [perturb3(fr["pose"], 0.02, 2.0, axis=(np.cos(a), np.sin(a), 0.5), tdir=(np.sin(a), 0.7, np.cos(a)))
                  for a in np.linspace(0, 2 * np.pi, args.frames, endpoint=False)]
        run("bigbird_640x480_held_out", builds, fcalls, mcalls, tfs, tms, truths, err3,
            (builds[0], [call3(gb, df, tfs[0], fr["depth"], s, fr["cam"], True) for s in starts]))

    if "gazebo" in args.workloads:
        fr2 = replay.load_gazebo()
        maps = {}
        for k in (6, 14, 22):
            g2 = gpismap_amd.GPisMap()
            for i in range(k):
                g2.update(fr2[i]["thetas"], fr2[i]["ranges"], fr2[i]["pose"])
            g2.sync()
            df = gpismap_amd.DistanceField()
            g2.distance_field(field=df, **BOX2)
            maps[k] = (g2, df)
        for dt, deg in ((0.1, 2.0), (0.3, 5.0)):
            builds, fcalls, mcalls, tfs, tms, truths = [], [], [], [], [], []
            for k, (g2, df) in maps.items():
                builds.append(lambda g2=g2, df=df: g2.distance_field(field=df, **BOX2))
                start = perturb2(fr2[k]["pose"], dt, deg)
                tf, tm = gpismap_amd.Tracker(), gpismap_amd.Tracker()
                fcalls.append(call2(g2, df, tf, fr2[k], start, True))
                mcalls.append(call2(g2, df, tm, fr2[k], start, False))
                tfs.append(tf)
                tms.append(tm)
                truths.append(fr2[k]["pose"])
            g2, df = maps[14]
            starts = [perturb2(fr2[14]["pose"], dt, deg, tdir=(np.cos(a), np.sin(a)))
                      for a in np.linspace(0, 2 * np.pi, args.frames, endpoint=False)]
            run("gazebo_270_beams_from_%gm_%gdeg" % (dt, deg), builds, fcalls, mcalls, tfs, tms, truths, err2,
                (builds[1], [call2(g2, df, tfs[1], fr2[14], s, True) for s in starts]))
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
