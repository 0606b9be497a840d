"""Detector benchmark (gpis2_detect_scan_field / gpis3_detect_depth_field).  Workloads: gazebo scan 14 on the gazebo field (demo
grid at 0.1 m); one 640 x 480 synthetic depth frame at stride 1 and 2 on the synthetic F = 5 map's field at shape (256, 192, 64);
each with 0, 1 and 8 discs / spheres inserted into the measurement by a ray intersection (discs of 0.2 m half-way along a beam,
spheres of 0.02 m 0.06 m in front of the surface).  Default options.  Per workload and count it prints one JSON line with
  - detect_ms: wall time of one detect call (median of --repeats; the call returns with its work done), samples, foreign samples,
    components, balls, labelling rounds,
  - stage_ms: the stages' own times (set-up, flags, compaction, labelling, table) from calls that synchronise after every stage
    (Detector.set_schedule(profile=True)), and their sum,
  - track_pass_ms: one gpis*_track_*_field call with max_iters = 0 on the same frame in the same process (the set-up and one
    fused pass), detect_over_track,
  - host_ms: the host route -- tests/detect_ref.py on the same input and the device's dist -- and whether its label image and
    balls equal the device's (skipped with --no-host).
The kernel times come from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o detect -- python tools/detect_bench.py --repeats 3 --no-host
  python profiles/summarize_rocpd.py DIR/detect_results.db"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32, F64 = np.float32, np.float64
LO = (-0.60, -0.45, 0.85)
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
OFF2 = (0.08, 0.0)
COUNTS = (0, 1, 8)


def med(f, repeats):
    ts = []
    for _ in range(repeats + 1):                          # (the first call warms up and is dropped)
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), ts[1:]


def with_discs(thetas, ranges, n, radius=0.2):
    """The scan with n discs, each centred half-way along one of n evenly chosen beams that measured more than 2 m (sensor frame)."""
    r = np.asarray(ranges, F64).copy()
    far = np.nonzero((r > 2.0) & (r < 30.0))[0]
    a = np.asarray(thetas, F32).astype(F64)
    for k in far[np.linspace(0, far.size - 1, n + 2).astype(int)[1:-1]] if n else ():
        c = 0.5 * ranges[k] * np.array([np.cos(a[k]), np.sin(a[k])])
        b = c[0] * np.cos(a) + c[1] * np.sin(a)
        disc = b * b - (c @ c - radius * radius)
        with np.errstate(invalid="ignore"):
            t = b - np.sqrt(disc)
        r = np.where((disc >= 0) & (t > 0) & (t < r), t, r)
    return r.astype(F32)


def with_spheres(depth, cam6, n, radius=0.02, before=0.06):
    """The depth image (column-major) with n spheres, each centred `before` metres in front of what one of n evenly chosen valid
    pixels measured (the synthetic field is a slab of 0.3 m about the surface: farther out a sample is off the lattice)."""
    fx, fy, cx, cy, W, H = cam6
    W, H = int(W), int(H)
    d = np.asarray(depth, F64).reshape(W, H).copy()
    u = ((np.arange(W) - cx) / fx)[:, None] * np.ones((1, H))
    v = np.ones((W, 1)) * ((np.arange(H) - cy) / fy)[None, :]
    ok = np.nonzero(((d > 0.4) & (d < 4.0)).ravel())[0]
    a = u * u + v * v + 1.0
    for k in ok[np.linspace(0, ok.size - 1, n + 2).astype(int)[1:-1]] if n else ():
        z0 = d.ravel()[k] - before
        c = np.array([u.ravel()[k] * z0, v.ravel()[k] * z0, z0])
        b = u * c[0] + v * c[1] + c[2]
        disc = b * b - a * (c @ c - radius * radius)
        with np.errstate(invalid="ignore"):
            z = (b - np.sqrt(disc)) / a
        hit = (disc >= 0) & (z > 0.4) & ((z < d) | ~((d > 0.4) & (d < 4.0)))
        d = np.where(hit, z, d)
    return d.astype(F32).ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "syn_s1", "syn_s2"])
    ap.add_argument("--no-host", action="store_true", help="skip the host route (profiler runs)")
    args = ap.parse_args()

    import gpismap_amd
    import replay

    df = gpismap_amd.DistanceField()
    det, prof = gpismap_amd.Detector(), gpismap_amd.Detector().set_schedule(profile=True)
    trk = gpismap_amd.Tracker()
    built = None
    for w in args.workloads:
        dim = 2 if w == "gazebo" else 3
        if built != dim:
            if dim == 2:
                gm, b = gpismap_amd.GPisMap(), dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
                for fr in replay.load_gazebo():
                    gm.update(fr["thetas"], fr["ranges"], fr["pose"])
            else:
                gm, b = gpismap_amd.GPisMap3(), dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
                for f in range(5):
                    gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
            gm.sync()
            gm.distance_field(field=df, **b)
            dist, step, built = df.get()[0].ravel(), df.info()["step"], dim
        stride = 2 if w == "syn_s2" else 1
        for n in COUNTS:
            t = [0.0]

            def clock():
                t[0] += 0.1
                return t[0]

            if dim == 2:
                fr = replay.load_gazebo()[14]
                th, pose = np.asarray(fr["thetas"], F32), np.asarray(fr["pose"], F64)
                meas = with_discs(th, fr["ranges"], n)
                call = lambda d: df.detect_scan(th, meas, pose, OFF2, clock(), detector=d)
                track = lambda: df.track_scan(th, meas, pose.astype(F32), OFF2, tracker=trk, max_iters=0)
                frame, kw = (th, meas, OFF2), {}
            else:
                pose = np.asarray(replay.IDENTITY_POSE, F64)
                meas = with_spheres(replay.synthetic_depth(2), SYN_CAM, n)
                kw = dict(stride=stride)
                call = lambda d: df.detect_depth(meas, pose, SYN_CAM, clock(), detector=d, **kw)
                track = lambda: df.track_depth(meas, pose.astype(F32), SYN_CAM, tracker=trk, max_iters=0, stride=stride)
                frame = (meas, SYN_CAM)
            det.reset_tracks()
            prof.reset_tracks()
            detect_ms, detect_all = med(lambda: call(det), args.repeats)
            inf = det.info()
            stages = {k: [] for k in ("setup_ms", "flag_ms", "compact_ms", "label_ms", "table_ms")}
            for _ in range(args.repeats + 1):
                call(prof)
                for k in stages:
                    stages[k].append(prof.info()[k])
            stage_ms = {k: float(np.median(v[1:])) for k, v in stages.items()}
            track_ms, _ = med(track, args.repeats)
            r = {"workload": w, "inserted": n, "stride": stride, "repeats": args.repeats, "detect_ms": detect_ms, "detect_ms_all": detect_all,
                 "grid": inf["grid"], "samples": inf["samples"], "foreign": inf["foreign"], "components": inf["components"],
                 "balls": inf["balls"], "rounds": inf["rounds"], "stage_ms": stage_ms, "stage_sum_ms": float(sum(stage_ms.values())),
                 "track_pass_ms": track_ms, "detect_over_track": detect_ms / track_ms}
            if not args.no_host:
                import detect_ref
                det.reset_tracks()
                got = call(det)
                img = det.samples()["label"]
                t0 = time.perf_counter()
                ref = detect_ref.Detector().detect(dist, b["shape"], b["origin"], step, dim, frame, pose, 1.0, detect_ref.opts(dim, step, **kw))
                r["host_ms"] = (time.perf_counter() - t0) * 1e3
                r["host_equal"] = bool(np.array_equal(img, ref["label"]) and got["centre"].tobytes() == ref["balls"]["centre"].tobytes()
                                       and got["radius"].tobytes() == ref["balls"]["radius"].tobytes())
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
