"""View-scoring benchmark (gpis*_view_gain_*).  Workloads: tools/cover_bench.py's fields and masks -- the synthetic F = 5 map on the
bench box at the cubic steps of the shapes (256, 192, 64) and (512, 384, 128), each after one integrated 640 x 480 synthetic depth
frame, scored for m = 256 poses of an 80 x 60 camera around the map's own view; gazebo on the demo grid at 0.1 m after one of its
scans, scored for m = 256 poses of that scan's beams around its pose.  Default options.  Per workload it prints one JSON line with
  - call_ms: wall time of one gpis3_view_gain_depth / gpis2_view_gain_scan (median of --repeats), and the holder's own stage
    times of the median call: predict_ms, table_ms (2-D), target_ms, gather_ms,
  - targets, rays, samples, hits; rules_per_s = targets x poses / gather_ms; rays_per_s = poses x rays / predict_ms,
  - loop_ms: the host route in the same process, composed from the single-pose entries -- per pose render_*_field, the misses
    filled, the mask uploaded into a scratch coverage, the frame integrated, the mask read back and counted (--loop-poses of
    the poses, scaled to all of them) -- and loop_equal: whether its counts equal the batch's,
  - ref_ms: tests/view_ref.py on the first --ref-poses poses (scaled to all of them; skipped with --no-ref and above
    --ref-limit lattice points), and ref_equal.
The kernel times come from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o view -- python tools/view_bench.py --repeats 3 --no-ref --loop-poses 0
  python profiles/summarize_rocpd.py DIR/view_results.db
(profiles/view_kernel_stats.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LO = (-0.60, -0.45, 0.85)
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
CAM80 = (71.0, 71.0, 38.75, 28.0, 80, 60)              # the map's camera at an eighth of its resolution
OFF2 = (0.08, 0.0)


def med(f, repeats):
    ts, infos = [], []
    for k in range(repeats + 1):                          # (the first call warms up and is dropped)
        t0 = time.perf_counter()
        infos.append(f())
        ts.append((time.perf_counter() - t0) * 1e3)
    ts, infos = ts[1:], infos[1:]
    return float(np.median(ts)), ts, infos[int(np.argsort(ts)[len(ts) // 2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--workloads", nargs="+", default=["syn256", "syn512", "gazebo"])
    ap.add_argument("--loop-poses", type=int, default=32, help="poses the composed host route is run on (0: skip it)")
    ap.add_argument("--ref-poses", type=int, default=4, help="poses the numpy reference is run on")
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy reference (profiler runs)")
    ap.add_argument("--ref-limit", type=int, default=4 * 10 ** 6, help="largest lattice the numpy reference is run on")
    args = ap.parse_args()

    import gpismap_amd
    import replay

    maps = {}

    def get_map(name):
        if name in maps:
            return maps[name]
        if name == "syn":
            gm = gpismap_amd.GPisMap3()
            for f in range(5):
                gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        else:
            gm = gpismap_amd.GPisMap()
            for fr in replay.load_gazebo():
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
        gm.sync()
        maps[name] = gm
        return gm

    df = gpismap_amd.DistanceField()
    cv, scratch = gpismap_amd.Coverage(), gpismap_amd.Coverage()
    v = gpismap_amd.ViewScorer()
    m = args.poses
    rng = np.random.default_rng(7)
    for w in args.workloads:
        if w == "syn256":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
        elif w == "syn512":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 128, shape=(512, 384, 128))
        else:
            gm, b = get_map("gazebo"), dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
        shape, dim = b["shape"], len(b["shape"])
        npts = int(np.prod(shape))
        gm.distance_field(field=df, **b)
        step = df.info()["step"]
        cv.reset(df)
        if dim == 3:
            gm.cover_depth(cv, replay.synthetic_depth(2), replay.IDENTITY_POSE)
            # the map's own view shifted up to 0.15 m sideways and turned up to 0.3 rad about the optical axis and the vertical
            off = np.stack([rng.uniform(-0.15, 0.15, m), rng.uniform(-0.1, 0.1, m), rng.uniform(-0.05, 0.05, m)], axis=1)
            rv = np.stack([np.zeros(m), rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m)], axis=1)
            poses = np.concatenate([gpismap_amd.pose_grid3(replay.IDENTITY_POSE, off[k:k + 1], rv[k:k + 1]) for k in range(m)])
            rays = CAM80[4] * CAM80[5]
            call = lambda: df.view_gain_depth(cv, CAM80, poses, scorer=v)
        else:
            fr = replay.load_gazebo()[14]
            gm.cover_scan(cv, fr["thetas"], fr["ranges"], fr["pose"])
            th = np.arctan2(fr["pose"][3], fr["pose"][2])
            poses = np.concatenate([gpismap_amd.pose_grid2([fr["pose"][0] + rng.uniform(-1.0, 1.0)], [fr["pose"][1] + rng.uniform(-1.0, 1.0)],
                                                           [th + rng.uniform(-3.1, 3.1)]) for _ in range(m)])
            rays = int(np.asarray(fr["thetas"]).size)
            call = lambda: df.view_gain_scan(cv, fr["thetas"], poses, OFF2, scorer=v)
        seen = cv.get().ravel()

        def timed():
            call()
            return v.info()
        call_ms, call_all, inf = med(timed, args.repeats)
        gain, hits = v.get()
        r = {"workload": w, "shape": list(shape), "step": b["step"], "lattice_points": npts, "seen": int(seen.sum()), "poses": m,
             "rays": rays, "repeats": args.repeats, "call_ms": call_ms, "call_ms_all": call_all,
             "predict_ms": inf["predict_ms"], "table_ms": inf["table_ms"], "target_ms": inf["target_ms"], "gather_ms": inf["gather_ms"],
             "targets": inf["targets"], "samples": inf["samples"], "hits": int(hits.sum()), "gain_min": int(gain.min()),
             "gain_max": int(gain.max()),
             "rules_per_s": inf["targets"] * m / (inf["gather_ms"] * 1e-3) if inf["gather_ms"] > 0 else None,
             "rays_per_s": m * rays / (inf["predict_ms"] * 1e-3)}
        if args.loop_poses > 0:
            n = min(m, args.loop_poses)
            miss = gpismap_amd.view_opts(dim, step).miss
            scratch.reset(df)
            base = int(seen.sum())

            def loop():
                out = np.zeros(n, np.int64)
                for k in range(n):
                    if dim == 3:
                        d, _, status = df.render_depth(poses[k], CAM80)
                        d = np.where(status == 0, d, np.float32(miss)).astype(np.float32)
                        out[k] = int(scratch.set(seen).integrate_depth(d, poses[k], CAM80).get().sum()) - base
                    else:
                        d, _, status = df.render_scan(fr["thetas"], poses[k], OFF2)
                        d = np.where(status == 0, d, np.float32(miss)).astype(np.float32)
                        out[k] = int(scratch.set(seen).integrate_scan(fr["thetas"], d, poses[k], OFF2).get().sum()) - base
                return out
            loop_ms, _, got = med(loop, max(1, args.repeats // 2))
            r.update(loop_poses=n, loop_ms=loop_ms * m / n, loop_equal=bool(np.array_equal(got, gain[:n])),
                     loop_over_call=loop_ms * m / n / call_ms)
        if not args.no_ref and npts <= args.ref_limit:
            import view_ref
            n = min(m, args.ref_poses)
            dist = df.get()[0].ravel()
            t0 = time.perf_counter()
            if dim == 3:
                rg, rh, _ = view_ref.gain_depth(dist, seen, shape, b["origin"], step, CAM80, poses[:n])
            else:
                rg, rh, _ = view_ref.gain_scan(dist, seen, shape, b["origin"], step, fr["thetas"], OFF2, poses[:n])
            r.update(ref_poses=n, ref_ms=(time.perf_counter() - t0) * 1e3 * m / n,
                     ref_equal=bool(np.array_equal(rg, gain[:n]) and np.array_equal(rh, hits[:n])))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
