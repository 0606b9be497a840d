"""Trajectory-smoothing benchmark (gpis_traj_*).  Workloads: tools/plan_bench.py's fields (the synthetic F = 5 map at the cubic
steps of (256, 192, 64) and (512, 384, 128), bigbird at 2.5 mm, gazebo at 0.1 m), its goal and its 1000 random free starts.  Per
workload and N in --waypoints it prints one JSON line with
  - solve_ms / paths_ms: the planner's solve and gpis_plan_paths in the same process (medians of --repeats),
  - traj_ms: gpis_traj_from_paths + gpis_traj_optimize with the default options through Python (median), opt_ms the wall time
    inside gpis_traj_optimize alone, resample_ms the rest (medians over the same calls),
  - iterations (min / median / max) and the counts of status 0 / 1 / 2,
  - collision_free_before / _after: the share of trajectories with an input that do not collide at iters = 0 and after the run,
  - length_before / _after: mean length,
  - host_ms: tests/traj_ref.py on the same resampled input (the host route it replaces; skipped with --no-host), and whether
    its bits equal the device's.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 600 python tools/traj_bench.py --workloads syn256 &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -o traj -- python tools/traj_bench.py --workloads syn256 --no-host &&
  python profiles/summarize_rocpd.py DIR/traj_results.db
(profiles/traj_kernel_stats.txt)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--waypoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--workloads", nargs="+", default=["syn256", "bigbird", "gazebo"])
    ap.add_argument("--no-host", action="store_true", help="skip the numpy reference (profiler runs)")
    args = ap.parse_args()

    import gpismap_amd
    import replay

    def get_map(name):
        if name == "syn":
            gm = gpismap_amd.GPisMap3()
            for f in range(5):
                gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        elif name == "bigbird":
            frames = replay.load_bigbird()
            gm = gpismap_amd.GPisMap3(frames[0]["cam"])
            for i in range(5):
                if i:
                    gm.set_camera(frames[i]["cam"])
                gm.update(frames[i]["depth"], frames[i]["pose"])
        else:
            gm = gpismap_amd.GPisMap()
            for fr in replay.load_gazebo():
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
        gm.sync()
        return gm

    def med(fn):
        fn()
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    df = gpismap_amd.DistanceField()
    pl = gpismap_amd.Planner()
    tj = gpismap_amd.Trajectories()
    for w in args.workloads:
        if w == "syn256":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
        elif w == "syn512":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 128, shape=(512, 384, 128))
        elif w == "bigbird":
            gm, b = get_map("bigbird"), dict(origin=(-0.07, -0.10, 0.0), step=0.0025, shape=(81, 97, 113))
        else:
            gm, b = get_map("gazebo"), dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
        shape, dim = b["shape"], len(b["shape"])
        gm.distance_field(field=df, **b)
        dist = df.get()[0].ravel()
        free = np.flatnonzero(dist >= 0)
        p0 = int(free[0])
        cell = (p0 % shape[0], (p0 // shape[0]) % shape[1], p0 // (shape[0] * shape[1]))[:dim]
        goal = (np.array(b["origin"], np.float64) + np.array(cell) * b["step"]).astype(np.float32)[None]
        rng = np.random.default_rng(0)
        sp0 = free[rng.integers(0, free.size, args.paths)]
        sc = np.stack([sp0 % shape[0], (sp0 // shape[0]) % shape[1], sp0 // (shape[0] * shape[1])], axis=1)[:, :dim]
        starts = (np.array(b["origin"], np.float64) + sc * b["step"]).astype(np.float32)
        solve_ms = med(lambda: pl.solve(df, goal))
        paths_ms = med(lambda: pl.paths(starts))
        paths, _, pst = pl.paths(starts)
        for N in args.waypoints:
            df.smooth(pl, N=N, trajectories=tj)
            tw, to = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                df.smooth(pl, N=N, trajectories=tj)
                tw.append((time.perf_counter() - t0) * 1e3)
                to.append(tj.info()["ms"])
            traj_ms, opt_ms = float(np.median(tw)), float(np.median(to))
            resample_ms = float(np.median(np.array(tw) - np.array(to)))
            after = tj.get()
            before = df.smooth(pl, N=N, trajectories=tj, iters=0).get()
            ok = after["status"] != 2
            it = after["iterations"][ok]
            r = {"workload": w, "shape": list(shape), "N": N, "trajectories": int(ok.sum()), "repeats": args.repeats,
                 "solve_ms": solve_ms, "paths_ms": paths_ms, "traj_ms": traj_ms, "opt_ms": opt_ms, "resample_ms": resample_ms,
                 "traj_over_solve": traj_ms / solve_ms,
                 "iterations": [int(it.min()), float(np.median(it)), int(it.max())] if it.size else [],
                 "status": np.bincount(after["status"], minlength=3).tolist(),
                 "collision_free_before": float((before["collides"][ok] == 0).mean()) if ok.any() else None,
                 "collision_free_after": float((after["collides"][ok] == 0).mean()) if ok.any() else None,
                 "length_before": float(before["length"][ok].mean()) if ok.any() else None,
                 "length_after": float(after["length"][ok].mean()) if ok.any() else None}
            if not args.no_host:
                import traj_ref
                o = gpismap_amd.traj_opts(dim, np.float32(b["step"]))
                opts = {k: getattr(o, k) for k in traj_ref.OPT_NAMES}
                t0 = time.perf_counter()
                ref = traj_ref.optimize(dist, shape, b["origin"], b["step"], before["x"], np.where(before["status"] == 2, 2, 0).astype(np.uint8), opts)
                r["host_ms"] = (time.perf_counter() - t0) * 1e3
                r["host_over_traj"] = r["host_ms"] / traj_ms
                r["host_bits_equal"] = bool(np.array_equal(ref["x"].view(np.uint32), after["x"].view(np.uint32)))
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
