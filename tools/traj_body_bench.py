"""Benchmark of smoothing for the robot's footprint (gpis_smooth_body_optimize).  Workloads: tools/traj_bench.py's
fields, goal and 1000 random free starts, the planner's paths resampled to N in --waypoints.  Per workload and N it prints one
JSON line per footprint of --balls balls (a row of equal balls along the body's x axis, 12 lattice steps long, radius 1.5
steps) with
  - point_ms: the wall time inside gpis_traj_optimize (the point) on the same input, in the same process (median of --repeats):
    the yardstick,
  - body_ms: the same of gpis_smooth_body_optimize with the defaults for that footprint, body_over_point their ratio,
  - iterations (min / median / max) of both and the counts of status 0 / 1 / 2,
  - body_free_point / body_free_body: the share of trajectories with an input whose body result (the point's through
    gpis_body_traj_clearance) does not collide,
  - host_ms: tests/traj_body_ref.py on the same input (the host route; skipped with --no-host), and whether its bits equal the
    device's.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 600 python tools/traj_body_bench.py --workloads syn256 &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -o trajbody -- python tools/traj_body_bench.py --workloads syn256 --no-host"""
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


def row_of_balls(dim, balls, step):
    """(offset [balls, dim], radius [balls]): centres spread over 12 steps along x (one ball: the reference point itself)."""
    off = np.zeros((balls, dim), np.float64)
    if balls > 1:
        off[:, 0] = np.linspace(-6.0, 6.0, balls) * step
    return off, np.full(balls, 1.5 * step, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--waypoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--balls", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--workloads", nargs="+", default=["syn256", "gazebo"])
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

    def med_opt(fn, tj):
        fn()
        t = []
        for _ in range(args.repeats):
            fn()
            t.append(tj.info()["ms"])
        return float(np.median(t))

    df = gpismap_amd.DistanceField()
    pl = gpismap_amd.Planner()
    tj = gpismap_amd.Trajectories()
    for w in args.workloads:
        if w == "syn256":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
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
        pl.solve(df, goal)
        pl.paths(starts)
        for N in args.waypoints:
            tj.from_paths(pl, N)
            x0 = tj.optimize(df, iters=0).get()
            ist = np.where(x0["status"] == 2, 2, 0).astype(np.uint8)
            ok = ist == 0
            point_ms = med_opt(lambda: tj.optimize(df), tj)
            pt = tj.get()
            for balls in args.balls:
                off, rad = row_of_balls(dim, balls, b["step"])
                fp = gpismap_amd.Footprint(dim).set(off, rad)
                pfree = tj.optimize(df).body_clearance(fp, df)["collides"][ok] == 0
                body_ms = med_opt(lambda: tj.optimize(df, footprint=fp), tj)
                got, body = tj.get(), tj.body_result()
                it_p, it_b = pt["iterations"][ok], got["iterations"][ok]
                r = {"workload": w, "shape": list(shape), "N": N, "balls": balls, "trajectories": int(ok.sum()), "repeats": args.repeats,
                     "point_ms": point_ms, "body_ms": body_ms, "body_over_point": body_ms / point_ms,
                     "iterations_point": [int(it_p.min()), float(np.median(it_p)), int(it_p.max())] if it_p.size else [],
                     "iterations_body": [int(it_b.min()), float(np.median(it_b)), int(it_b.max())] if it_b.size else [],
                     "status": np.bincount(got["status"], minlength=3).tolist(),
                     "body_free_point": float(pfree.mean()) if ok.any() else None,
                     "body_free_body": float((body["collides"][ok] == 0).mean()) if ok.any() else None}
                if not args.no_host:
                    import body_ref
                    import traj_body_ref
                    import traj_ref
                    o, wt = gpismap_amd.traj_body_opts(dim, np.float32(b["step"]), balls)
                    opts = {k: getattr(o, k) for k in traj_ref.OPT_NAMES}
                    t0 = time.perf_counter()
                    ref = traj_body_ref.optimize(dist, shape, b["origin"], b["step"], body_ref.make(dim, off, rad), x0["x"], ist, opts, wt)
                    r["host_ms"] = (time.perf_counter() - t0) * 1e3
                    r["host_over_body"] = r["host_ms"] / body_ms
                    r["host_bits_equal"] = bool(np.array_equal(ref["x"].view(np.uint32), got["x"].view(np.uint32)) and
                                                np.array_equal(ref["D_min"].view(np.uint64), body["D_min"].view(np.uint64)))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
