"""Time-planner benchmark (gpis_tplan_*).  Workloads: the gazebo map's 2-D field (249 x 199, step 0.1) and a 2-D
slice of the synthetic 3-D field (256 x 192, the layer through the middle of its z range, rebuilt as a 2-D field from the
slice's signs); the goal is the first free lattice point, 1000 starts are random free points; n balls scattered over the
field's box with speeds up to 0.25 m/s scaled by the step, radius two lattice steps, t_begin = 0; slot 0.1.  Per workload, S in
--horizons and n in --balls it prints one JSON line with
  - solve_ms: TimePlanner.solve through Python with the default schedule (median of --repeats), solve_L1_ms: one layer per
    launch, solve_nocull_ms: the broad phase off; the triples the broad phase skipped and the share of points served at slot 0,
  - paths_ms (1000 starts, host copies included), check_ms, controls_ms (T = --steps); solve_ms_all .. controls_ms_all: every
    repeat, the spread a comparison between two builds needs,
  - plan_ms: Planner.solve on the same field in the same process; retime_ms: Trajectories.retime of the static routes (N = 64,
    smoothed and timed with the defaults) against the same balls: what the new stage is set against, with the statuses of both,
  - host_solve_ms: tests/tplan_ref.py on --host-layers layers, scaled to S (the host route; skipped with --no-host), and whether
    its policy bytes equal the device's on those layers.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 900 python tools/tplan_bench.py --workloads gazebo &&
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -d DIR -o tplan -- python tools/tplan_bench.py --workloads gazebo --no-host &&
  python profiles/summarize_rocpd.py DIR/tplan_results.db
(profiles/tplan_*)."""
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
SLOT = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--horizons", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--balls", type=int, nargs="+", default=[0, 8, 64, 256])
    ap.add_argument("--layers", type=int, nargs="+", default=[], help="further layers-per-launch values to time")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synslice"])
    ap.add_argument("--host-layers", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy reference (profiler runs)")
    args = ap.parse_args()

    import torch
    import gpismap_amd
    import replay

    def med(fn):
        fn()
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med.all = t
        return float(np.median(t))

    df = gpismap_amd.DistanceField()
    pl = gpismap_amd.Planner()
    tj = gpismap_amd.Trajectories()
    tp = gpismap_amd.TimePlanner()
    T = args.steps
    for w in args.workloads:
        if w == "gazebo":
            gm = gpismap_amd.GPisMap()
            for fr in replay.load_gazebo():
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
            gm.sync()
            b = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
            gm.distance_field(field=df, **b)
        else:
            gm = gpismap_amd.GPisMap3()
            for f in range(5):
                gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
            gm.sync()
            b3 = dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
            gm.distance_field(field=df, **b3)
            sl = np.ascontiguousarray(df.get()[0].reshape(64, 192, 256)[32], np.float32)
            b = dict(origin=LO[:2], step=b3["step"], shape=(256, 192))
            g = torch.from_numpy(sl.ravel()).to("cuda")
            df.from_grid(g.data_ptr(), b["shape"], b["origin"], b["step"], 0.0)
        shape, step = b["shape"], b["step"]
        dist = df.get()[0].ravel()
        free = np.flatnonzero(dist >= 0)
        p0 = int(free[0])
        lo = np.array(b["origin"], np.float64)
        hi = lo + (np.array(shape, np.float64) - 1) * step
        goal = (lo + np.array((p0 % shape[0], p0 // shape[0])) * step).astype(np.float32)[None]
        rng = np.random.default_rng(0)
        sp0 = free[rng.integers(0, free.size, args.paths)]
        starts = (lo + np.stack([sp0 % shape[0], sp0 // shape[0]], axis=1) * step).astype(np.float32)
        plan_ms = med(lambda: pl.solve(df, goal))
        pl.paths(starts)
        df.smooth(pl, N=64, trajectories=tj)
        tj.time(df)
        for n in args.balls:
            brng = np.random.default_rng(1000 + n)
            centre = lo + (hi - lo) * brng.random((n, 2))
            velocity = brng.uniform(-2.5 * step, 2.5 * step, (n, 2))
            radius = np.full(n, 2.0 * step)
            ob = gpismap_amd.Obstacles(2, step)
            ob.set(centre, velocity, radius, epoch=0.0)
            retime_ms = med(lambda: tj.retime(ob, slot=SLOT, max_pause=255))
            rstat = np.bincount(tj.retimed()["status"], minlength=5).tolist()
            for S in args.horizons:
                kw = dict(slot=SLOT, horizon=S)
                r = {"workload": w, "shape": list(shape), "S": S, "balls": n, "slot": SLOT, "T": T, "paths": args.paths,
                     "repeats": args.repeats, "plan_ms": plan_ms, "retime_ms": retime_ms, "retime_status": rstat}
                for L in args.layers:
                    tp.set_schedule(L, 1)
                    r["solve_L%d_ms" % L] = med(lambda: tp.solve(df, goal, ob, **kw))
                tp.set_schedule(1, 1)
                r["solve_L1_ms"] = med(lambda: tp.solve(df, goal, ob, **kw))
                tp.set_schedule(0, 0)
                r["solve_nocull_ms"] = med(lambda: tp.solve(df, goal, ob, **kw))
                tp.set_schedule(0, 1)
                r["solve_ms"] = med(lambda: tp.solve(df, goal, ob, **kw))
                r["solve_ms_all"] = med.all
                i = tp.info()
                r.update(solve_inner_ms=i["solve_ms"], layer_launches=i["layer_launches"], skipped=i["skipped"],
                         served=i["finite0"] / max(i["free"], 1), solve_over_plan=r["solve_ms"] / plan_ms,
                         solve_over_retime=r["solve_ms"] / retime_ms)
                r["paths_ms"] = med(lambda: tp.paths(starts))
                r["paths_ms_all"] = med.all
                pa = tp.paths(starts)
                r["check_ms"] = med(lambda: tp.check(ob))
                r["check_ms_all"] = med.all
                r["controls_ms"] = med(lambda: tp.controls(T))
                r["controls_ms_all"] = med.all
                ck = tp.check(ob)
                r.update(status=np.bincount(pa["status"], minlength=5).tolist(), arrive_max=int(pa["arrive"].max()),
                         collides=int(ck["collides"].sum()))
                if not args.no_host:
                    import obst_ref
                    import tplan_ref
                    k = min(args.host_layers, S)
                    So = obst_ref.make(2, centre, velocity, radius, epoch=0.0, step=step)
                    o = dict(tplan_ref.default_opts(step), slot=SLOT, horizon=k)
                    t0 = time.perf_counter()
                    ref = tplan_ref.solve(dist, shape, b["origin"], step, goal, So, 0.0, o)
                    r["host_layers"] = k
                    r["host_solve_ms"] = (time.perf_counter() - t0) * 1e3 * S / k
                    r["host_over_solve"] = r["host_solve_ms"] / r["solve_ms"]
                    tp.solve(df, goal, ob, slot=SLOT, horizon=k)
                    r["host_equal"] = bool(np.array_equal(tp.get()["policy"].reshape(k + 1, -1), ref["policy"]))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
