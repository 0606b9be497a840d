"""Time-parametrisation benchmark (gpis_timing_*).  Workloads: tools/traj_bench.py's fields, goal and 1000 random free starts,
smoothed with the default options first.  Per workload and N in --waypoints it prints one JSON line with
  - opt_ms: the wall time inside gpis_traj_optimize (what the new stages are set against),
  - time_ms: Trajectories.time(df) with the default limits through Python, host copies of every output included (median of
    --repeats); time_inner_ms: the wall time inside gpis_timing_time alone (kernel and the status copy),
  - controls_ms / controls_inner_ms: Trajectories.controls(dt, T) at T = --steps, dt = the median duration / (0.75 T), with the
    copy of U to the host, and the time inside gpis_timing_controls,
  - follow_ms: Controller.follow of one timed trajectory into a controller of K = 256 rollouts and the same T,
  - each over opt_ms, the timing statuses, the median duration over length / v_max and the share of waypoints per limiter,
  - host_time_ms / host_controls_ms: tests/timing_ref.py on the same input (the host route; skipped with --no-host) and whether
    its bits equal the device's.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 600 python tools/timing_bench.py --workloads syn256 &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -o timing -- python tools/timing_bench.py --workloads syn256 --no-host &&
  python profiles/summarize_rocpd.py DIR/timing_results.db
(profiles/timing_kernel_stats.txt)."""
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
    ap.add_argument("--steps", type=int, default=64)
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

    def med(fn, inner=None):
        fn()
        t, ti = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
            if inner:
                ti.append(inner())
        return float(np.median(t)), (float(np.median(ti)) if inner else None)

    df = gpismap_amd.DistanceField()
    pl = gpismap_amd.Planner()
    tj = gpismap_amd.Trajectories()
    ctl = gpismap_amd.Controller()
    T = args.steps
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
        ctl.init(dim, 256, T, seed=1)
        for N in args.waypoints:
            df.smooth(pl, N=N, trajectories=tj)
            opt_ms = tj.info()["ms"]
            res = tj.get()
            time_ms, time_inner = med(lambda: tj.time(df), lambda: tj.timing_info()["time_ms"])
            tm = tj.time(df)
            ok = np.flatnonzero(tm["status"] == 0)
            dur = tm["duration"][ok]
            dt = float(np.median(dur[dur > 0])) / (0.75 * T) if (dur > 0).any() else 0.1
            ctl_ms, ctl_inner = med(lambda: tj.controls(dt, T), lambda: tj.timing_info()["controls_ms"])
            U, h0, q0, clamped = tj.controls(dt, T)
            index = int(ok[np.argmax(dur)]) if ok.size else 0
            follow_ms = med(lambda: ctl.follow(tj, index, dt))[0] if ok.size else None
            vmax = float(gpismap_amd.timing_opts(dim, b["step"]).v_max)
            counts = tm["limiter_counts"][ok].sum(axis=0)
            r = {"workload": w, "shape": list(shape), "N": N, "T": T, "dt": dt, "trajectories": int(ok.size), "repeats": args.repeats,
                 "opt_ms": opt_ms, "time_ms": time_ms, "time_inner_ms": time_inner, "controls_ms": ctl_ms,
                 "controls_inner_ms": ctl_inner, "follow_ms": follow_ms, "time_over_opt": time_ms / opt_ms,
                 "controls_over_opt": ctl_ms / opt_ms, "follow_over_opt": follow_ms / opt_ms if follow_ms else None,
                 "status": np.bincount(tm["status"], minlength=4).tolist(), "clamped_steps": int(clamped.sum()),
                 "duration_over_length": float(np.median(dur[dur > 0] / (res["length"][ok][dur > 0] / vmax))) if (dur > 0).any() else None,
                 "limiter_share": (counts / max(1, int(counts.sum()))).round(4).tolist()}
            if not args.no_host:
                import timing_ref
                o = gpismap_amd.timing_opts(dim, np.float32(b["step"]))
                opts = {k: getattr(o, k) for k in timing_ref.OPT_NAMES}
                t0 = time.perf_counter()
                ref = timing_ref.time(res["x"], res["status"], opts, (dist, shape, b["origin"], b["step"]))
                r["host_time_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                rc = timing_ref.controls(res["x"], ref["v"], ref["t"], ref["status"], dt, T)
                r["host_controls_ms"] = (time.perf_counter() - t0) * 1e3
                r["host_time_over_time"] = r["host_time_ms"] / time_ms
                r["host_controls_over_controls"] = r["host_controls_ms"] / ctl_ms
                same = lambda a, c: bool(np.array_equal(a, c, equal_nan=True))
                r["host_bits_equal"] = same(ref["v"], tm["v"]) and same(ref["t"], tm["t"]) and same(ref["limiter"], tm["limiter"]) and \
                    bool(np.array_equal(rc["U"].view(np.uint64), U.view(np.uint64)))
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
