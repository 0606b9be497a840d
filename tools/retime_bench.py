"""Re-timing benchmark (gpis_retime_*).  Workloads: tools/traj_bench.py's fields, goal and 1000 random free starts,
smoothed and timed with the default options first; n balls scattered over the field's box with speeds up to a quarter of
v_max, radius two lattice steps, t_begin = 0; slot 0.1.  Per workload, N in --waypoints, n in --balls and P in --pauses it prints
one JSON line with
  - retime_ms: Trajectories.retime(obstacles) through Python, host copies of the schedule included (median of --repeats);
    retime_inner_ms: the wall time inside gpis_retime_solve alone (kernel and the status copy),
  - check_ms: Trajectories.check on the same input in the same process (dt = slot, steps = the longest arrival, at most 4096):
    what the new stages are set against; retimed_check_ms: Trajectories.retimed_check with the same steps,
  - controls_ms / retimed_controls_ms: Trajectories.controls(slot, T) and Trajectories.retimed_controls(T) at T = --steps,
  - each new stage over check_ms (controls: over controls_ms), the schedule statuses, the largest number of own slots and pauses,
  - host_retime_ms: tests/retime_ref.py on the first --host-rows trajectories, scaled to all of them (the host route; skipped
    with --no-host), and whether its integers equal the device's on those rows.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 600 python tools/retime_bench.py --workloads gazebo &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -o retime -- python tools/retime_bench.py --workloads gazebo --no-host &&
  python profiles/summarize_rocpd.py DIR/retime_results.db
(profiles/retime_*)."""
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
    ap.add_argument("--waypoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--balls", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--pauses", type=int, nargs="+", default=[63, 255])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--workloads", nargs="+", default=["syn256", "bigbird", "gazebo"])
    ap.add_argument("--host-rows", type=int, default=8)
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
        lo = np.array(b["origin"], np.float64)
        hi = lo + (np.array(shape, np.float64) - 1) * b["step"]
        vmax = float(gpismap_amd.timing_opts(dim, b["step"]).v_max)
        for N in args.waypoints:
            df.smooth(pl, N=N, trajectories=tj)
            res = tj.get()
            tm = tj.time(df)
            for n in args.balls:
                brng = np.random.default_rng(1000 + n)
                centre = lo + (hi - lo) * brng.random((n, dim))
                velocity = brng.uniform(-0.25 * vmax, 0.25 * vmax, (n, dim))
                radius = np.full(n, 2.0 * b["step"])
                ob = gpismap_amd.Obstacles(dim, b["step"])
                ob.set(centre, velocity, radius, epoch=0.0)
                for P in args.pauses:
                    kw = dict(slot=SLOT, max_pause=P)
                    retime_ms, inner = med(lambda: tj.retime(ob, **kw), lambda: tj.retimed()["ms"])
                    s = tj.retimed()
                    steps = int(max(1, min(4096, s["arrive"].max())))
                    check_ms = med(lambda: tj.check(ob, SLOT, steps))[0]
                    rcheck_ms = med(lambda: tj.retimed_check(ob, steps))[0]
                    ctl_ms = med(lambda: tj.controls(SLOT, T))[0]
                    rctl_ms = med(lambda: tj.retimed_controls(T))[0]
                    plain = tj.check(ob, SLOT, steps)
                    after = tj.retimed_check(ob, steps)
                    r = {"workload": w, "shape": list(shape), "N": N, "balls": n, "max_pause": P, "slot": SLOT, "T": T, "steps": steps,
                         "trajectories": int(tm["status"].size), "repeats": args.repeats, "retime_ms": retime_ms, "retime_inner_ms": inner,
                         "check_ms": check_ms, "retimed_check_ms": rcheck_ms, "controls_ms": ctl_ms, "retimed_controls_ms": rctl_ms,
                         "retime_over_check": retime_ms / check_ms, "retimed_check_over_check": rcheck_ms / check_ms,
                         "retimed_controls_over_controls": rctl_ms / ctl_ms, "status": np.bincount(s["status"], minlength=5).tolist(),
                         "own_slots_max": int(s["own_slots"].max()), "pauses_max": int(s["pauses"].max()),
                         "plain_collides": int(plain["collides"].sum()), "retimed_collides": int(after["collides"].sum())}
                    if not args.no_host:
                        import obst_ref
                        import retime_ref
                        k = min(args.host_rows, tm["status"].size)
                        S = obst_ref.make(dim, centre, velocity, radius, epoch=0.0, step=b["step"])
                        o = dict(slot=SLOT, max_pause=P, clearance=s["clearance"], press_on=0)
                        t0 = time.perf_counter()
                        ref = retime_ref.solve(res["x"][:k], tm["v"][:k], tm["t"][:k], tm["status"][:k], S, 0.0, o)
                        r["host_rows"] = k
                        r["host_retime_ms"] = (time.perf_counter() - t0) * 1e3 * tm["status"].size / k
                        r["host_over_retime"] = r["host_retime_ms"] / retime_ms
                        r["host_equal"] = all(bool(np.array_equal(ref[q], s[q][:k])) for q in retime_ref.RES_KEYS + ("own",))
                    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
