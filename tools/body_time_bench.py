"""Benchmark of the footprint in the moving-obstacle check and in re-timing (gpis_timed_body_*) on
tools/retime_bench.py's inputs: its fields, goal and 1000 random free starts, smoothed and timed with the default options; n balls
scattered over the field's box with speeds up to a quarter of v_max, radius two lattice steps, t_begin = 0; slot 0.1.  The
footprint is a row of --body equal balls along x, 10 lattice steps long and 4 wide (Footprint.box_table; 3-D: at the reference
point's height).  Per workload, N in --waypoints, n in --balls, body balls in --body and P in --pauses it prints one JSON line with
  - check_ms / body_check_ms: Trajectories.check without and with the footprint (dt = slot, steps = the point schedule's longest
    arrival, at most 4096), through Python, host copies included (median of --repeats),
  - retime_ms / body_retime_ms and their *_inner_ms (the wall time inside the library's solve alone),
  - retimed_check_ms / body_retimed_check_ms, each on its own schedule,
  - each body form over its point form on the same input in the same process, the schedule statuses of both solves,
  - host_*_ms: tests/body_time_ref.py's check, solve and sched_check on the first --host-rows trajectories, scaled to all of them
    (the host route; skipped with --no-host), and whether its integers and bits equal the device's on those rows.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 600 python tools/body_time_bench.py --workloads gazebo &&
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d DIR -o body_time -- python tools/body_time_bench.py --workloads gazebo --no-host &&
  python profiles/summarize_rocpd.py DIR/body_time_results.db"""
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
    ap.add_argument("--waypoints", type=int, nargs="+", default=[64])
    ap.add_argument("--balls", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--body", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--pauses", type=int, nargs="+", default=[63])
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "bigbird"])
    ap.add_argument("--host-rows", type=int, default=4)
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

    def same(a, b, keys):
        ok = True
        for k in keys:
            u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            ok = ok and bool(((u == v) | ((u != u) & (v != v))).all())
        return ok

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
                for nb in args.body:
                    off2, rho = gpismap_amd.Footprint.box_table(10.0 * b["step"], 4.0 * b["step"], nb)
                    off = np.zeros((nb, dim))
                    off[:, :2] = off2
                    fp = gpismap_amd.Footprint(dim).set(off, rho)
                    for P in args.pauses:
                        kw = dict(slot=SLOT, max_pause=P)
                        retime_ms, inner = med(lambda: tj.retime(ob, **kw), lambda: tj.retimed()["ms"])
                        s = tj.retimed()
                        steps = int(max(1, min(4096, s["arrive"].max())))
                        rcheck_ms = med(lambda: tj.retimed_check(ob, steps))[0]
                        check_ms = med(lambda: tj.check(ob, SLOT, steps))[0]
                        bcheck_ms = med(lambda: tj.check(ob, SLOT, steps, footprint=fp))[0]
                        bretime_ms, binner = med(lambda: tj.retime(ob, footprint=fp, **kw), lambda: tj.retimed()["ms"])
                        sb = tj.retimed()
                        brcheck_ms = med(lambda: tj.retimed_check(ob, steps, footprint=fp))[0]
                        after = tj.retimed_check(ob, steps, footprint=fp)
                        plain = tj.check(ob, SLOT, steps, footprint=fp)
                        r = {"workload": w, "shape": list(shape), "N": N, "balls": n, "body": nb, "max_pause": P, "slot": SLOT, "steps": steps,
                             "trajectories": int(tm["status"].size), "repeats": args.repeats, "check_ms": check_ms, "body_check_ms": bcheck_ms,
                             "retime_ms": retime_ms, "retime_inner_ms": inner, "body_retime_ms": bretime_ms, "body_retime_inner_ms": binner,
                             "retimed_check_ms": rcheck_ms, "body_retimed_check_ms": brcheck_ms, "body_check_over_check": bcheck_ms / check_ms,
                             "body_retime_over_retime": bretime_ms / retime_ms, "body_retimed_check_over_retimed_check": brcheck_ms / rcheck_ms,
                             "status": np.bincount(s["status"], minlength=5).tolist(), "body_status": np.bincount(sb["status"], minlength=5).tolist(),
                             "own_slots_max": int(sb["own_slots"].max()), "body_pauses_max": int(sb["pauses"].max()),
                             "body_plain_collides": int(plain["collides"].sum()), "body_retimed_collides": int(after["collides"].sum())}
                        if not args.no_host:
                            import body_ref
                            import body_time_ref as btr
                            import obst_ref
                            import retime_ref
                            k = min(args.host_rows, tm["status"].size)
                            scale = tm["status"].size / k
                            S = obst_ref.make(dim, centre, velocity, radius, epoch=0.0, step=b["step"])
                            B = body_ref.make(dim, off, rho)
                            a = (res["x"][:k], tm["v"][:k], tm["t"][:k], tm["status"][:k])
                            o = dict(slot=SLOT, max_pause=P, clearance=sb["clearance"], press_on=0)
                            t0 = time.perf_counter()
                            hc = btr.check(*a, S, B, SLOT, steps, 0.0, 0.0, None)
                            t1 = time.perf_counter()
                            hs = btr.solve(*a, S, B, 0.0, o)
                            t2 = time.perf_counter()
                            hk = btr.sched_check(*a, hs, S, B, steps, None)
                            t3 = time.perf_counter()
                            r.update(host_rows=k, host_check_ms=(t1 - t0) * 1e3 * scale, host_retime_ms=(t2 - t1) * 1e3 * scale,
                                     host_retimed_check_ms=(t3 - t2) * 1e3 * scale)
                            r["host_equal"] = (same(hc, {q: plain[q][:k] for q in btr.CHECK_KEYS}, btr.CHECK_KEYS) and
                                               same(hs, {q: sb[q][:k] for q in retime_ref.RES_KEYS + ("own",)}, retime_ref.RES_KEYS + ("own",)) and
                                               same(hk, {q: after[q][:k] for q in btr.CHECK_KEYS}, btr.CHECK_KEYS))
                        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
