"""Time-pose-planner benchmark (gpis_tpplan_*).  Workloads: tools/tplan_bench.py's -- the gazebo map's 2-D field
(249 x 199, step 0.1) and a 2-D slice of the synthetic 3-D field (256 x 192); the goal is the lattice point with a free heading nearest the median of
such points, at every heading, 1000 starts are random free points at heading -1; n balls scattered over the field's box with speeds up to 0.25 m/s
scaled by the step, radius two lattice steps, t_begin = 0; slot 0.1.  The footprint is Footprint.box(1.0, 0.4, 5) on the gazebo
field and the same box in lattice units (10 x 4 steps) on the slice, whose step is 4.7 mm.  Per workload, H in --headings and n
in --balls it prints one JSON line with
  - solve_ms: TimePosePlanner.solve through Python with the broad phase on (median of --repeats), solve_nocull_ms: one call with
    it off; the triples the broad phase skipped and the share of free states served at slot 0,
  - paths_ms (1000 starts, host copies included), check_ms, controls_ms (T = --steps), statuses and the longest arrival;
    solve_ms_all .. controls_ms_all: every repeat, the spread a comparison between two builds needs,
  - tplan_ms: TimePlanner.solve and pplan_ms: PosePlanner.solve on the same field, set and footprint in the same process: the
    yardsticks (tplan_ms x H x body balls is the naive product),
  - host_solve_ms: tests/tpplan_ref.py on --host-layers layers, scaled to S, with goals on a grid of three lattice steps so that
    every layer has candidates everywhere (the host route; only for H in --host-headings and n <= --host-balls, its arrays grow with states x n x body
    balls; skipped with --no-host), and whether its policy bytes equal the device's on those layers.
Every step that uses the GPU is one process under its own time limit; kernel statistics come from a run of their own:
  timeout -k 10 900 python tools/tpplan_bench.py --workloads gazebo &&
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -d DIR -o tpplan -- python tools/tpplan_bench.py --workloads gazebo --no-host &&
  python profiles/summarize_rocpd.py DIR/tpplan_results.db
(profiles/tpplan_*)."""
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
BOX = (1.0, 0.4, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--headings", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--balls", type=int, nargs="+", default=[0, 8, 64, 256])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synslice"])
    ap.add_argument("--host-layers", type=int, default=2)
    ap.add_argument("--host-balls", type=int, default=8)
    ap.add_argument("--host-headings", type=int, nargs="+", default=[16])
    ap.add_argument("--no-host", action="store_true", help="skip the numpy reference (profiler runs)")
    ap.add_argument("--no-nocull", action="store_true", help="skip the call with the broad phase off")
    args = ap.parse_args()

    import torch
    import gpismap_amd
    import replay

    def med(fn, repeats=args.repeats):
        fn()
        t = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med.all = t
        return float(np.median(t))

    def once(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    df = gpismap_amd.DistanceField()
    tpl = gpismap_amd.TimePlanner()
    ppl = gpismap_amd.PosePlanner()
    tp = gpismap_amd.TimePosePlanner()
    T, S = args.steps, args.horizon
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
        scale = step / 0.1
        boff, brad = gpismap_amd.Footprint.box_table(BOX[0] * scale, BOX[1] * scale, BOX[2])
        fp = gpismap_amd.Footprint(2).set(boff, brad)
        dist = df.get()[0].ravel()
        lo = np.array(b["origin"], np.float64)
        hi = lo + (np.array(shape, np.float64) - 1) * step
        rng = np.random.default_rng(0)
        for H in args.headings:
            kwp = dict(turn=0.5 * step)
            ppl.solve(df, fp, (lo + 0.5 * (hi - lo)).astype(np.float32)[None], H=H, **kwp)        # (for c: which points have a free heading)
            free = np.flatnonzero((ppl.get()[2] > 0).any(axis=0).ravel())
            fxy = np.stack([free % shape[0], free // shape[0]], axis=1)
            p0 = int(free[np.argmin(((fxy - np.median(fxy, axis=0)) ** 2).sum(axis=1))])       # the free point nearest the free points' median
            goal = (lo + np.array((p0 % shape[0], p0 // shape[0])) * step).astype(np.float32)[None]
            pplan_ms = med(lambda: ppl.solve(df, fp, goal, H=H, **kwp))
            sp0 = free[rng.integers(0, free.size, args.paths)]
            starts = (lo + np.stack([sp0 % shape[0], sp0 // shape[0]], axis=1) * step).astype(np.float32)
            for n in args.balls:
                brng = np.random.default_rng(1000 + n)
                centre = lo + (hi - lo) * brng.random((n, 2))
                velocity = brng.uniform(-2.5 * step, 2.5 * step, (n, 2))
                radius = np.full(n, 2.0 * step)
                ob = gpismap_amd.Obstacles(2, step)
                ob.set(centre, velocity, radius, epoch=0.0)
                kw = dict(slot=SLOT, horizon=S, **kwp)
                r = {"workload": w, "shape": list(shape), "H": H, "S": S, "balls": n, "body_balls": BOX[2], "slot": SLOT, "T": T,
                     "paths": args.paths, "repeats": args.repeats, "pplan_ms": pplan_ms}
                r["tplan_ms"] = med(lambda: tpl.solve(df, goal, ob, slot=SLOT, horizon=S))
                tp.set_schedule(1)
                r["solve_ms"] = med(lambda: tp.solve(df, goal, fp, ob, H=H, **kw))
                r["solve_ms_all"] = med.all
                i = tp.info()
                r.update(solve_inner_ms=i["solve_ms"], launches=i["launches"], skipped=i["skipped"], free=i["free"],
                         served=i["finite0"] / max(i["free"], 1), naive_ms=r["tplan_ms"] * H * BOX[2],
                         solve_over_naive=r["solve_ms"] / (r["tplan_ms"] * H * BOX[2]), solve_over_pplan=r["solve_ms"] / pplan_ms)
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
                if not args.no_nocull:
                    pol = tp.get()["policy"]
                    tp.set_schedule(0)
                    r["solve_nocull_ms"] = once(lambda: tp.solve(df, goal, fp, ob, H=H, **kw))
                    r["nocull_equal"] = bool(np.array_equal(tp.get()["policy"], pol))
                    tp.set_schedule(1)
                if not args.no_host and n <= args.host_balls and H in args.host_headings:
                    import body_ref
                    import obst_ref
                    import pplan_ref
                    import tpplan_ref
                    k = min(args.host_layers, S)
                    gi, gj = np.meshgrid(np.arange(1, shape[0], 3), np.arange(1, shape[1], 3))
                    grid = np.concatenate([lo + np.stack([gi.ravel(), gj.ravel()], axis=1) * step, np.full((gi.size, 1), -1.0)], axis=1).astype(np.float32)
                    So = obst_ref.make(2, centre, velocity, radius, epoch=0.0, step=step)
                    o = dict(tpplan_ref.default_opts(step, H), slot=SLOT, horizon=k, **kwp)
                    t0 = time.perf_counter()
                    ref = tpplan_ref.solve(dist, shape, b["origin"], step, body_ref.make(2, boff, brad), pplan_ref.heading_table(H),
                                           pplan_ref.heading_moves(H, "any"), grid, So, 0.0, o)
                    r["host_layers"] = k
                    r["host_solve_ms"] = (time.perf_counter() - t0) * 1e3 * S / k
                    r["host_over_solve"] = r["host_solve_ms"] / r["solve_ms"]
                    tp.solve(df, grid, fp, ob, H=H, slot=SLOT, horizon=k, **kwp)
                    r["host_equal"] = bool(np.array_equal(tp.get()["policy"].reshape(k + 1, -1), ref["policy"]))
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
