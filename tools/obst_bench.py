"""Moving-obstacle benchmark (gpis_obst_*), on tools/mppi_bench.py's two controller configurations and tools/timing_bench.py's
1000 timed trajectories.  One JSON line per record, appended to --out.
  --part step   per workload (gazebo: K = 4096, T = 64 with the planner; synthetic: K = 8192, T = 48 towards a goal point) and n
                in --balls (0 = the plain Controller.step): step_ms, one step + one shift through Python (median of --repeats),
                step_info_ms, the library's own wall time, the step's obstacle statistics, and host_ms, tests/obst_ref.py's
                step on the same input (--host-repeats, 0 = skip).
  --part plain  the plain Controller.step alone, n = 0: what is set against the parent commit's build.  The library is the one
                GPISMAP_AMD_LIB names, so the same script times either build; run them interleaved, A-B-A-B, a process each:
                  python tools/obst_bench.py --part plain --tag new
                  GPISMAP_AMD_LIB=<parent's libgpismap_amd.so> python tools/obst_bench.py --part plain --tag parent
  --part check  the synthetic field's 1000 trajectories of 64 waypoints, timed; Trajectories.check at --steps (256) and n in
                --balls without 0: check_ms (median of --repeats), collisions found, and host_ms of tests/obst_ref.py's check on
                the first --host-paths trajectories, scaled to all of them.
Every process that uses the GPU runs under its own time limit.  Kernel statistics come from a run of their own:
  rocprofv3 --kernel-trace --stats -d DIR -o obst -- python tools/obst_bench.py --part step --repeats 3 --host-repeats 0 --out ''
  python profiles/summarize_rocpd.py DIR/obst_results.db"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pf_bench import BOX2, SYN  # noqa: E402

F32 = np.float32
F64 = np.float64


def scatter(dim, n, lo, hi, step, seed=0):
    """n balls scattered over the box with speeds up to two lattice steps a second and radii of one to three steps."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    return (lo + (hi - lo) * rng.random((n, dim)), rng.uniform(-2.0, 2.0, (n, dim)) * step, rng.uniform(1.0, 3.0, n) * step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("step", "plain", "check"), default="step")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--host-paths", type=int, default=50)
    ap.add_argument("--balls", type=int, nargs="+", default=[0, 8, 64, 256])
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synthetic"])
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obst_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
    import mppi_ref
    import replay

    def emit(rec):
        rec = dict(part=args.part, tag=args.tag, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def controller_inputs(name):
        """(dim, field, K, T, pose, goal, planner, opts) of tools/mppi_bench.py's configuration `name`."""
        df = gpismap_amd.DistanceField()
        if name == "gazebo":
            fr2 = replay.load_gazebo()
            g2 = gpismap_amd.GPisMap()
            for k in range(14):
                g2.update(fr2[k]["thetas"], fr2[k]["ranges"], fr2[k]["pose"])
            g2.sync()
            g2.distance_field(field=df, **BOX2)
            pl = df.plan(np.asarray(fr2[0]["pose"][:2], F32)[None], planner=gpismap_amd.Planner(), clearance=0.0)
            return 2, df, 4096, 64, np.asarray(fr2[14]["pose"], F64), None, pl, dict(clearance=0.1)
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        gm.distance_field(field=df, **SYN)
        lo = np.array(SYN["origin"], F64)
        hi = lo + (np.array(SYN["shape"]) - 1) * SYN["step"]
        pose = mppi_ref.pose_of_state(list(lo + 0.1 * (hi - lo)) + [math.cos(0.5), math.sin(0.5)], 3)
        return 3, df, 8192, 48, pose, lo + 0.9 * (hi - lo), None, dict(dt=0.02, sigma=(0.25, 0.25, 0.25, 0.5), w_goal=20.0)

    def step_part(name, ns):
        import obst_ref
        dim, df, K, T, pose, goal, planner, opts = controller_inputs(name)
        i = df.info()
        lo = np.array(i["origin"][:dim], F64)
        hi = lo + (np.array(i["shape"][:dim]) - 1) * i["step"]
        for n in ns:
            ctl = gpismap_amd.Controller(**opts)
            ctl.init(dim, K, T, seed=1)
            ob, S = None, None
            if n > 0:
                c, v, r = scatter(dim, n, lo, hi, i["step"])
                ob = gpismap_amd.Obstacles(dim, i["step"]).set(c, v, r, epoch=0.0)
                S = obst_ref.make(dim, c, v, r, epoch=0.0, step=i["step"])
            clock = [0.0]

            def one():
                r_ = df.control(ctl, pose, goal=goal, planner=planner, obstacles=ob, t=clock[0]) if ob is not None else \
                    df.control(ctl, pose, goal=goal, planner=planner)
                ctl.shift()
                clock[0] += 0.1
                return r_

            for _ in range(3):                            # (warm-up; the nominal sequence leaves zero)
                one()
            ms, lib_ms = [], []
            for _ in range(args.repeats):
                t, (u0, info) = timed(one)
                ms.append(t)
                lib_ms.append(ctl.info()["ms"])
            rec = {"workload": name, "dim": dim, "rollouts": K, "horizon": T, "balls": n, "repeats": args.repeats,
                   "step_ms": float(np.median(ms)), "step_ms_all": ms, "step_info_ms": float(np.median(lib_ms)), "neff": info["neff"],
                   "nominal_cost": info["nominal_cost"]}
            if hasattr(gpismap_amd.lib(), "gpis_obst_mppi_get"):      # (the parent's library has none)
                rec.update(ctl.obstacle_stats())
            if args.host_repeats > 0 and args.part == "step":
                dist = df.get()[0].ravel()
                cost = planner.get()[0].ravel() if planner is not None else None
                o = mppi_ref.default_opts(dim, i["step"])
                o.update(opts)
                U = ctl.get()["U"]
                tick = ctl.info()["tick"] + 1
                hms = [timed(lambda: obst_ref.step(dist, i["shape"], i["origin"], i["step"], pose, U, 1, tick, K, o, cost, goal, obst=S,
                                                   t_now=clock[0]))[0] for _ in range(args.host_repeats)]
                rec.update(host_ms=float(np.median(hms)), host_over_step=float(np.median(hms)) / rec["step_ms"])
            emit(rec)

    def check_part():
        import obst_ref
        LO = (-0.60, -0.45, 0.85)
        b = dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df, pl, tj = gpismap_amd.DistanceField(), gpismap_amd.Planner(), gpismap_amd.Trajectories()
        gm.distance_field(field=df, **b)
        shape = b["shape"]
        dist = df.get()[0].ravel()
        free = np.flatnonzero(dist >= 0)
        cell = lambda p: np.stack([p % shape[0], (p // shape[0]) % shape[1], p // (shape[0] * shape[1])], axis=-1)
        goal = (np.array(LO, F64) + cell(int(free[0])) * b["step"]).astype(F32)[None]
        starts = (np.array(LO, F64) + cell(free[np.random.default_rng(0).integers(0, free.size, 1000)]) * b["step"]).astype(F32)
        pl.solve(df, goal)
        pl.paths(starts)
        df.smooth(pl, N=64, trajectories=tj)
        res = tj.get()
        tm = tj.time(df)
        dur = tm["duration"][tm["status"] == 0]
        dt = float(np.median(dur[dur > 0])) / (0.75 * args.steps)
        lo = np.array(LO, F64)
        hi = lo + (np.array(shape) - 1) * b["step"]
        for n in [k for k in args.balls if k > 0]:
            c, v, r = scatter(3, n, lo, hi, b["step"])
            ob = gpismap_amd.Obstacles(3, b["step"]).set(c, v, r, epoch=0.0)
            tj.check(ob, dt, args.steps)
            ms = [timed(lambda: tj.check(ob, dt, args.steps))[0] for _ in range(args.repeats)]
            got = tj.check(ob, dt, args.steps)
            rec = {"workload": "syn256_N64", "trajectories": int(res["x"].shape[0]), "timed": int((tm["status"] == 0).sum()), "steps": args.steps,
                   "dt": dt, "balls": n, "repeats": args.repeats, "check_ms": float(np.median(ms)), "check_ms_all": ms,
                   "collides": int(got["collides"].sum())}
            if args.host_repeats > 0:
                m = min(args.host_paths, res["x"].shape[0])
                S = obst_ref.make(3, c, v, r, epoch=0.0, step=b["step"])
                t, ref = timed(lambda: obst_ref.check(res["x"][:m], tm["v"][:m], tm["t"][:m], tm["status"][:m], S, dt, args.steps))
                same = all(np.array_equal(ref[k], got[k][:m], equal_nan=True) for k in ref)
                rec.update(host_paths=m, host_ms=t * res["x"].shape[0] / m, host_over_check=t * res["x"].shape[0] / m / rec["check_ms"],
                           host_bits_equal=bool(same))
            emit(rec)

    if args.part == "check":
        check_part()
    else:
        for w in args.workloads:
            step_part(w, [0] if args.part == "plain" else args.balls)


if __name__ == "__main__":
    main()
