"""Pose-planner benchmark (gpis_pplan_*).  Workloads: the gazebo field of tools/plan_bench.py (249 x 199 at 0.1 m) with
box(1.0, 0.4, 5), and the middle z slice of the synthetic (256, 192, 64) field taken as a 2-D f grid (its step is 4.7 mm, so the
box there is 10 x 4 steps).  The goal is the free state cell nearest the last recorded robot position (gazebo) or the lattice
point of largest dist (slice), at every heading; default options except margin 0 and turn = half a step.  One JSON line per
workload and H in --headings, appended to --out.  It measures; no test asserts any of it.
  - point_solve_ms: Planner.solve on the same field towards the same point with the disc radius as clearance (median of
    --repeats), in the same process;
  - solve_ms: PosePlanner.solve (median), setup_ms: the library's wall time of the set-up kernel inside it, its share,
    solve_over_point, outer rounds, tile launches, states_relaxed_per_s = tile launches x 64 H / solve time;
  - setup_samples_per_s = nx ny H m / setup_ms, next to sample_samples_per_s of gpis_dfield_sample on as many device points;
  - project_ms: PosePlanner.project into a kept Planner; paths_ms: --paths pose paths from random free points without a
    heading, their total length (solve_ms_all, project_ms_all, paths_ms_all: every repeat, the spread a comparison between two
    builds needs);
  - host_ms: tests/pplan_ref.py (numpy body rule, heapq Dijkstra on the reversed graph) on the same input, and whether its bits
    equal the device's (skipped with --no-host).
Kernel statistics come from a run of their own:
  rocprofv3 --kernel-trace --stats -d DIR -o pplan -- python tools/pplan_bench.py --repeats 3 --no-host --out ''
  python profiles/summarize_rocpd.py DIR/pplan_results.db
(profiles/pplan_kernel_stats.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32 = np.float32
LO = (-0.60, -0.45, 0.85)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--headings", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synslice"])
    ap.add_argument("--moves", default="any")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy reference (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pplan_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import torch
    import gpismap_amd
    import replay

    dev = torch.device("cuda", 0)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    repeats = {}                                            # every repeat of the times a comparison between builds looks at

    def med(fn, key=None):
        fn()
        t = [timed(fn)[0] for _ in range(args.repeats)]
        if key:
            repeats[key + "_all"] = t
        return float(np.median(t))

    df = gpismap_amd.DistanceField()
    pl, proj, pp = gpismap_amd.Planner(), gpismap_amd.Planner(), gpismap_amd.PosePlanner()
    for w in args.workloads:
        if w == "gazebo":
            frames = replay.load_gazebo()
            gm = gpismap_amd.GPisMap()
            for fr in frames:
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
            gm.sync()
            b = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
            gm.distance_field(field=df, **b)
            length, width = 1.0, 0.4
            want = np.array(frames[-1]["pose"][:2], np.float64)
        else:
            g3 = gpismap_amd.GPisMap3()
            for f in range(5):
                g3.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
            g3.sync()
            d3 = gpismap_amd.DistanceField()
            g3.distance_field(field=d3, origin=LO, step=0.3 / 64, shape=(256, 192, 64))
            sl = np.ascontiguousarray(d3.get()[0][32], F32)                 # the slice's signed distances as the 2-D f grid
            b = dict(origin=LO[:2], step=0.3 / 64, shape=(256, 192))
            df.from_grid(torch.from_numpy(sl.ravel()).to(dev).data_ptr(), b["shape"], b["origin"], b["step"], 0.0)
            length, width = 10 * b["step"], 4 * b["step"]
            want = None
        nx, ny = b["shape"]
        step = float(F32(b["step"]))
        dist = df.get()[0].ravel()
        off, rad = gpismap_amd.Footprint.box_table(length, width, 5)
        fp = gpismap_amd.Footprint(2).set(off, rad)
        m = rad.size
        X = b["origin"][0] + np.arange(nx) * b["step"]
        Y = b["origin"][1] + np.arange(ny) * b["step"]
        for H in args.headings:
            opts = dict(clearance=0.0, margin=0.0, turn=0.5 * step)
            # the goal: a point with a free heading, found with a first solve towards a throw-away goal
            pp.solve(df, fp, [[X[0], Y[0]]], H=H, moves=args.moves, **opts)
            free2 = (pp.get()[2] > 0).any(axis=0).ravel()
            cand = np.flatnonzero(free2)
            if want is not None:
                gx, gy = cand % nx, cand // nx
                p0 = int(cand[np.argmin((X[gx] - want[0]) ** 2 + (Y[gy] - want[1]) ** 2)])
            else:
                p0 = int(cand[np.argmax(dist[cand])])
            goal = np.array([[X[p0 % nx], Y[p0 // nx]]], F32)
            point_ms = med(lambda: pl.solve(df, goal, clearance=float(rad[0]), margin=0.0))
            pinf = pl.info()
            solve_ms = med(lambda: pp.solve(df, fp, goal, H=H, moves=args.moves, **opts), "solve_ms")
            inf = pp.info()
            setups = []
            for _ in range(args.repeats):
                pp.solve(df, fp, goal, H=H, moves=args.moves, **opts)
                setups.append(pp.info()["setup_ms"])
            setup_ms = float(np.median(setups))
            nsamp = nx * ny * H * m
            xs = torch.rand((nsamp, 2), dtype=torch.float32, device=dev) * torch.tensor([(nx - 1) * step, (ny - 1) * step], device=dev) \
                + torch.tensor(list(b["origin"]), dtype=torch.float32, device=dev)
            out = torch.empty((nsamp, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            sample_ms = med(lambda: df.sample(xs.data_ptr(), m=nsamp, d_out=out.data_ptr()))
            del xs, out
            project_ms = med(lambda: pp.project(proj), "project_ms")
            rng = np.random.default_rng(0)
            sp = cand[rng.integers(0, cand.size, args.paths)]
            starts = np.stack([X[sp % nx], Y[sp // nx]], axis=1).astype(F32)
            paths_ms = med(lambda: pp.paths(starts), "paths_ms")
            st = pp.paths(starts)[3]
            r = {"workload": w, "shape": [nx, ny], "H": H, "step": step, "states": nx * ny * H, "body_balls": int(m), "moves": args.moves,
                 "repeats": args.repeats, "point_solve_ms": point_ms, "point_rounds": pinf["rounds"], "point_tile_launches": pinf["tile_launches"],
                 "solve_ms": solve_ms, "setup_ms": setup_ms, "setup_share": setup_ms / solve_ms, "solve_over_point": solve_ms / point_ms,
                 "rounds": inf["rounds"], "tile_launches": inf["tile_launches"], "free": inf["free"], "reachable": inf["reachable"],
                 "goals_kept": inf["goals_kept"], "max_cost": inf["max_cost"],
                 "states_relaxed_per_s": inf["tile_launches"] * 64 * H / (solve_ms * 1e-3),
                 "setup_samples": nsamp, "setup_samples_per_s": nsamp / (setup_ms * 1e-3), "sample_ms": sample_ms,
                 "sample_samples_per_s": nsamp / (sample_ms * 1e-3), "project_ms": project_ms, "projected_reachable": proj.info()["reachable"],
                 "paths": args.paths, "paths_ms": paths_ms, "path_states": int(pp.last_off[-1]), "paths_arrived": int((st == 0).sum()),
                 **repeats}
            if not args.no_host:
                import body_ref
                import pplan_ref
                g3_ = np.array([[goal[0, 0], goal[0, 1], -1]], F32)
                t0 = time.perf_counter()
                pb = pplan_ref.Problem(dist, b["shape"], b["origin"], b["step"], body_ref.make(2, off, rad), pplan_ref.heading_table(H),
                                       pplan_ref.heading_moves(H, args.moves), g3_, **opts)
                t1 = time.perf_counter()
                rc = pplan_ref.solve_dijkstra(pb)
                t2 = time.perf_counter()
                got = pp.get()
                r["host_ms"] = {"problem": (t1 - t0) * 1e3, "dijkstra": (t2 - t1) * 1e3, "total": (t2 - t0) * 1e3}
                r["host_over_solve"] = (t2 - t0) * 1e3 / solve_ms
                r["host_bits_equal"] = bool(np.array_equal(got[0].ravel().view(np.uint32), rc.view(np.uint32))
                                            and np.array_equal(got[2].ravel().view(np.uint32), pb.c.ravel().view(np.uint32)))
            line = json.dumps(r)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
