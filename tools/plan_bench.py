"""Path-planning benchmark (gpis_plan_*).  Workloads: tools/dfield_bench.py's fields -- the synthetic F = 5 map on the bench box at
the cubic steps of the shapes (256, 192, 64) and (512, 384, 128), bigbird (5 frames) on the demo box at 2.5 mm, gazebo on the demo
grid at 0.1 m.  One goal at the free lattice point nearest the box's lower corner, default options (clearance 0, margin 4 steps,
gain 4, all diagonals).  Per workload it prints one JSON line with
  - field_ms: the field's own build in the same process (median of --repeats),
  - solve_ms: wall time of gpis_plan_solve (median), solve_over_field, outer rounds, tile launches,
    cells_relaxed_per_s = tile launches x points per tile / solve time,
  - paths_ms: gpis_plan_paths from --paths random free starts, and their total length in points
    (solve_ms_all, paths_ms_all: every repeat, the spread a comparison between two builds needs),
  - host_ms: the host route it replaces -- the same edge list as a scipy.sparse matrix and scipy.sparse.csgraph.dijkstra from
    the goal, timed with and without building the graph (float64 sums: the route, not the bits; skipped without scipy, with
    --no-host, and above --host-limit lattice points).
The planner's kernel times come from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o plan -- python tools/plan_bench.py --repeats 3 --no-host
  python profiles/summarize_rocpd.py DIR/plan_results.db
(profiles/plan_kernel_stats.txt)."""
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


def host_route(dist, shape, step, goal_cell, opts):
    import plan_ref
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    t0 = time.perf_counter()
    pb = plan_ref.Problem(dist, shape, (0.0,) * len(shape), step, np.array([goal_cell[:len(shape)]], np.float64) * step,
                          clearance=opts.clearance, margin=opts.margin, gain=opts.gain, connectivity=opts.connectivity)
    nz, ny, nx = pb.n3
    rows, cols, vals = [], [], []
    for k, o, e, w in pb.edges:
        p = np.flatnonzero(e.ravel())
        rows.append(p)
        cols.append(p + o[0] + nx * (o[1] + ny * o[2]))
        vals.append(w.ravel()[p].astype(np.float64))
    n = nx * ny * nz
    g = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    t1 = time.perf_counter()
    src = (goal_cell[2] * ny + goal_cell[1]) * nx + goal_cell[0] if len(shape) == 3 else goal_cell[1] * nx + goal_cell[0]
    d = dijkstra(g, directed=True, indices=[src])
    t2 = time.perf_counter()
    return {"graph": (t1 - t0) * 1e3, "dijkstra": (t2 - t1) * 1e3, "total": (t2 - t0) * 1e3}, d.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--workloads", nargs="+", default=["syn256", "syn512", "bigbird", "gazebo"])
    ap.add_argument("--no-host", action="store_true", help="skip the host route (profiler runs)")
    ap.add_argument("--host-limit", type=int, default=4 * 10 ** 6, help="largest lattice the host route is run on")
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
        maps[name] = gm
        return gm

    df = gpismap_amd.DistanceField()
    pl = gpismap_amd.Planner()
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
        npts = int(np.prod(shape))

        def field():
            t0 = time.perf_counter()
            gm.distance_field(field=df, **b)
            return (time.perf_counter() - t0) * 1e3

        field()
        field_ms = [field() for _ in range(args.repeats)]
        dist = df.get()[0].ravel()
        free = np.flatnonzero(dist >= 0)
        p0 = int(free[0])
        cell = (p0 % shape[0], (p0 // shape[0]) % shape[1], p0 // (shape[0] * shape[1]))[:dim]
        goal = (np.array(b["origin"], np.float64) + np.array(cell) * b["step"]).astype(np.float32)[None]

        def solve():
            t0 = time.perf_counter()
            pl.solve(df, goal)
            return (time.perf_counter() - t0) * 1e3

        solve()
        solve_ms = [solve() for _ in range(args.repeats)]
        inf = pl.info()
        tile = 32 * 32 if dim == 2 else 8 * 8 * 8
        r = {"workload": w, "shape": list(shape), "step": b["step"], "lattice_points": npts, "repeats": args.repeats,
             "field_ms": float(np.median(field_ms)), "solve_ms": float(np.median(solve_ms)), "solve_ms_all": solve_ms,
             "rounds": inf["rounds"], "tile_launches": inf["tile_launches"], "free": inf["free"], "reachable": inf["reachable"],
             "goals_kept": inf["goals_kept"], "max_cost": inf["max_cost"]}
        r["solve_over_field"] = r["solve_ms"] / r["field_ms"]
        r["cells_relaxed_per_s"] = inf["tile_launches"] * tile / (r["solve_ms"] * 1e-3)

        rng = np.random.default_rng(0)
        sp0 = free[rng.integers(0, free.size, args.paths)]
        sc = np.stack([sp0 % shape[0], (sp0 // shape[0]) % shape[1], sp0 // (shape[0] * shape[1])], axis=1)[:, :dim]
        starts = (np.array(b["origin"], np.float64) + sc * b["step"]).astype(np.float32)

        def paths():
            t0 = time.perf_counter()
            out = pl.paths(starts)
            return (time.perf_counter() - t0) * 1e3, out

        paths()
        pm = [paths() for _ in range(args.repeats)]
        r["paths"] = args.paths
        r["paths_ms"] = float(np.median([t for t, _ in pm]))
        r["paths_ms_all"] = [t for t, _ in pm]
        r["path_points"] = int(pl.last_off[-1])
        r["paths_arrived"] = int((pm[-1][1][2] == 0).sum())

        if not args.no_host and npts <= args.host_limit:
            try:
                import scipy  # noqa: F401
                cell3 = tuple(cell) + (0,) * (3 - dim)
                o = gpismap_amd.plan_opts(dim, np.float32(b["step"]))
                t, d = host_route(dist, shape, b["step"], cell3, o)
                r["host_ms"] = t
                cost = pl.get()[0].ravel().astype(np.float64)
                fin = np.isfinite(cost)
                r["host_reachable"] = int(np.isfinite(d).sum())
                r["host_max_rel_diff"] = float(np.max(np.abs(d[fin] - cost[fin]) / np.maximum(cost[fin], 1e-30))) if fin.any() else 0.0
            except ImportError:
                pass
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
