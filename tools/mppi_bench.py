"""Sampling-controller benchmark (gpis_mppi_step) on tools/pf_bench.py's fields:
  - gazebo: the field (demo grid at 0.1 m) of the map of the first 14 scans, a planner solved towards the first recorded
    pose, the controller started at the 14th; K = --rollouts2 (4096), T = --horizon2 (64), the planner's cost-to-go at the end;
  - synthetic: the bench map's field at (256, 192, 64), from one corner region of the lattice towards a goal point in the
    opposite one; K = --rollouts3 (8192), T = --horizon3 (48), dt and the limits scaled to the 1.2 m lattice.
Per workload it prints one JSON line (and appends it to --out) with
  - step_ms: one step (four launches, one copy back) + one shift of a running controller, arguments built by the Python
    layer inside the clock (median of --repeats); step_info_ms: the library's own wall time of the step;
  - host_ms: the route it replaces, the numpy reference (tests/mppi_ref.py) on the same field, cost-to-go, pose and nominal
    sequence (median of --host-repeats);
  - filter_ms: one predict + update of a particle filter in the same process (2-D: 100 000 particles x the 14th scan; 3-D:
    10 000 particles x a rendered 640x480 frame at stride 8), for scale;
  - the step's statistics (N_eff, rollouts with a hit, the nominal rollout's cost).
Kernel times come from a separate profiler run (no timing there):
  rocprofv3 --kernel-trace --stats -d DIR -o mppi -- python tools/mppi_bench.py --repeats 3 --host-repeats 0 --out ''
  python profiles/summarize_rocpd.py DIR/mppi_results.db
(profiles/mppi_kernel_stats.txt)."""
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

from pf_bench import BOX2, OFF2, SYN, SYN_CAM  # noqa: E402
from track_bench import perturb3  # noqa: E402

F32 = np.float32
F64 = np.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3, help="0 = skip the numpy route and the filter")
    ap.add_argument("--rollouts2", type=int, default=4096)
    ap.add_argument("--horizon2", type=int, default=64)
    ap.add_argument("--rollouts3", type=int, default=8192)
    ap.add_argument("--horizon3", type=int, default=48)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppi_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
    import mppi_ref
    import replay

    out_f = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def record(name, dim, df, K, T, pose, goal, planner, opts, filter_step):
        ctl = gpismap_amd.Controller(**opts)
        ctl.init(dim, K, T, seed=1)
        for _ in range(3):                                # (warm-up; the nominal sequence leaves zero)
            df.control(ctl, pose, goal=goal, planner=planner)
            ctl.shift()
        ms, lib_ms = [], []
        for _ in range(args.repeats):
            def one():
                r = df.control(ctl, pose, goal=goal, planner=planner)
                ctl.shift()
                return r
            t, (u0, info) = timed(one)
            ms.append(t)
            lib_ms.append(ctl.info()["ms"])
        rec = {"workload": name, "repeats": args.repeats, "rollouts": K, "horizon": T, "dim": dim, "step_ms": float(np.median(ms)),
               "step_ms_all": ms, "step_info_ms": float(np.median(lib_ms)), "neff": info["neff"], "hits": info["hits"],
               "nominal_cost": info["nominal_cost"], "Jmin": info["Jmin"], "u0": [float(v) for v in u0]}
        if args.host_repeats > 0:
            i = df.info()
            shape, origin = i["shape"], i["origin"]
            dist = df.get()[0].ravel()
            cost = planner.get()[0].ravel() if planner is not None else None
            o = mppi_ref.default_opts(dim, i["step"])
            o.update(opts)
            U = ctl.get()["U"]
            tick = ctl.info()["tick"] + 1
            hms = [timed(lambda: mppi_ref.step(dist, shape, origin, i["step"], pose, U, 1, tick, K, o, cost, goal))[0]
                   for _ in range(args.host_repeats)]
            fms = [timed(filter_step)[0] for _ in range(args.host_repeats + 2)][2:]
            rec.update(host_ms=float(np.median(hms)), host_ms_all=hms, host_over_step=float(np.median(hms)) / rec["step_ms"],
                       filter_ms=float(np.median(fms)), filter_over_step=float(np.median(fms)) / rec["step_ms"])
        emit(rec)

    if "gazebo" in args.workloads:
        fr2 = replay.load_gazebo()
        g2 = gpismap_amd.GPisMap()
        for k in range(14):
            g2.update(fr2[k]["thetas"], fr2[k]["ranges"], fr2[k]["pose"])
        g2.sync()
        df = gpismap_amd.DistanceField()
        g2.distance_field(field=df, **BOX2)
        pl = df.plan(np.asarray(fr2[0]["pose"][:2], F32)[None], planner=gpismap_amd.Planner(), clearance=0.0)
        fr = fr2[14]
        pose = np.asarray(fr["pose"], F64)
        x, y, th = float(pose[0]), float(pose[1]), math.atan2(float(pose[3]), float(pose[2]))
        poses = np.ascontiguousarray(gpismap_amd.pose_grid2(x + np.linspace(-2.0, 2.0, 50), y + np.linspace(-2.0, 2.0, 50),
                                                            th + np.radians(np.linspace(-20.0, 20.0, 40))))
        pf = gpismap_amd.ParticleFilter()
        pf.init(poses, seed=1)
        tht, rg = np.ascontiguousarray(fr["thetas"], F32), np.ascontiguousarray(fr["ranges"], F32)

        def filter2():
            pf.predict((0.0, 0.0, 0.0))
            g2.pf_update_scan_field(df, pf, tht, rg)

        record("gazebo_planner_K%d_T%d" % (args.rollouts2, args.horizon2), 2, df, args.rollouts2, args.horizon2, pose, None, pl,
               dict(clearance=0.1), filter2)

    if "synthetic" in args.workloads:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df = gpismap_amd.DistanceField()
        gm.distance_field(field=df, **SYN)
        lo = np.array(SYN["origin"], F64)
        hi = lo + (np.array(SYN["shape"]) - 1) * SYN["step"]
        start = lo + 0.1 * (hi - lo)
        goal = lo + 0.9 * (hi - lo)
        pose = mppi_ref.pose_of_state(list(start) + [math.cos(0.5), math.sin(0.5)], 3)
        truth = perturb3(replay.IDENTITY_POSE, 0.015, 1.0, axis=(1.0, 2.0, -1.0), tdir=(0.6, -1.0, 0.5))
        depth = np.ascontiguousarray(gm.render_depth(truth, cam6=SYN_CAM)[0], F32)
        a = np.linspace(-0.05, 0.05, 10)
        off = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
        rv = [(0.0, 0.0, 0.0)] + [(0.02 * math.cos(t), 0.02 * math.sin(t), 0.01) for t in np.linspace(0, 2 * math.pi, 9, endpoint=False)]
        pf = gpismap_amd.ParticleFilter()
        pf.init(np.ascontiguousarray(gpismap_amd.pose_grid3(truth, off, rv)), seed=1)

        def filter3():
            pf.predict(((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
            gm.pf_update_depth_field(df, pf, depth, cam6=SYN_CAM, stride=8)

        record("synthetic_goal_K%d_T%d" % (args.rollouts3, args.horizon3), 3, df, args.rollouts3, args.horizon3, pose, goal, None,
               dict(dt=0.02, sigma=(0.25, 0.25, 0.25, 0.5), w_goal=20.0), filter3)
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
