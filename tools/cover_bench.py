"""Coverage benchmark (gpis_cover_*).  Workloads: tools/dfield_bench.py's fields -- the synthetic F = 5 map on the bench box at the
cubic steps of the shapes (256, 192, 64) and (512, 384, 128), each with one 640 x 480 synthetic depth frame from the map's camera;
gazebo on the demo grid at 0.1 m with one of its own scans.  Default options (back_off one step, max_gap 2 degrees, clearance 3
steps, min_size 8).  Per workload it prints one JSON line with
  - field_ms: the field's own build in the same process (median of --repeats),
  - integrate_ms: wall time of one gpis3_cover_depth / gpis2_cover_scan into an empty mask (median; the reset is not timed),
    integrate_gbs = 2 B per lattice point / that time (the estimate of DESIGN.md 7m: one byte read, one written; the gathers
    of depth or sector table come on top), seen points,
  - frontiers_ms: wall time of one gpis_cover_frontiers (median), frontiers_over_field, frontier points, components, clusters,
    labelling rounds,
  - restrict_ms: one gpis_cover_restrict,
  - host_ms: the host route -- tests/cover_ref.py on the same input (integrate, frontiers), and whether its bytes equal the
    device's (skipped with --no-host and above --host-limit lattice points).
The kernel times come from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o cover -- python tools/cover_bench.py --repeats 3 --no-host
  python profiles/summarize_rocpd.py DIR/cover_results.db
(profiles/cover_kernel_stats.txt)."""
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
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
OFF2 = (0.08, 0.0)


def med(f, repeats, before=None):
    ts = []
    for k in range(repeats + 1):                          # (the first call warms up and is dropped)
        if before is not None:
            before()
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), ts[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["syn256", "syn512", "gazebo"])
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
        else:
            gm = gpismap_amd.GPisMap()
            for fr in replay.load_gazebo():
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
        gm.sync()
        maps[name] = gm
        return gm

    df = gpismap_amd.DistanceField()
    out = gpismap_amd.DistanceField()
    cv = gpismap_amd.Coverage()
    for w in args.workloads:
        if w == "syn256":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 64, shape=(256, 192, 64))
        elif w == "syn512":
            gm, b = get_map("syn"), dict(origin=LO, step=0.3 / 128, shape=(512, 384, 128))
        else:
            gm, b = get_map("gazebo"), dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
        shape, dim = b["shape"], len(b["shape"])
        npts = int(np.prod(shape))
        field_ms, _ = med(lambda: gm.distance_field(field=df, **b), args.repeats)
        step = df.info()["step"]
        if dim == 3:
            depth, pose = replay.synthetic_depth(2), replay.IDENTITY_POSE
            integrate = lambda: gm.cover_depth(cv, depth, pose)
        else:
            fr = replay.load_gazebo()[14]
            integrate = lambda: gm.cover_scan(cv, fr["thetas"], fr["ranges"], fr["pose"])
        integrate_ms, integrate_all = med(integrate, args.repeats, before=lambda: cv.reset(df))
        seen = cv.get().ravel()
        frontiers_ms, frontiers_all = med(lambda: cv.frontiers(df), args.repeats)
        fr_out = cv.frontiers(df, points=True)
        inf = cv.info()
        restrict_ms, _ = med(lambda: cv.restrict(df, out=out), args.repeats)
        r = {"workload": w, "shape": list(shape), "step": b["step"], "lattice_points": npts, "repeats": args.repeats,
             "field_ms": field_ms, "integrate_ms": integrate_ms, "integrate_ms_all": integrate_all,
             "integrate_gbs": 2.0 * npts / (integrate_ms * 1e-3) / 1e9, "seen": int(seen.sum()),
             "frontiers_ms": frontiers_ms, "frontiers_ms_all": frontiers_all, "frontiers_over_field": frontiers_ms / field_ms,
             "frontier_points": inf["points"], "components": inf["components"], "clusters": inf["clusters"], "rounds": inf["rounds"],
             "restrict_ms": restrict_ms}
        if not args.no_host and npts <= args.host_limit:
            import cover_ref
            dist = df.get()[0].ravel()
            o = gpismap_amd.cover_opts(dim, step)
            t0 = time.perf_counter()
            if dim == 3:
                ref = cover_ref.depth_mask(shape, b["origin"], step, depth, SYN_CAM, pose, o.back_off)
            else:
                ref = cover_ref.scan_mask(shape, b["origin"], step, fr["thetas"], fr["ranges"], fr["pose"], OFF2, o.back_off, o.max_gap)
            t1 = time.perf_counter()
            rf = cover_ref.frontiers(ref, dist, shape, b["origin"], step, o.clearance, o.min_size)
            t2 = time.perf_counter()
            r["host_ms"] = {"integrate": (t1 - t0) * 1e3, "frontiers": (t2 - t1) * 1e3}
            r["host_equal"] = bool(np.array_equal(seen, ref.astype(np.uint8)) and np.array_equal(fr_out["points"], rf["points"])
                                   and np.array_equal(fr_out["point_label"], rf["point_label"])
                                   and np.array_equal(fr_out["rep_index"], rf["rep"]))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
