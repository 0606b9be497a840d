"""Field-rendering benchmark (gpis3_render_depth_field / gpis2_render_scan_field) on tools/render_bench.py's inputs:
  - synthetic: the bench map (synthetic 640x480 depth, F = 5 frames, identity pose) and its field on the lattice of
    tests/test_gpu_dfield.py's SYN (129x97x33 at 0.3/32 m), rendered at 640x480 from the identity pose;
  - bigbird: the bigbird map of all 40 frames and its field on the demo box at 2.5 mm, rendered at 640x480 from the pose and
    camera of every --every-th frame;
  - gazebo: the 2-D gazebo map and its field (demo grid at 0.1 m), scans of 270 beams from every frame's pose.
Per workload it prints one JSON line (and appends it to --out) with
  - field_ms: the map-level distance_field call that builds the field (median of --repeats),
  - call_ms / call_ms_per_render: the field render calls, default thread-to-pixel mapping (median of --repeats; each returns
    with its work done), call_ms_linear: the same with the other mapping (3-D), and whether both give the same bits,
  - samples / samples_per_ray / max_samples / hits / rays of the calls,
  - map_call_ms / map_hits / map_samples_per_ray: the map renderer (gpis3_render_depth / gpis2_render_scan) on the same poses
    in the same process (--map-repeats), and (field_ms + one render) / one map render: a frame against a new field,
  - views_per_field: --views renders from different poses against one field with the build shared out,
  - ref_ms: the numpy reference (tests/render_field_ref.py) on the first pose, and whether it gives the same bits.
The kernel's time comes from a separate profiler run (no timing there):
  rocprofv3 --kernel-trace --stats -d DIR -o render_field -- python tools/render_field_bench.py --repeats 3 --map-repeats 0 --no-ref --out ''
  python profiles/summarize_rocpd.py DIR/render_field_results.db
(profiles/render_field_kernel_stats.txt)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from track_bench import perturb2, perturb3  # noqa: E402

F32 = np.float32
U32 = np.uint32
LEVEL = -0.2
SYN = dict(origin=(-0.60, -0.45, 0.85), step=0.3 / 32, shape=(129, 97, 33))
BOX3 = dict(origin=(-0.07, -0.10, 0.0), step=0.0025, shape=(81, 97, 113))
BOX2 = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
OFF2 = (0.08, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--map-repeats", type=int, default=1, help="0 = skip the map renderer (profiler runs)")
    ap.add_argument("--views", type=int, default=10, help="renders against one field for the shared-cost record")
    ap.add_argument("--every", type=int, default=4, help="bigbird: every n-th frame's pose")
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy reference")
    ap.add_argument("--workloads", nargs="+", default=["synthetic", "bigbird", "gazebo"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_field_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
    import render_field_ref
    import replay

    L = gpismap_amd.lib()
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out_f = open(args.out, "w") if args.out else None
    far3 = float(F32(0.9) * F32(np.float64(F32(0.025)) * 3.0))
    far2 = float(F32(0.9) * F32(np.float64(F32(1.2)) * 4.0))

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

    def field3(df, r, pose, cam6):
        """the C call alone: arguments built before the clock starts, the host copies taken after it stops"""
        p, cam = np.ascontiguousarray(pose, F32), gpismap_amd._cam(cam6)
        o = gpismap_amd.render_field_opts(3, df.info()["step"])
        return lambda: L.gpis3_render_depth_field(None, df.h, r.h, C.byref(cam), P(p), C.byref(o), None)

    def map3(gm, r, pose, cam6):
        p, cam = np.ascontiguousarray(pose, F32), gpismap_amd._cam(cam6)
        o = gpismap_amd.render_opts(3, level=LEVEL, far_step=far3)
        return lambda: L.gpis3_render_depth(gm.h, r.h, C.byref(cam), P(p), C.byref(o), None)

    def field2(df, r, thetas, pose):
        th, p, off = np.ascontiguousarray(thetas, F32), np.ascontiguousarray(pose, F32), np.array(OFF2, F32)
        o = gpismap_amd.render_field_opts(2, df.info()["step"])
        return lambda: L.gpis2_render_scan_field(None, df.h, r.h, P(th), th.size, P(off), P(p), C.byref(o), None)

    def map2(g2, r, thetas, pose):
        th, p = np.ascontiguousarray(thetas, F32), np.ascontiguousarray(pose, F32)
        o = gpismap_amd.render_opts(2, level=LEVEL, far_step=far2)
        return lambda: L.gpis2_render_scan(g2.h, r.h, P(th), th.size, P(p), C.byref(o), None)

    def measure(calls, r, repeats):
        """median over the repeats of the summed wall time of the calls; the summed counters and the results of one repeat"""
        for c in calls:                                   # (warm-up: buffers grow on the first call)
            assert c() == 0
        ms, infos, outs = [], [], []
        for _ in range(repeats):
            tot, infos, outs = 0.0, [], []
            for c in calls:
                dt, rc = timed(c)
                assert rc == 0
                tot += dt
                infos.append(r.info())
                outs.append(r.get())
            ms.append(tot)
        return float(np.median(ms)), ms, infos, outs

    def same(a, b):
        return all(np.array_equal(x[0].view(U32), y[0].view(U32)) and np.array_equal(x[1].view(U32), y[1].view(U32))
                   and np.array_equal(x[2], y[2]) for x, y in zip(a, b))

    def run(name, dim, build, fcalls, mcalls, views, ref, r, rm):
        fms = [timed(build)[0] for _ in range(args.repeats)]
        r.set_field_tiles(True)
        cms, call_all, infos, outs = measure(fcalls, r, args.repeats)
        sm = lambda k: float(sum(i[k] for i in infos))
        n = len(fcalls)
        rec = {"workload": name, "renders": n, "repeats": args.repeats, "field_ms": float(np.median(fms)), "field_ms_all": fms,
               "call_ms": cms, "call_ms_all": call_all, "call_ms_per_render": cms / n, "rays": sm("rays"), "samples": sm("samples"),
               "hits": sm("hits"), "max_samples": max(i["max_samples"] for i in infos)}
        rec["samples_per_ray"] = rec["samples"] / rec["rays"]
        rec["samples_per_s"] = rec["samples"] / (cms * 1e-3)
        if dim == 3:
            r.set_field_tiles(False)
            lms, lin_all, _, louts = measure(fcalls, r, args.repeats)
            r.set_field_tiles(True)
            rec.update(call_ms_linear=lms, call_ms_linear_all=lin_all, linear_same_bits=same(outs, louts))
        if args.map_repeats > 0:
            mms, _, minfos, mouts = measure(mcalls, rm, args.map_repeats)
            rec.update(map_call_ms=mms, map_call_ms_per_render=mms / n, map_hits=float(sum(i["hits"] for i in minfos)),
                       map_samples_per_ray=float(sum(i["samples"] for i in minfos)) / rec["rays"],
                       map_over_field=mms / cms, new_field_frame_over_map_render=(rec["field_ms"] + cms / n) / (mms / n))
        bms = timed(build)[0]
        for c in views:
            assert c() == 0
        tot = sum(timed(c)[0] for c in views)
        rec["views_per_field"] = {"views": len(views), "field_ms": bms, "calls_ms": tot,
                                  "ms_per_view_shared": (bms + tot) / len(views)}
        if not args.no_ref:
            dt, o = timed(ref)
            rec.update(ref_ms=dt, ref_same_bits=same([outs[0]], [o[:3]]))
        emit(rec)

    if "synthetic" in args.workloads:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df = gpismap_amd.DistanceField()
        gm.distance_field(field=df, **SYN)
        r, rm = gpismap_amd.Renderer(), gpismap_amd.Renderer()
        poses = [perturb3(replay.IDENTITY_POSE, 0.02, 2.0, axis=(np.cos(a), np.sin(a), 0.5), tdir=(np.sin(a), 0.7, np.cos(a)))
                 for a in np.linspace(0, 2 * np.pi, args.views, endpoint=False)]

        def ref():
            i = df.info()
            return render_field_ref.render_depth(df.get()[0].ravel(), i["shape"], i["origin"], i["step"], SYN_CAM, replay.IDENTITY_POSE)
        run("synthetic_640x480", 3, lambda: gm.distance_field(field=df, **SYN), [field3(df, r, replay.IDENTITY_POSE, SYN_CAM)],
            [map3(gm, rm, replay.IDENTITY_POSE, SYN_CAM)], [field3(df, r, p, SYN_CAM) for p in poses], ref, r, rm)

    if "bigbird" in args.workloads:
        frames = replay.load_bigbird()
        gb = gpismap_amd.GPisMap3(frames[0]["cam"])
        for fr in frames:
            gb.set_camera(fr["cam"])
            gb.update(fr["depth"], fr["pose"])
        gb.sync()
        df = gpismap_amd.DistanceField()
        gb.distance_field(field=df, **BOX3)
        r, rm = gpismap_amd.Renderer(), gpismap_amd.Renderer()
        ids = list(range(0, len(frames), args.every))

        def ref():
            i = df.info()
            return render_field_ref.render_depth(df.get()[0].ravel(), i["shape"], i["origin"], i["step"], frames[ids[0]]["cam"],
                                                 frames[ids[0]]["pose"])
        run("bigbird_640x480_%d_poses" % len(ids), 3, lambda: gb.distance_field(field=df, **BOX3),
            [field3(df, r, frames[i]["pose"], frames[i]["cam"]) for i in ids],
            [map3(gb, rm, frames[i]["pose"], frames[i]["cam"]) for i in ids],
            [field3(df, r, frames[i]["pose"], frames[i]["cam"]) for i in range(args.views)], ref, r, rm)

    if "gazebo" in args.workloads:
        fr2 = replay.load_gazebo()
        g2 = gpismap_amd.GPisMap()
        for fr in fr2:
            g2.update(fr["thetas"], fr["ranges"], fr["pose"])
        g2.sync()
        df = gpismap_amd.DistanceField()
        g2.distance_field(field=df, **BOX2)
        r, rm = gpismap_amd.Renderer(), gpismap_amd.Renderer()

        def ref():
            i = df.info()
            return render_field_ref.render_scan(df.get()[0].ravel(), i["shape"], i["origin"], i["step"], fr2[0]["thetas"],
                                                fr2[0]["pose"], OFF2)
        run("gazebo_%d_scans" % len(fr2), 2, lambda: g2.distance_field(field=df, **BOX2),
            [field2(df, r, fr["thetas"], fr["pose"]) for fr in fr2], [map2(g2, rm, fr["thetas"], fr["pose"]) for fr in fr2],
            [field2(df, r, fr2[i]["thetas"], perturb2(fr2[i]["pose"], 0.1, 2.0)) for i in range(args.views)], ref, r, rm)
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
