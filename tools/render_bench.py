"""Rendering benchmark (gpis3_render_depth / gpis2_render_scan).  Workloads:
  - synthetic: the bench map (synthetic 640x480 depth, F = 5 frames, identity pose) rendered at 640x480 from the identity pose;
  - bigbird: the bigbird map of all 40 frames rendered at 640x480 from each frame's pose and camera;
  - gazebo: the 2-D gazebo map, scans of 270 beams from every frame's pose.
Per workload it prints one JSON line with
  - call_ms: wall time of the render call (median of --repeats; the call returns with its work finished),
  - passes / march_passes / samples / evals (K4 evaluations) / hits of one call,
  - mq_ms: the host wall time inside its test() passes (MapQuery::run_prepared, each synchronised), and call_ms / mq_ms,
  - today_ms: the same image the way a user gets it without the call: the numpy reference (tests/render_ref.py) stepping the
    rays on the host and calling the map's test() once per pass, and whether it gives the same bits.
The time of the renderer's own kernels (the render_* kernels) comes from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o render -- python tools/render_bench.py --repeats 3 --no-today
  python profiles/summarize_rocpd.py DIR/render_results.db
(profiles/render_kernel_stats.txt)."""
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

LEVEL = -0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["synthetic", "bigbird", "gazebo"])
    ap.add_argument("--no-today", action="store_true", help="skip the host-side path (profiler runs)")
    args = ap.parse_args()

    import gpismap_amd
    import render_ref
    import replay

    F32 = np.float32
    U32 = np.uint32
    far3 = float(F32(0.9) * F32(np.float64(F32(0.025)) * 3.0))
    far2 = float(F32(0.9) * F32(np.float64(F32(1.2)) * 4.0))
    L = gpismap_amd.lib()

    def render3(gm, r, pose, cam6):
        """the C call alone: arguments built before the clock starts, the host copies taken after it stops"""
        p = np.ascontiguousarray(pose, F32)
        cam = gpismap_amd._cam(cam6)
        o = gpismap_amd.render_opts(3, level=LEVEL, far_step=far3)

        def fn():
            assert L.gpis3_render_depth(gm.h, r.h, C.byref(cam), p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(o), None) == 0
            return r
        return fn

    def run(name, calls, today):
        """calls: list of zero-argument functions, one C-level render each (timed alone), returning its renderer."""
        ms, per = [], []
        for c in calls:                         # (warm-up: buffers grow on the first call)
            c()
        for _ in range(args.repeats):
            t = 0.0
            per = []
            for c in calls:
                t0 = time.perf_counter()
                r = c()
                t += (time.perf_counter() - t0) * 1e3
                per.append((r.get(), r.info()))
            ms.append(t)
        info = [i for _, i in per]
        tot = {k: float(sum(i[k] for i in info)) for k in ("passes", "march_passes", "samples", "evals", "hits", "mq_ms", "rays")}
        res = {"workload": name, "renders": len(calls), "repeats": args.repeats, "call_ms": float(np.median(ms)),
               "call_ms_all": ms, **tot}
        res["call_ms_per_render"] = res["call_ms"] / len(calls)
        res["call_over_mq"] = float(ms[-1] / max(tot["mq_ms"], 1e-9))      # (mq_ms is that of the last repeat)
        res["passes_per_render"] = tot["passes"] / len(calls)
        res["samples_per_ray"] = tot["samples"] / max(tot["rays"], 1)
        res["evals_per_s"] = tot["evals"] / (ms[-1] * 1e-3)
        if today is not None and not args.no_today:
            t0 = time.perf_counter()
            same = True
            for (out, _), ref in zip(per, today()):
                same = same and np.array_equal(out[2], ref[2]) and np.array_equal(out[0].view(U32), ref[0].view(U32)) \
                    and np.array_equal(out[1].view(U32), ref[1].view(U32))
            res["today_ms"] = (time.perf_counter() - t0) * 1e3
            res["today_same_bits"] = bool(same)
        print(json.dumps(res), flush=True)

    if "synthetic" in args.workloads:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        r = gpismap_amd.Renderer()
        cam = (568.0, 568.0, 310.0, 224.0, 640, 480)
        call = render3(gm, r, replay.IDENTITY_POSE, cam)

        def today():
            lo, hi = r.box()
            return [render_ref.render_depth(lambda x, res: gm.test(x, res), cam, replay.IDENTITY_POSE, (lo, hi),
                                            render_ref.Opts(3, level=LEVEL, far_step=far3))]
        run("synthetic_640x480", [call], today)

    if "bigbird" in args.workloads:
        frames = replay.load_bigbird()
        gb = gpismap_amd.GPisMap3(frames[0]["cam"])
        for i, fr in enumerate(frames):
            if i:
                gb.set_camera(fr["cam"])
            gb.update(fr["depth"], fr["pose"])
        gb.sync()
        rs = [gpismap_amd.Renderer() for _ in frames]

        def mk(i):
            return render3(gb, rs[i], frames[i]["pose"], frames[i]["cam"])

        def today():
            out = []
            for i, fr in enumerate(frames):
                lo, hi = rs[i].box()
                out.append(render_ref.render_depth(lambda x, res: gb.test(x, res), fr["cam"], fr["pose"], (lo, hi),
                                                   render_ref.Opts(3, level=LEVEL, far_step=far3)))
            return out
        run("bigbird_640x480_%d_poses" % len(frames), [mk(i) for i in range(len(frames))], today)

    if "gazebo" in args.workloads:
        g2 = gpismap_amd.GPisMap()
        fr2 = replay.load_gazebo()
        for fr in fr2:
            g2.update(fr["thetas"], fr["ranges"], fr["pose"])
        g2.sync()
        r2 = [gpismap_amd.Renderer() for _ in fr2]

        def mk2(i):
            th = np.ascontiguousarray(fr2[i]["thetas"], F32)
            p6 = np.ascontiguousarray(fr2[i]["pose"], F32)
            o = gpismap_amd.render_opts(2, level=LEVEL, far_step=far2)
            P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

            def fn():
                assert L.gpis2_render_scan(g2.h, r2[i].h, P(th), th.size, P(p6), C.byref(o), None) == 0
                return r2[i]
            return fn

        def today2():
            out = []
            for i, fr in enumerate(fr2):
                lo, hi = r2[i].box()
                out.append(render_ref.render_scan(lambda x, res: g2.test(x, res), fr["thetas"], fr["pose"], (0.08, 0.0), (lo, hi),
                                                  render_ref.Opts(2, level=LEVEL, far_step=far2)))
            return out
        run("gazebo_%d_scans" % len(fr2), [mk2(i) for i in range(len(fr2))], today2)


if __name__ == "__main__":
    main()
