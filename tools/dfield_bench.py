"""Distance-field benchmark (gpis3_distance_field / gpis2_distance_field).  Workloads: the synthetic F = 5 map on the bench box
[-0.60,0.60]x[-0.45,0.45]x[0.85,1.15] at the cubic steps of the shapes (256, 192, 64) and (512, 384, 128); bigbird (5 frames) on the
demo box at 2.5 mm; gazebo on the demo grid at 0.1 m.  Per workload it prints one JSON line with
  - call_ms: wall time of the call (median of --repeats; the call returns with its work finished),
  - lattice_test_ms: test_device on the same lattice, device-resident, same process, and call_over_lattice = their ratio,
  - sample_pts_per_s: gpis_dfield_sample on --samples random device-resident points in the box,
  - host_ms: the host route it replaces: test() on the lattice (host arrays), then scipy.ndimage.distance_transform_edt on
    the inside and outside masks (skipped without scipy or with --no-host).
The time of the field's own kernels (the df_* kernels) comes from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o dfield -- python tools/dfield_bench.py --repeats 3 --no-host
  python profiles/summarize_rocpd.py DIR/dfield_results.db
(profiles/dfield_kernel_stats.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LO, HI = (-0.60, -0.45, 0.85), (0.60, 0.45, 1.15)


def syn_box(shape):
    s = 0.3 / shape[2]
    return dict(origin=LO, step=s, shape=shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10 ** 7)
    ap.add_argument("--workloads", nargs="+", default=["syn256", "syn512", "bigbird", "gazebo"])
    ap.add_argument("--no-host", action="store_true", help="skip the host route (profiler runs)")
    args = ap.parse_args()

    import torch
    import gpismap_amd
    import mesh_ref
    import replay

    dev = torch.device("cuda", 0)
    torch.cuda.init()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    maps = {}

    def get_map(name):
        if name in maps:
            return maps[name]
        if name == "syn":
            gm = gpismap_amd.GPisMap3()
            for f in range(5):
                gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
            gm.sync()
        elif name == "bigbird":
            frames = replay.load_bigbird()
            gm = gpismap_amd.GPisMap3(frames[0]["cam"])
            for i in range(5):
                if i:
                    gm.set_camera(frames[i]["cam"])
                gm.update(frames[i]["depth"], frames[i]["pose"])
            gm.sync()
        else:
            gm = gpismap_amd.GPisMap()
            for fr in replay.load_gazebo():
                gm.update(fr["thetas"], fr["ranges"], fr["pose"])
            gm.sync()
        maps[name] = gm
        return gm

    df = gpismap_amd.DistanceField()
    for w in args.workloads:
        if w == "syn256":
            gm, b = get_map("syn"), syn_box((256, 192, 64))
        elif w == "syn512":
            gm, b = get_map("syn"), syn_box((512, 384, 128))
        elif w == "bigbird":
            gm, b = get_map("bigbird"), dict(origin=(-0.07, -0.10, 0.0), step=0.0025, shape=(81, 97, 113))
        else:
            gm, b = get_map("gazebo"), dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
        dim = len(b["shape"])
        npts = int(np.prod(b["shape"]))
        nrec = 2 * (1 + dim)

        def call():
            t0 = time.perf_counter()
            gm.distance_field(field=df, **b)
            return (time.perf_counter() - t0) * 1e3

        call()
        call_ms = [call() for _ in range(args.repeats)]
        dist, site, _ = df.get()

        lat = torch.from_numpy(mesh_ref.lattice(b["shape"], b["origin"], [b["step"]] * dim)).to(dev)
        res = torch.zeros((npts, nrec), dtype=torch.float32, device=dev)

        def lattice_test():
            res.zero_()
            gm.test_device(lat.data_ptr(), npts, res.data_ptr(), 0)

        lattice_test()
        lt = [timed(lattice_test) for _ in range(args.repeats)]
        del lat, res
        torch.cuda.empty_cache()

        lo = np.array(b["origin"], np.float64)
        hi = lo + (np.array(b["shape"]) - 1) * b["step"]
        rng = np.random.default_rng(0)
        xs = torch.from_numpy((lo + rng.random((args.samples, dim)) * (hi - lo)).astype(np.float32)).to(dev)
        out = torch.empty((args.samples, 1 + dim), dtype=torch.float32, device=dev)
        df.sample(xs.data_ptr(), m=args.samples, d_out=out.data_ptr())
        st = [timed(lambda: df.sample(xs.data_ptr(), m=args.samples, d_out=out.data_ptr())) for _ in range(args.repeats)]
        del xs, out
        torch.cuda.empty_cache()

        r = {"workload": w, "shape": list(b["shape"]), "step": b["step"], "lattice_points": npts, "repeats": args.repeats,
             "sites": int(np.count_nonzero(site.ravel() == np.arange(site.size))),
             "call_ms": float(np.median(call_ms)), "call_ms_all": call_ms, "lattice_test_ms": float(np.median(lt))}
        r["call_over_lattice"] = r["call_ms"] / r["lattice_test_ms"]
        r["call_minus_lattice_ms"] = r["call_ms"] - r["lattice_test_ms"]
        r["sample_ms"] = float(np.median(st))
        r["sample_pts_per_s"] = args.samples / (r["sample_ms"] * 1e-3)

        if not args.no_host:
            try:
                import scipy.ndimage as nd
            except ImportError:
                nd = None
            if nd is not None:
                t = {}
                t0 = time.perf_counter()
                x = mesh_ref.lattice(b["shape"], b["origin"], [b["step"]] * dim)
                rec = gm.test(x)
                t["test"] = time.perf_counter() - t0
                t1 = time.perf_counter()
                f = rec[:, 0].reshape(tuple(b["shape"])[::-1])
                ins = f < np.float32(-0.2)
                d_out = nd.distance_transform_edt(~ins)
                d_in = nd.distance_transform_edt(ins)
                _ = (d_out - d_in) * b["step"]
                t["scipy_edt"] = time.perf_counter() - t1
                t["total"] = time.perf_counter() - t0
                r["host_ms"] = {k: v * 1e3 for k, v in t.items()}
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
