"""Surface extraction benchmark (gpis3_extract_mesh) on the bench workload: synthetic 640x480 depth, F = 5 frames, identity pose,
the synthetic_grid box [-0.60,0.60]x[-0.45,0.45]x[0.85,1.15] as an n^3 lattice.  Per size it prints one JSON line with
  - extract_ms: wall time of the extraction call (median of --repeats; the call returns with its work finished),
  - lattice_test_ms / vertex_test_ms: test_device on the same lattice / on the returned vertices, device-resident, same process,
  - counts, and the bytes the extraction's own kernels move (from the shapes),
  - today_ms: the surface the way a user gets it without the call: lattice built and uploaded, test_device, f copied to the host,
    the numpy reference (tests/mesh_ref.py), test() on the vertices.
The time of the extraction's own kernels (the mesh_* kernels) comes from a separate profiler run:
  rocprofv3 --kernel-trace --stats -d DIR -o mesh -- python tools/mesh_bench.py --sizes 128 256 --repeats 3 --no-today
  python profiles/summarize_rocpd.py DIR/mesh_results.db
(profiles/mesh_kernel_stats.txt); mesh_kernel_bytes / that time against 8 TB/s is their share of the HBM peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 8.0


def box(n):
    return dict(origin=(-0.60, -0.45, 0.85), step=(1.2 / (n - 1), 0.9 / (n - 1), 0.3 / (n - 1)), shape=(n, n, n))


def kernel_bytes(n, nv, nf):
    """Bytes the extraction's own kernels move, from the shapes (3-D, lattice of n points, nv vertices, nf triangles)."""
    return {
        "mesh_lattice_kernel": 12 * n,                        # positions written
        "mesh_fcol_kernel": 32 * n + 4 * n,                   # record lines read (f is one of 8 slots), value written
        "mesh_classify_kernel": 4 * n + 9 * n,                # values (neighbours from cache), mask + two counts written
        "mesh_scan_partial_kernel": 2 * 4 * n,                # both scans: counts read ...
        "mesh_scan_apply_kernel": 2 * 8 * n,                  # ... read again and written
        "mesh_vertex_kernel": n + 8 * nv + 12 * nv,           # mask; base + values of the crossed edges; vertices written
        "mesh_prim_kernel": 4 * n + 12 * nf + 4 * 8 * nf,     # triangle bases; triangles written; corner values / masks / bases
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--no-today", action="store_true", help="skip the host-side path (profiler runs)")
    args = ap.parse_args()

    import torch
    import gpismap_amd
    import mesh_ref
    import replay

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    gm = gpismap_amd.GPisMap3()
    for f in range(args.frames):
        gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
    gm.sync()
    m = gpismap_amd.Mesh()
    L = gpismap_amd.lib()

    for n in args.sizes:
        b = box(n)
        npts = n ** 3

        def extract():
            t0 = time.perf_counter()
            m._extract(L.gpis3_extract_mesh, gm.h, 3, b["origin"], b["step"], b["shape"], None, "gpis3_extract_mesh")
            return (time.perf_counter() - t0) * 1e3

        extract()
        ext_ms = [extract() for _ in range(args.repeats)]
        nv, nf = m.counts()
        v, f, rec = m.get()

        # test_device on the same lattice and on the vertices, device-resident, same process
        lat = torch.from_numpy(mesh_ref.lattice(b["shape"], b["origin"], b["step"])).to(dev)
        res = torch.zeros((npts, 8), dtype=torch.float32, device=dev)
        vx = torch.from_numpy(v).to(dev)
        vres = torch.zeros((nv, 8), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def lattice_test():
            res.zero_()
            gm.test_device(lat.data_ptr(), npts, res.data_ptr(), 0)

        def vertex_test():
            vres.zero_()
            gm.test_device(vx.data_ptr(), nv, vres.data_ptr(), 0)

        lattice_test(); vertex_test()
        lt = [timed(lattice_test) for _ in range(args.repeats)]
        vt = [timed(vertex_test) for _ in range(args.repeats)]
        del lat, res, vx, vres
        torch.cuda.empty_cache()

        out = {"n": n, "lattice_points": npts, "vertices": nv, "triangles": nf, "repeats": args.repeats,
               "extract_ms": float(np.median(ext_ms)), "extract_ms_all": ext_ms,
               "lattice_test_ms": float(np.median(lt)), "vertex_test_ms": float(np.median(vt))}
        out["extract_over_tests"] = out["extract_ms"] / (out["lattice_test_ms"] + out["vertex_test_ms"])
        kb = kernel_bytes(npts, nv, nf)
        out["mesh_kernel_bytes"] = int(sum(kb.values()))
        out["mesh_kernel_ms_at_8TBs"] = out["mesh_kernel_bytes"] / (HBM_TBS * 1e12) * 1e3

        if not args.no_today:
            # today: host lattice uploaded, test_device, f to the host, numpy triangulation, test() on the vertices
            t = {}
            t0 = time.perf_counter()
            x = mesh_ref.lattice(b["shape"], b["origin"], b["step"])
            dx = torch.from_numpy(x).to(dev)
            dr = torch.zeros((npts, 8), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            t["upload"] = time.perf_counter() - t0
            t1 = time.perf_counter()
            gm.test_device(dx.data_ptr(), npts, dr.data_ptr(), 0)
            torch.cuda.synchronize()
            t["test_device"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            fcol = dr[:, 0].cpu().numpy()
            t["copy_f"] = time.perf_counter() - t1
            del dx, dr
            torch.cuda.empty_cache()
            t1 = time.perf_counter()
            hv, hf, _, _ = mesh_ref.extract(fcol, b["shape"], b["origin"], b["step"], -np.float32(0.2))
            t["numpy_triangulation"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            hrec = gm.test(hv)
            t["vertex_test"] = time.perf_counter() - t1
            t["total"] = time.perf_counter() - t0
            out["today_ms"] = {k: v * 1e3 for k, v in t.items()}
            out["today_same_mesh"] = bool(np.array_equal(hf, f) and np.array_equal(hv.view(np.uint32), v.view(np.uint32))
                                          and hrec is not None and np.array_equal(hrec.view(np.uint32), rec.view(np.uint32)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
