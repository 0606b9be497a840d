"""Footprint benchmark (gpis_body_*), on tools/dfield_bench.py's fields and tools/mppi_bench.py's two controller configurations.
One JSON line per record, appended to --out.  It measures; no test asserts any of it.
  --part query  per field (syn256, gazebo) and m in --balls-body without 0: gpis_body_clearance of --states (10^6) host states,
                query_ms (median of --repeats, the host copies in and out included), query_info the samples per second it
                amounts to (states x m), next to sample_ms and samples per second of gpis_dfield_sample of the same number of
                points already on the device, in the same process; host_ms, tests/body_ref.py's clearance on the first
                --host-states states, scaled to all of them.
  --part step   per workload (gazebo: K = 4096, T = 64 with the planner; synthetic: K = 8192, T = 48 towards a goal point), m in
                --balls-body (0 = no footprint) and n in --balls (0 = no set): step_ms, one step + one shift through Python
                (median of --repeats), step_info_ms, the library's own wall time, and host_ms, tests/body_ref.py's step on the
                same input (--host-repeats, 0 = skip).
Every process that uses the GPU runs under its own time limit.  Kernel statistics come from a run of their own:
  rocprofv3 --kernel-trace --stats -d DIR -o body -- python tools/body_bench.py --part step --repeats 3 --host-repeats 0 --out ''
  python profiles/summarize_rocpd.py DIR/body_results.db"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dfield_bench import syn_box  # noqa: E402
from obst_bench import scatter  # noqa: E402
from pf_bench import BOX2, SYN  # noqa: E402

F32 = np.float32
F64 = np.float64


def body_table(dim, m, step):
    """m balls along the body's x axis over 12 lattice steps, every other one a step to the side (3-D: and up), radius one step."""
    b = np.zeros((m, dim), F64)
    b[:, 0] = (np.arange(m) - 0.5 * (m - 1)) * (12.0 * step / max(m, 2))
    b[1::2, 1] = step
    if dim == 3:
        b[::2, 2] = step
    return b, np.full(m, step, F64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("query", "step"), default="step")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--host-states", type=int, default=20000)
    ap.add_argument("--states", type=int, default=10 ** 6)
    ap.add_argument("--balls-body", type=int, nargs="+", default=[0, 1, 4, 16])
    ap.add_argument("--balls", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synthetic"])
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import math
    import gpismap_amd
    import body_ref
    import mppi_ref
    import obst_ref
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

    def gazebo_map(frames=None):
        fr2 = replay.load_gazebo()
        g2 = gpismap_amd.GPisMap()
        for k in range(len(fr2) if frames is None else frames):
            g2.update(fr2[k]["thetas"], fr2[k]["ranges"], fr2[k]["pose"])
        g2.sync()
        return g2, fr2

    def syn_map():
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        return gm

    def query_part():
        import torch
        dev = torch.device("cuda", 0)
        for w in ("syn256", "gazebo"):
            df = gpismap_amd.DistanceField()
            if w == "syn256":
                b = syn_box((256, 192, 64))
                syn_map().distance_field(field=df, **b)
            else:
                b = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
                gazebo_map()[0].distance_field(field=df, **b)
            dim = len(b["shape"])
            dist = df.get()[0].ravel()
            lo = np.array(b["origin"], F64)
            hi = lo + (np.array(b["shape"]) - 1) * b["step"]
            rng = np.random.default_rng(0)
            S = np.zeros((args.states, dim + 2), F64)
            S[:, :dim] = lo + rng.random((args.states, dim)) * (hi - lo)
            th = rng.uniform(-math.pi, math.pi, args.states)
            S[:, dim], S[:, dim + 1] = np.cos(th), np.sin(th)
            for m in [k for k in args.balls_body if k > 0]:
                off, rad = body_table(dim, m, b["step"])
                fp = gpismap_amd.Footprint(dim).set(off, rad)
                fp.clearance(df, S)
                ms = [timed(lambda: fp.clearance(df, S))[0] for _ in range(args.repeats)]
                got = fp.clearance(df, S)
                npts = args.states * m
                xs = torch.from_numpy((lo + rng.random((npts, dim)) * (hi - lo)).astype(F32)).to(dev)
                out = torch.empty((npts, 1 + dim), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                df.sample(xs.data_ptr(), m=npts, d_out=out.data_ptr())
                st = [timed(lambda: df.sample(xs.data_ptr(), m=npts, d_out=out.data_ptr()))[0] for _ in range(args.repeats)]
                del xs, out
                torch.cuda.empty_cache()
                rec = {"workload": w, "dim": dim, "states": args.states, "body_balls": m, "repeats": args.repeats,
                       "query_ms": float(np.median(ms)), "query_ms_all": ms, "query_samples_per_s": npts / (float(np.median(ms)) * 1e-3),
                       "sample_ms": float(np.median(st)), "sample_samples_per_s": npts / (float(np.median(st)) * 1e-3),
                       "below": got["below"], "off": got["off"]}
                if args.host_repeats > 0:
                    k = min(args.host_states, args.states)
                    B = body_ref.make(dim, off, rad)
                    t, ref = timed(lambda: body_ref.clearance(dist, b["shape"], b["origin"], b["step"], B, S[:k]))
                    same = np.array_equal(ref["ball"], got["ball"][:k]) and np.array_equal(ref["D"], got["D"][:k], equal_nan=True)
                    rec.update(host_states=k, host_ms=t * args.states / k, host_over_query=t * args.states / k / rec["query_ms"],
                               host_bits_equal=bool(same))
                emit(rec)

    def controller_inputs(name):
        """(dim, field, K, T, pose, goal, planner, opts) of tools/mppi_bench.py's configuration `name`."""
        df = gpismap_amd.DistanceField()
        if name == "gazebo":
            g2, fr2 = gazebo_map(14)
            g2.distance_field(field=df, **BOX2)
            pl = df.plan(np.asarray(fr2[0]["pose"][:2], F32)[None], planner=gpismap_amd.Planner(), clearance=0.0)
            return 2, df, 4096, 64, np.asarray(fr2[14]["pose"], F64), None, pl, dict(clearance=0.1)
        syn_map().distance_field(field=df, **SYN)
        lo = np.array(SYN["origin"], F64)
        hi = lo + (np.array(SYN["shape"]) - 1) * SYN["step"]
        pose = mppi_ref.pose_of_state(list(lo + 0.1 * (hi - lo)) + [math.cos(0.5), math.sin(0.5)], 3)
        return 3, df, 8192, 48, pose, lo + 0.9 * (hi - lo), None, dict(dt=0.02, sigma=(0.25, 0.25, 0.25, 0.5), w_goal=20.0)

    def step_part(name):
        dim, df, K, T, pose, goal, planner, opts = controller_inputs(name)
        i = df.info()
        lo = np.array(i["origin"][:dim], F64)
        hi = lo + (np.array(i["shape"][:dim]) - 1) * i["step"]
        for n in args.balls:
            for m in args.balls_body:
                ctl = gpismap_amd.Controller(**opts)
                ctl.init(dim, K, T, seed=1)
                ob, S, fp, B = None, None, None, None
                if n > 0:
                    c, v, r = scatter(dim, n, lo, hi, i["step"])
                    ob = gpismap_amd.Obstacles(dim, i["step"]).set(c, v, r, epoch=0.0)
                    S = obst_ref.make(dim, c, v, r, epoch=0.0, step=i["step"])
                if m > 0:
                    off, rad = body_table(dim, m, i["step"])
                    fp = gpismap_amd.Footprint(dim).set(off, rad)
                    B = body_ref.make(dim, off, rad)
                clock = [0.0]

                def one():
                    r_ = df.control(ctl, pose, goal=goal, planner=planner, obstacles=ob, t=clock[0], footprint=fp)
                    ctl.shift()
                    clock[0] += 0.1
                    return r_

                for _ in range(3):                        # (warm-up; the nominal sequence leaves zero)
                    one()
                ms, lib_ms = [], []
                for _ in range(args.repeats):
                    t, (u0, info) = timed(one)
                    ms.append(t)
                    lib_ms.append(ctl.info()["ms"])
                rec = {"workload": name, "dim": dim, "rollouts": K, "horizon": T, "body_balls": m, "balls": n, "repeats": args.repeats,
                       "step_ms": float(np.median(ms)), "step_ms_all": ms, "step_info_ms": float(np.median(lib_ms)), "neff": info["neff"],
                       "nominal_cost": info["nominal_cost"], "hits": info["hits"]}
                if args.host_repeats > 0:
                    dist = df.get()[0].ravel()
                    cost = planner.get()[0].ravel() if planner is not None else None
                    o = mppi_ref.default_opts(dim, i["step"])
                    o.update(opts)
                    U = ctl.get()["U"]
                    tick = ctl.info()["tick"] + 1
                    hms = [timed(lambda: body_ref.step(dist, i["shape"], i["origin"], i["step"], pose, U, 1, tick, K, o, cost, goal, obst=S,
                                                       t_now=clock[0], body=B))[0] for _ in range(args.host_repeats)]
                    rec.update(host_ms=float(np.median(hms)), host_over_step=float(np.median(hms)) / rec["step_ms"])
                emit(rec)

    if args.part == "query":
        query_part()
    else:
        for w in args.workloads:
            step_part(w)


if __name__ == "__main__":
    main()
