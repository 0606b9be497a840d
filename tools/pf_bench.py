"""Particle-filter benchmark (gpis_pf_predict + gpis2_pf_update_scan / gpis3_pf_update_depth) on tools/locate_bench.py's inputs:
  - gazebo: scan 14 (270 beams) against the field (demo grid at 0.1 m) of the map of the scans before it, --particles2
    (100 000) particles from a grid around the recorded pose;
  - synthetic: the bench map and its field at (256, 192, 64), a 640x480 depth rendered 1.5 cm / 1 degree off the identity at
    stride 8, --particles3 (10 000) particles from a grid around it.
Per workload it prints one JSON line (and appends it to --out) with
  - step_ms: one predict + one update (with whatever resampling the update decides), arguments built before the clock starts
    (median of --repeats steps of one running filter; both calls return with their work done); predict_ms and update_ms apart;
    resampled: how many of the timed steps resampled;
  - host_ms: the route the filter replaces, in the same process on the same poses: score_scan / score_depth of the current
    poses (upload, kernel, copy back, ranking), a numpy weigh (exp, normalise, N_eff, mean) and a numpy systematic resampling
    with the motion applied; the resampled poses go up again with the next score call, so one step of that route is one such
    iteration (median of --repeats);
  - the filter's last estimate against the recorded / rendered pose.
Kernel times come from a separate profiler run (no timing there):
  rocprofv3 --kernel-trace --stats -d DIR -o pf -- python tools/pf_bench.py --repeats 3 --out ''
  python profiles/summarize_rocpd.py DIR/pf_results.db
(profiles/pf_kernel_stats.txt)."""
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

from track_bench import err2, err3, perturb3  # noqa: E402

F32 = np.float32
SYN = dict(origin=(-0.60, -0.45, 0.85), step=0.3 / 64, shape=(256, 192, 64))
BOX2 = dict(origin=(-4.9, -14.9), step=0.1, shape=(249, 199))
SYN_CAM = (568.0, 568.0, 310.0, 224.0, 640, 480)
OFF2 = (0.08, 0.0)


def host_step(score, poses, dim, beta, sigma_t, sigma_r, rng):
    """One step of the host route: score on the device, weigh and resample (systematic) in numpy, move the survivors."""
    cost = score(poses)[0]
    L = beta * cost
    w = np.exp(-(L - L.min()))
    w /= w.sum()
    neff = 1.0 / float(np.sum(w * w))
    m = poses.shape[0]
    a = np.searchsorted(np.cumsum(w), (np.arange(m) + rng.random()) / m).clip(0, m - 1)
    P = poses[a].astype(np.float64)
    P[:, :dim] += rng.standard_normal((m, dim)) * np.asarray(sigma_t[:dim])
    if dim == 2:
        th = np.arctan2(P[:, 3], P[:, 2]) + rng.standard_normal(m) * sigma_r
        P[:, 2], P[:, 3], P[:, 4], P[:, 5] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    return np.ascontiguousarray(P, F32), neff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--particles2", type=int, default=100000)
    ap.add_argument("--particles3", type=int, default=10000)
    ap.add_argument("--workloads", nargs="+", default=["gazebo", "synthetic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_bench.jsonl"), help="'' = print only")
    args = ap.parse_args()

    import gpismap_amd
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

    def record(name, dim, poses, predict, update, score, err):
        o = gpismap_amd.pf_opts(dim)
        pf = gpismap_amd.ParticleFilter()
        pf.init(poses, seed=1)
        predict(pf)
        update(pf)                                        # (warm-up: buffers grow on the first call)
        pms, ums, rs = [], [], 0
        for _ in range(args.repeats):
            pms.append(timed(lambda: predict(pf))[0])
            ms, est = timed(lambda: update(pf))
            ums.append(ms)
            rs += int(est["resampled"])
        info = pf.info()
        step = [a + b for a, b in zip(pms, ums)]
        rec = {"workload": name, "repeats": args.repeats, "particles": info["particles"], "points": info["points"],
               "samples": info["particles"] * info["points"], "step_ms": float(np.median(step)), "step_ms_all": step,
               "predict_ms": float(np.median(pms)), "update_ms": float(np.median(ums)), "update_info_ms": info["ms"],
               "resampled": rs, "neff": est["neff"], "error": list(err(est["pose"]))}
        rng = np.random.default_rng(1)
        cur = poses
        cur, _ = host_step(score, cur, dim, o.beta, list(o.sigma_t), o.sigma_r, rng)
        hms = []
        for _ in range(args.repeats):
            ms, (cur, hneff) = timed(lambda: host_step(score, cur, dim, o.beta, list(o.sigma_t), o.sigma_r, rng))
            hms.append(ms)
        rec.update(host_ms=float(np.median(hms)), host_ms_all=hms, host_neff=hneff, host_over_step=float(np.median(hms)) / rec["step_ms"])
        emit(rec)

    if "gazebo" in args.workloads:
        fr2 = replay.load_gazebo()
        g2 = gpismap_amd.GPisMap()
        for i in range(14):
            g2.update(fr2[i]["thetas"], fr2[i]["ranges"], fr2[i]["pose"])
        g2.sync()
        df = gpismap_amd.DistanceField()
        g2.distance_field(field=df, **BOX2)
        fr = fr2[14]
        x, y, th = float(fr["pose"][0]), float(fr["pose"][1]), math.atan2(float(fr["pose"][3]), float(fr["pose"][2]))
        na = 40
        nxy = int(math.ceil(math.sqrt(args.particles2 / na)))
        poses = np.ascontiguousarray(gpismap_amd.pose_grid2(x + np.linspace(-2.0, 2.0, nxy), y + np.linspace(-2.0, 2.0, nxy),
                                                            th + np.radians(np.linspace(-20.0, 20.0, na)))[:args.particles2])
        tht, rg = np.ascontiguousarray(fr["thetas"], F32), np.ascontiguousarray(fr["ranges"], F32)
        loc = gpismap_amd.Locator()
        record("gazebo_270_beams_x_%d_particles" % poses.shape[0], 2, poses, lambda pf: pf.predict((0.0, 0.0, 0.0)),
               lambda pf: g2.pf_update_scan_field(df, pf, tht, rg), lambda q: g2.score_scan_field(df, tht, rg, q, locator=loc, top_k=1),
               lambda p: err2(np.asarray(p, F32), fr["pose"]))

    if "synthetic" in args.workloads:
        gm = gpismap_amd.GPisMap3()
        for f in range(5):
            gm.update(replay.synthetic_depth(f), replay.IDENTITY_POSE)
        gm.sync()
        df = gpismap_amd.DistanceField()
        gm.distance_field(field=df, **SYN)
        truth = perturb3(replay.IDENTITY_POSE, 0.015, 1.0, axis=(1.0, 2.0, -1.0), tdir=(0.6, -1.0, 0.5))
        depth = np.ascontiguousarray(gm.render_depth(truth, cam6=SYN_CAM)[0], F32)
        nr = 10
        no = int(math.ceil((args.particles3 / nr) ** (1.0 / 3.0)))
        a = np.linspace(-0.05, 0.05, no)
        off = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
        rv = [(0.0, 0.0, 0.0)] + [(0.02 * math.cos(t), 0.02 * math.sin(t), 0.01) for t in np.linspace(0, 2 * math.pi, nr - 1, endpoint=False)]
        poses = np.ascontiguousarray(gpismap_amd.pose_grid3(truth, off, rv)[:args.particles3])
        loc = gpismap_amd.Locator()
        ident = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))

        record("synthetic_640x480_stride8_x_%d_particles" % poses.shape[0], 3, poses, lambda pf: pf.predict(ident),
               lambda pf: gm.pf_update_depth_field(df, pf, depth, cam6=SYN_CAM, stride=8),
               lambda q: gm.score_depth_field(df, depth, q, cam6=SYN_CAM, locator=loc, stride=8, top_k=1), lambda p: err3(p, truth))
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
