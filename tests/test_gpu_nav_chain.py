"""One navigation round on the device, stage by stage: tests/nav_chain.py's round with one set of fresh handles,
every call on one caller's stream.  After each stage the device's outputs are compared with that stage's reference function
evaluated on the device's own outputs of the stages before it -- run() hands the next stage what the hook of the stage before
returned -- and the conditions of tests/test_nav_chain.py are asserted again on the device's data.  The comparison rules are
those of the per-object tests, through their checkers: bits everywhere; the controller's q within 1 of the reference's and
everything after it from the device's own q (test_gpu_body.Checked); the filter's weights by test_gpu_pf.Checked's rule.  Times
and round counts are not compared."""
import ctypes as C
import time

import numpy as np
import pytest

import nav_chain as nc
import pplan_ref
import test_gpu_body as tbd
import test_gpu_cover as tcv
import test_gpu_locate as tlo
import test_gpu_obst as tob
import test_gpu_pf as tpf
import test_gpu_plan as tpl
import test_gpu_pplan as tpp
import test_gpu_render_field as trf
import test_gpu_timing as ttm
import test_gpu_track_field as ttf
import test_gpu_traj as ttj
import test_gpu_view as tvw
from test_gpu_track import _check_bits as _check_track
from test_nav_chain import conditions

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
U32 = np.uint32


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)) // max(1, a.dtype.itemsize)
    assert bad.size == 0, (what, "%d bytes differ, first elements %s" % (bad.size, np.unique(bad)[:6]))


class Device:
    """One set of fresh handles and the hooks that run each stage on them."""

    def __init__(self, dim, stream):
        import gpismap_amd as g
        self.g, self.L, self.dim = g, g.lib(), dim
        self.stream, self.sv = stream, C.c_void_p(stream)
        self.df, self.rf, self.cv, self.r, self.v = g.DistanceField(), g.DistanceField(), g.Coverage(), g.Renderer(), g.ViewScorer()
        self.pl, self.tj, self.pf, self.loc, self.t = g.Planner(), g.Trajectories(), g.ParticleFilter(), g.Locator(), g.Tracker()
        self.pp, self.pj = (g.PosePlanner(), g.Planner()) if dim == 2 else (None, None)
        self.fp = None
        self.walls = {}

    def hooks(self, names=None):
        names = nc.stages_of(self.dim) if names is None else names

        def timed(name):
            fn = getattr(self, name)

            def hook(r, out):
                t0 = time.perf_counter()
                got = fn(r, out)
                self.walls[name] = time.perf_counter() - t0
                conditions(dict(r, **{name: got}), name)
                return got
            return hook
        return {name: timed(name) for name in names}

    # 1
    def field(self, r, out):
        c = r["cfg"]
        self.keep = tpl._dev(c["f"].copy())
        self.df.from_grid(self.keep.data_ptr(), c["shape"], c["origin"], c["step"], 0.0, stream=self.stream)
        dist, site, var = self.df.get()
        assert var is None and tpl._bits_equal(dist.ravel(), out["dist"]) and np.array_equal(site.ravel(), out["site"])
        return dict(dist=dist.ravel(), site=site.ravel())

    # 2
    def frame(self, r, out):
        c = r["cfg"]
        if self.dim == 2:
            assert trf._call2(self.L, None, self.df, self.r, c["thetas"], c["pose"], off2=c["off2"], stream=self.sv) == 0
        else:
            assert trf._call3(self.L, None, self.df, self.r, c["pose"], cam6=c["cam"], stream=self.sv) == 0
        got = self.r.get()
        trf._check_bits(got, self.r, (out["depth"], out["rec"], out["status"], out["stats"]), "the round's frame, dim %d" % self.dim)
        return dict(out, depth=got[0], rec=got[1], status=got[2], meas=nc.measured(c, got[0], got[2]))

    # 3
    def cover(self, r, out):
        c, dist, meas = r["cfg"], r["field"]["dist"], r["frame"]["meas"]
        cv = self.cv
        assert cv.reset(self.df) is cv and cv.get().sum() == 0
        if self.dim == 2:
            cv.integrate_scan(c["thetas"], meas, c["pose"], c["off2"], stream=self.stream, **c["cover"])
        else:
            cv.integrate_depth(meas, c["pose"], c["cam"], stream=self.stream, **c["cover"])
        seen = cv.get().ravel()
        assert np.array_equal(seen, out["seen"].astype(np.uint8)), np.flatnonzero(seen != out["seen"])[:8]
        fr, ref = tcv._check_frontiers(cv, self.df, dist, seen != 0, stream=self.stream, **c["cover"])
        _bits(ref["rep_point"], out["reps"], "the representatives")
        assert cv.restrict(self.df, out=self.rf, stream=self.stream) is self.rf
        rd = self.rf.get()
        assert rd[2] is None and tpl._bits_equal(rd[0].ravel(), out["restricted"]) and np.array_equal(rd[1], self.df.get()[1])
        assert self.rf.info() == self.df.info()
        return dict(out, seen=seen != 0, frontiers=ref, reps=fr["rep"], restricted=rd[0].ravel())

    # 4
    def view(self, r, out):
        c = r["cfg"]
        sensor = (c["thetas"], c["off2"]) if self.dim == 2 else c["cam"]
        poses = nc.candidate_poses(c, r["cover"]["reps"])
        _bits(poses, out["poses"], "the candidate poses")
        g, h, p = tvw._check(self.df, r["field"]["dist"], r["cover"]["seen"], sensor, poses, cv=self.cv, v=self.v, stream=self.stream, **c["view"])
        assert np.array_equal(g, out["gain"]) and np.array_equal(h, out["hits"]) and tpl._bits_equal(p, out["predicted"])
        return dict(out, gain=self.v.gain(), hits=self.v.hits())

    # 5
    def plan(self, r, out):
        c, pl, pb = r["cfg"], self.pl, out["pb"]
        assert pl.solve(self.rf, r["cover"]["reps"], stream=self.stream, **c["plan"]) is pl
        cost, pol = pl.get()
        assert tpl._bits_equal(cost.ravel(), out["cost"]), np.flatnonzero(cost.ravel().view(U32) != out["cost"].view(U32))[:8]
        assert np.array_equal(pol.ravel(), out["policy"])
        inf, fin = pl.info(), np.isfinite(out["cost"])
        assert (inf["goals"], inf["goals_kept"], inf["free"], inf["reachable"]) == (pb.goals_given, pb.goals_kept, int(pb.free.sum()), int(fin.sum()))
        starts = nc.path_starts(c, r["cover"]["seen"], r["cover"]["reps"], r["cover"]["restricted"])
        _bits(starts, out["starts"], "the path starts")
        paths, scost, st = pl.paths(starts, stream=self.stream)
        pts = np.concatenate(paths) if pl.last_off[-1] else np.zeros((0, self.dim), F32)
        assert np.array_equal(st, out["status"]) and np.array_equal(pl.last_off, out["off"])
        assert np.array_equal(scost.view(U32), out["start_cost"].view(U32)) and tpl._bits_equal(pts, out["points"])
        return dict(out, cost=cost.ravel(), policy=pol.ravel(), off=pl.last_off.copy(), points=pts, start_cost=scost, status=st)

    def footprint(self, c):
        if self.fp is None:
            self.fp = tbd.device_body(c["body"])
        return self.fp

    # 6
    def pplan(self, r, out):
        c, pp = r["cfg"], self.pp
        fp = self.footprint(c)
        assert pp.solve(self.rf, fp, out["goals"], H=c["H"], stream=self.stream, **c["pplan"]) is pp
        tpp._check(pp, out["pb"], out["cost"])
        tpp._paths_equal(pp.paths(out["starts"], stream=self.stream), (out["off"], out["points"], out["heading"], out["start_cost"], out["status"]))
        assert np.array_equal(pp.last_off, out["off"])
        pj = out["projection"]
        assert pp.project(self.pj) is self.pj
        cost2, pol2 = self.pj.get()
        assert tpp._bits(cost2.ravel(), pj["cost2"]) and np.array_equal(pol2.ravel(), pj["policy2"])
        assert np.array_equal(pp.heading2.ravel(), pj["heading2"])
        i = self.pj.info()
        assert (i["free"], i["reachable"]) == (pj["free"], pj["reachable"]) and F32(i["max_cost"]) == pj["max_cost"]
        cost = pp.get()[0].ravel()
        return dict(out, cost=cost, projection=dict(pj, cost2=cost2.ravel(), policy2=pol2.ravel(), heading2=pp.heading2.ravel().copy()))

    # 7
    def traj(self, r, out):
        c, tj = r["cfg"], self.tj
        fp = self.footprint(c)
        assert self.pl.trajectories(nc.N, trajectories=tj) is tj
        g0 = tj.optimize(self.rf, stream=self.stream, iters=0).get()
        live = out["in_status"] == 0
        assert np.array_equal(g0["x"][live].view(U32), out["x0"][live].view(U32)) and np.isnan(g0["x"][~live]).all()
        self.pl.trajectories(nc.N, trajectories=tj)
        g = tj.optimize(self.rf, stream=self.stream, iters=5).get()
        ttj._equal(g, out["result"], "the round's trajectories, dim %d" % self.dim)
        got = tj.body_clearance(fp, self.rf, clearance=0.0)
        tbd._traj_equal(got, out["clearance"], "the body along the round's trajectories")
        return dict(out, result=g, clearance=got)

    # 8
    def timing(self, r, out):
        c, tj = r["cfg"], self.tj
        tm = tj.time(self.rf, stream=self.stream, **ttm._kw(nc.timing_opts(c)))
        ttm._equal(tm, out["timing"], ttm.TKEYS, "the round's timing")
        cd = ttm._cdict(tj.controls(c["dt"], nc.T))
        ttm._equal(cd, out["controls"], ttm.CKEYS, "the round's controls")
        self.ob = tob.device_set(out["obst"], c["step"])
        chk = tj.check(self.ob, c["dt"], 2 * nc.T, t0=0.0, t_begin=c["t_begin"])
        tob._check_equal(chk, out["check"], "the round's timed trajectories against the balls")
        return dict(out, timing=tm, controls=dict(out["controls"], **cd), check=chk)

    # 9
    def control(self, r, out):
        c, rd, S = r["cfg"], r["cover"]["restricted"], r["timing"]["obst"]
        cost = nc.terminal_cost(r)
        pose = nc.control_pose(c, r["timing"]["controls"])
        case = dict(dim=self.dim, K=nc.K, T=nc.T, seed=c["seed"], pose=pose, terminal="plan", opts=nc.mppi_opts(c), obst=S, body=c["body"], t_now=c["t_begin"])
        ck = tbd.Checked(case, stream=self.sv, env_=(c, self.rf, rd, self.pj if self.dim == 2 else self.pl, cost))
        ck.ob.close()
        ck.ob, ck.fp = self.ob, self.footprint(c)
        p0, h0 = ck.ctl.follow(self.tj, 0, c["dt"])
        tbd._same_bits(ck.ctl.get()["U"], out["U0"], "follow writes trajectory 0's controls")
        tbd._same_bits(nc.mppi_ref.pose_of_state(np.concatenate([p0, h0]), self.dim), out["pose"], "follow's pose")
        steps = []
        for k in range(2):
            if k:
                ck.shift()
            before = ck.ctl.get()["U"]
            t_now = c["t_begin"] + k * c["dt"]
            ck.step(t_now)
            g = ck.ctl.get()
            steps.append(nc.control_step(c, rd, cost, pose, before, k + 1, t_now, S, q=g["q"]))
            so = ck.ctl.obstacle_stats()
            assert so["dyn_hit_rollouts"] == steps[-1]["finish"]["ndyn"] and tbd._b(g["stats"]["neff"]) == tbd._b(steps[-1]["finish"]["neff"])
        # the first step hangs on the stages before alone: the stage's own reference, evaluated on them, has the device's bits
        tbd._same_bits(steps[0]["roll"]["J"], out["steps"][0]["roll"]["J"], "step 1 against the stage's reference")
        self.q_off = ck.q_off
        return dict(out, steps=steps)

    # 10
    def localise(self, r, out):
        c, dist, meas = r["cfg"], r["field"]["dist"], r["frame"]["meas"]
        dim, grid, ref = self.dim, out["grid"], out["filter"]
        ck = tpf.Checked(grid[:nc.PARTICLES], c["pf_seed"], dim, pf=self.pf)
        if dim == 2:
            fr = tpf.Frame(2, self.df, dist, thetas=c["thetas"], ranges=meas, off2=c["off2"])
        else:
            fr = tpf.Frame(3, self.df, dist, depth=meas, cam6=c["cam"], stride=c["pf"]["stride"])
        g = ck.predict(c["motion"], stream=self.sv)
        _bits(g["state"], ref["predicted"], "the predicted particles")
        est, g = ck.update(fr, stream=self.sv)
        _bits(g["cost"], ref["cost"], "the particles' costs")
        assert np.array_equal(g["inliers"], ref["inliers"]) and est["resampled"] == ref["resampled"]
        assert np.abs(g["q"].astype(np.int64) - ref["q"].astype(np.int64)).max() <= 1
        flt = dict(ref, state=g["state"], L=g["L"], q=g["q"], cost=g["cost"], inliers=g["inliers"], ancestors=g["ancestors"], neff=est["neff"],
                   estimate=est["pose"])
        if dim == 2:
            assert tlo._call2(self.L, None, self.df, self.loc, c["thetas"], meas, grid[:nc.POSES], off2=c["off2"], stream=self.sv, **c["locate"]) == 0
            rc, tp = ttf._call2(self.L, None, self.df, self.t, dict(thetas=c["thetas"], ranges=meas), grid[5], off2=c["off2"], stream=self.sv, **c["track"])
        else:
            assert tlo._call3(self.L, None, self.df, self.loc, meas, grid[:nc.POSES], cam6=c["cam"], stream=self.sv, **c["locate"]) == 0
            rc, tp = ttf._call3(self.L, None, self.df, self.t, meas, grid[5], cam6=c["cam"], stream=self.sv, **c["track"])
        assert rc == 0
        score = self.loc.get()
        tlo._check(score, out["score"], "the round's %d scored poses" % nc.POSES)
        res = self.t.result()
        _check_track((tp, res), out["track"], "the round's tracking call, dim %d" % dim)
        return dict(out, filter=flt, score=score, track=dict(out["track"], pose=tp, status=res["status"], inliers=res["inliers"]))


def _stream():
    import torch
    return torch.cuda.Stream(device=0)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_whole_round_stage_by_stage(dim):
    s = _stream()
    dev = Device(dim, s.cuda_stream)
    t0 = time.perf_counter()
    r = nc.run(dim, hooks=dev.hooks())
    wall = time.perf_counter() - t0
    assert set(dev.walls) == set(nc.stages_of(dim))
    print("dim %d round: %.2f s wall (references included), device and checks per stage: %s; q off by one at %d of %d rollout-steps"
          % (dim, wall, ", ".join("%s %.2f" % (k, dev.walls[k]) for k in nc.stages_of(dim)), dev.q_off, 2 * nc.K))
    assert r["cover"]["reps"].shape[0] >= 1


def test_the_projection_feeds_paths_trajectories_and_the_body_check():
    """Stage 6 of the 2-D round alone: PosePlanner.project into a Planner, then Planner.paths, Planner.trajectories and
    Trajectories.body_clearance from that projected handle, each against the references on the device's projection."""
    s = _stream()
    dev = Device(2, s.cuda_stream)
    names = ("field", "frame", "cover", "plan", "pplan")
    t0 = time.perf_counter()
    r = nc.run(2, stages=names, hooks=dev.hooks(names))
    c, pj, rd = r["cfg"], r["pplan"]["projection"], r["cover"]["restricted"]
    starts = r["plan"]["starts"]
    P, scost, st = dev.pj.paths(starts, stream=dev.stream)
    nx = c["shape"][0]
    ok, ijk = nc.plan_ref.snap(starts, c["shape"], c["origin"], c["step"])
    walked = 0
    for k in range(len(starts)):
        p = int(ijk[k, 1] * nx + ijk[k, 0])
        assert ok[k] and scost[k].view(U32) == pj["cost2"][p].view(U32)
        if np.isfinite(pj["cost2"][p]):
            w = np.array(pplan_ref.greedy_walk(pj, c["shape"], (p % nx, p // nx)), np.int64)
            assert st[k] == 0 and tpl._bits_equal(P[k], r["pplan"]["pb"].world(w)), k
            walked += 1
        else:
            assert st[k] in (2, 3) and len(P[k]) == 0, (k, st[k])
    assert walked >= 4 and (st != 0).any()
    # the trajectories of the projected paths: the resampling, five iterations and the body along them
    off = dev.pj.last_off.copy()
    pts = np.concatenate(P) if off[-1] else np.zeros((0, 2), F32)
    x0, ist = nc.traj_ref.resample(off, pts, st, nc.N)
    tj = dev.pj.trajectories(nc.N, trajectories=dev.tj)
    g = tj.optimize(dev.rf, stream=dev.stream, iters=5).get()
    ref = nc.traj_ref.optimize(rd, *nc.lat(c), x0, ist, nc.traj_opts(c))
    ttj._equal(g, ref, "trajectories of the projected paths")
    got = tj.body_clearance(dev.footprint(c), dev.rf, clearance=0.0)
    tbd._traj_equal(got, nc.body_ref.traj_clearance(rd, *nc.lat(c), c["body"], g["x"], g["status"], 0.0), "the body along them")
    assert (got["collides"] == 1).any()
    print("the 2-D projection and its consumers: %.2f s wall" % (time.perf_counter() - t0))
