"""test() evaluates in full, in one pass with the two-candidate jobs (2F), the candidate among 2 and 3 of a three-candidate
fallback that a predictor expects the blend to read; the other gets its value column (2V) and the gradient columns of what the
blend reads beyond the prediction come last (2G).  A column has the same bits in every layout, so the pass-2 mode -- 0 no
prediction, 1 predicted, 2 / 3 always candidate 2 / 3, 4 the predictor inverted -- may change the time and nothing else: the
same bits and the same pass_jobs in every mode, against k5_ref.blend_ref on synthetic tables and against the CPU oracle (tiled)
on real maps.  The hit rate of the predictor is a condition on the heuristic alone."""
import numpy as np
import pytest

import k5_cases as Cs
import k5_ref as K

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
MODES = (0, 1, 2, 3, 4)
PLAN_MODE = {"F": 2, "V": 2, "G": 3}      # the mode in which the jobs per model of a pass are counted


# ---------------------------------------------------------------------------------------------------- query level ----
def _train(st, centres, sizes, spread, rng):
    """One model per centre (sizes[i] points with unit normals within spread[i] of it): the slots and the points."""
    from test_gpu_ongpis import soa9
    g = Cs.GEOM[3]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    own = np.repeat(np.arange(centres.shape[0]), sizes)
    n = int(off[-1])
    pos = (centres[own, :3].astype(np.float64) + rng.uniform(-1, 1, (n, 3)) * spread[own, None]).astype(F)
    nrm = rng.normal(0, 1, (n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    val = rng.uniform(-0.3, 0.3, n).astype(F) * F(g["scale"])
    sx = rng.uniform(1e-3, 5e-3, n).astype(F); sg = rng.uniform(0.01, 0.1, n).astype(F)
    return st.train(soa9(3, pos, nrm, val, sx, sg), off, np.arange(n, dtype=np.int32)), pos, off


def _plan(R, rec, thre, prior, mode):
    """The jobs a deterministic mode (0, 2, 3) gives every three-candidate fallback: dict of [njobs, 2] (query, candidate
    position) arrays for the passes "F" (predicted, in full), "V" (value only), "G" (gradient columns afterwards), and the
    number of predicted records the blend does not read."""
    pairs = []
    K.blend_ref(R["ncand"], R["cand"], rec, np.zeros((R["ncand"].size, 8), dtype=F), thre, prior, 3, pairs=pairs)
    value = {(int(q), int(s)) for q, s in pairs[2]}          # candidates 2 / 3 with a model of the three-candidate fallbacks
    read = {(int(q), int(s)) for q, s in pairs[3]}           # those the blend reads in full
    out = {"F": [], "V": [], "G": []}
    unread = 0
    for q in sorted({q for q, _ in value}):
        have = [s for s in (1, 2) if (q, s) in value]
        pick = None if mode == 0 else ((1 if mode == 2 else 2) if len(have) == 2 else have[0])
        for s in have:
            if s == pick:
                out["F"].append((q, s)); unread += (q, s) not in read
            else:
                out["V"].append((q, s))
                if (q, s) in read:
                    out["G"].append((q, s))
    return {k: np.array(v, dtype=np.int64).reshape(-1, 2) for k, v in out.items()}, unread, pairs


def test_modes_agree_on_synthetic_tables():
    """Islands A B C (k5_cases.islands_table), a query inside B, var_thre = -1: every query falls back and the blend reads two of
    its three records.  Always candidate 2 / 3 (modes 2 / 3) make the jobs of every pass a function of the reference alone, so
    the queries are chosen from a pool for them: per model, pass 2F gets 0, 1, 7, 8, 9 jobs (two-candidate and predicted ones
    alike) and pass 2V 31, 32, 33 in mode 2, pass 2G 9, 10, 11 in mode 3 (the nearer of A and C is the one read, so only there
    is the gradient pass busy), on models of N = 12, 90 and 300 points (three K4 size classes).  Islands whose A,
    whose C and whose A and C have no model; a query on a training point; a NaN query whose first candidate has no model (the
    gate opens on the prior and the predictor scores NaN).  Modes 0 to 4: the bits of blend_ref, its pass_jobs, and counters that
    add up; in modes 0, 2 and 3 the counters are the plan's."""
    import gpismap_amd
    from test_gpu_k5 import new_probe, new_store, reference, set_table, size_classes
    g = Cs.GEOM[3]
    rng = np.random.default_rng(4711)
    thre, prior = F(-1.0), g["prior"]
    tab, isl = Cs.islands_table()
    A, B, C = isl[:, 0], isl[:, 1], isl[:, 2]
    ncl = tab["c"].shape[0]
    sizes = rng.integers(3, 13, ncl)
    spread = np.full(ncl, 0.8 * float(g["cluster_half"]))
    big = (12, 90, 300)
    for k, i in enumerate((0, 1, 2, 4, 5, 6, 8, 9, 10, 19, 20, 21)):           # A and C of the islands whose jobs are counted
        for cell in (A[i], C[i]):
            if cell >= 0:
                sizes[cell] = big[k % 3]
                spread[cell] = 2.0 * g["scale"] if k % 3 else spread[cell]
    st = new_store(3)
    slots, pos, off = _train(st, tab["c"], sizes, spread, rng)
    tab["model"] = slots.astype(np.int32)
    tab["slotK"] = {int(m): 4 * int(n) for m, n in zip(slots, sizes)}
    tab["model"][A[11]] = -1
    tab["model"][C[12]] = -1
    for i in (13, 14):
        tab["model"][A[i]] = -1; tab["model"][C[i]] = -1
    # the NaN query: x undefined, y and z those of island 16: it sees the cells of islands 15 to 17 in traversal order
    xnan = tab["c"][B[16], :3].copy(); xnan[0] = np.nan
    Rn = K.lookup_ref(tab, xnan[None, :], g["half"])
    assert Rn["ncand"][0] == 3
    tab["model"][Rn["cell"][0, 0]] = -1
    assert (tab["model"][Rn["cell"][1:3, 0]] >= 0).all()
    bt = B[17] if tab["model"][B[17]] >= 0 else B[16]
    xtrain = pos[off[bt]]                                                        # a training point of B of island 17 (16)

    pool, own = Cs.island_queries(tab, isl, rng, 150)
    R, rec = reference(tab, pool, g["half"], st)
    assert np.all(R["count"] == np.where(own < 18, 3, 2)) and np.all(R["cell"][0] == B[own])
    plan = {p: _plan(R, rec, thre, prior, m)[0][p] for p, m in PLAN_MODE.items()}
    want = {"V": (range(0, 3), [31, 32, 33]), "F": (range(3, 8), [0, 1, 7, 8, 9]), "G": (range(8, 11), [9, 10, 11])}
    keep = []
    target = {}
    for i in range(27):
        mine = np.nonzero(own == i)[0]
        t = None
        for p, (islands, counts) in want.items():
            if i in islands:
                t = counts[i - islands[0]]
                jobs = plan[p]
                # the cell whose jobs are counted: A or C, the one that gets this kind of job more often
                reads = {c: np.isin(mine, jobs[R["cell"][jobs[:, 1], jobs[:, 0]] == c, 0]) for c in (A[i], C[i])}
                target[p, i] = max(reads, key=lambda c: reads[c].sum())
                yes = reads[target[p, i]]
                assert yes.sum() >= t, (p, i, yes.sum())
                keep.append(np.concatenate([mine[yes][:t], mine[~yes][:3]]))
        if t is None:
            keep.append(mine[:[0, 1, 7, 8, 9][i - 18]] if 18 <= i < 23 else mine[:8 if 11 <= i < 15 else 4])
    x = np.concatenate([pool[np.sort(np.concatenate(keep))], xnan[None, :], xtrain[None, :]]).astype(F)
    assert 200 < x.shape[0] < 1000
    R, rec = reference(tab, x, g["half"], st)
    plans = {m: _plan(R, rec, thre, prior, m) for m in (0, 2, 3)}
    pairs = plans[2][2]
    plan = {p: plans[m][0][p] for p, m in PLAN_MODE.items()}
    per = {p: np.bincount(R["cell"][j[:, 1], j[:, 0]], minlength=ncl) for p, j in plan.items()}
    per["F"] = per["F"] + np.bincount(R["cell"][pairs[1][:, 1], pairs[1][:, 0]], minlength=ncl)       # 2F carries the two-candidate jobs
    for p, (islands, counts) in want.items():
        got = [int(per[p][target[p, i]]) for i in islands]
        assert got == counts, (p, got, counts)
        assert len(size_classes(tab, R["cand"][plan[p][:, 1], plan[p][:, 0]])) >= 3, p
    assert [int(per["F"][A[i]]) for i in range(18, 23)] == [0, 1, 7, 8, 9]
    holes = Cs.hole_positions(R["ncand"], R["cand"])
    assert holes[(1,)] >= 1 and holes[(2,)] >= 1 and holes[(1,)] + holes[(2,)] >= 16 and holes[(1, 2)] >= 16 and holes[(0,)] >= 1, holes
    qn, qt = x.shape[0] - 2, x.shape[0] - 1
    assert R["cand"][0, qn] < 0 and (R["cand"][1:, qn] >= 0).all() and np.isnan(rec[qn, 1:, 4]).all()
    assert np.array_equal(x[qt], xtrain) and R["ncand"][qt] == 3

    prefill = np.full((x.shape[0], 8), 12345.0, dtype=F)
    exp, branch, jobs = K.blend_ref(R["ncand"], R["cand"], rec, prefill, thre, prior, 3)
    probe = new_probe(st, g["half"], thre, prior)
    set_table(probe, tab)
    seen = {}
    for mode in MODES + (1,):                       # (4 is followed by 1: a mode set on a live handle takes effect)
        probe.set_pass2_mode(mode)
        got = probe.run(x, prefill)
        d = probe.pass_detail(); d.pop("pick_ms")
        print("mode %d: jobs %s detail %s" % (mode, probe.pass_jobs(), d))
        diff = np.nonzero((got.view(U) != exp.view(U)).any(axis=1))[0]
        assert diff.size == 0, "mode %d: %d results differ, first %d (branch %s): %s against %s" % (
            mode, diff.size, diff[0], K.BRANCH_NAMES[int(branch[diff[0]])], got[diff[0]], exp[diff[0]])
        assert probe.pass_jobs() == jobs, (mode, probe.pass_jobs(), jobs)
        assert d["mode"] == mode
        assert d["predicted_full"] + d["value_only"] == jobs[2] and d["repair"] + d["predicted_full"] - d["unread"] == jobs[3], (d, jobs)
        assert d["hits"] <= d["predictions"] <= d["predicted_full"]
        if mode in plans:
            pl, unread, _ = plans[mode]
            assert [d["predicted_full"], d["value_only"], d["repair"], d["unread"]] == [pl["F"].shape[0], pl["V"].shape[0], pl["G"].shape[0], unread], (mode, d)
        if mode in seen:
            assert seen[mode] == d
        seen[mode] = d
    # the inverted predictor picks the other candidate wherever there is a choice
    assert seen[4]["predictions"] == seen[1]["predictions"] > 100 and seen[4]["predicted_full"] == seen[1]["predicted_full"]
    assert seen[1]["hits"] != seen[4]["hits"] and seen[0]["predicted_full"] == 0 and seen[3]["repair"] > 0
    L = gpismap_amd.lib()
    assert L.gpis_mapquery_set_pass2_mode(probe.h, 5) == -1 and L.gpis_mapquery_set_pass2_mode(probe.h, -1) == -1
    assert L.gpis_mapquery_set_pass2_mode(None, 1) == -1 and L.gpis_mapquery_pass_detail(probe.h, None) == -1
    probe.close(); st.close()


# ------------------------------------------------------------------------------------------------------ map level ----
def _bench_map():
    import gpismap_amd
    import oracle_lib
    import replay
    gm, om = gpismap_amd.GPisMap3(), oracle_lib.OracleMap3()
    for f in range(5):
        d = replay.synthetic_depth(f)
        gm.update(d, replay.IDENTITY_POSE); om.update(d, replay.IDENTITY_POSE)
    return gm, om, replay.synthetic_grid(32)


def _sequence3():
    import gpismap_amd
    import oracle_lib
    import replay
    frames = replay.load_bigbird()
    gm, om = gpismap_amd.GPisMap3(frames[0]["cam"]), oracle_lib.OracleMap3(frames[0]["cam"])
    for i, fr in enumerate(frames[:10]):
        if i:
            gm.set_camera(fr["cam"]); om.set_camera(fr["cam"])
        gm.update(fr["depth"], fr["pose"]); om.update(fr["depth"], fr["pose"])
    return gm, om, replay.demo3_grid()


def _sequence2():
    import gpismap_amd
    import oracle_lib
    import replay
    gm, om = gpismap_amd.GPisMap(), oracle_lib.OracleMap2()
    for fr in replay.load_gazebo():
        gm.update(fr["thetas"], fr["ranges"], fr["pose"]); om.update(fr["thetas"], fr["ranges"], fr["pose"])
    return gm, om, replay.demo2_grid()


@pytest.mark.parametrize("which", ["bench", "sequence3", "sequence2"])
def test_modes_on_real_maps_match_oracle(which):
    """One oracle pass per map; the modes in the order 0, 1, 2, 3, 4, 1 on one handle.  On the benchmark's map the predictor
    must be right for at least 0.90 of its predictions: the mean of the 8 to 32 nearest distances is right for 0.94 to 0.97 on
    the CPU oracle and always picking candidate 2 for 0.75 to 0.78, so the floor tells a broken score, not a sample."""
    gm, om, grid = {"bench": _bench_map, "sequence3": _sequence3, "sequence2": _sequence2}[which]()
    ro = om.test(grid)
    seen = {}
    jobs = None
    for mode in MODES + (1,):
        gm.set_pass2_mode(mode)
        rg = gm.test(grid)
        pj, d = gm.pass_jobs(), gm.pass_detail()
        d.pop("pick_ms")
        print("%s mode %d: %d queries, jobs %s, detail %s" % (which, mode, grid.shape[0], pj, d))
        assert np.array_equal(rg.view(U), ro.view(U)), (which, mode, int(np.sum(np.any(rg != ro, axis=1))))
        jobs = jobs or pj
        assert pj == jobs and pj["pass2a_value"] > 0 and pj["pass2b_grad"] > 0, (mode, pj, jobs)
        assert d["mode"] == mode
        assert d["predicted_full"] + d["value_only"] == pj["pass2a_value"], (mode, d, pj)
        assert d["repair"] + d["predicted_full"] - d["unread"] == pj["pass2b_grad"], (mode, d, pj)
        assert int(gm.stats()["last_test_evals"]) == pj["pass1"] + pj["pass2_full"] + pj["pass2a_value"]
        if mode in seen:
            assert seen[mode] == d                   # after the inverted predictor the default is back
        seen[mode] = d
    assert seen[0]["predicted_full"] == 0 and seen[1]["predicted_full"] > 0
    assert seen[4]["predictions"] == seen[1]["predictions"] and seen[4]["repair"] > seen[1]["repair"]
    if which == "bench":
        rate = seen[1]["hits"] / seen[1]["predictions"]
        print("bench map: hit rate %.4f of %d predictions (always candidate 2: %.4f, always 3: %.4f, inverted: %.4f)" % (
            rate, seen[1]["predictions"], seen[2]["hits"] / seen[2]["predictions"], seen[3]["hits"] / seen[3]["predictions"],
            seen[4]["hits"] / seen[4]["predictions"]))
        assert rate >= 0.90, rate
