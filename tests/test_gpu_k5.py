"""K5 (the driver of test(): cluster lookup, std::sort tie emulation, job lists, binning into K4 tiles, decide, blend) on
synthetic cluster tables against a plain reference, bit for bit.

Expected result of every case: k5_ref.blend_ref(k5_ref.lookup_ref(table, x), rec), rec = OnGPIS.eval(layout 0) on the same
store for every (query, candidate) pair.  Compared per case and per pre-fill (zeros, 12345): the candidates, the jobs of each
pass and every float of the result as uint32.  test_k5_ref.py holds the reference to the CPU oracle and asserts the
generators' populations without a GPU; each case here asserts the populations it is about again on its own inputs."""
import numpy as np
import pytest

import k5_cases as Cs
import k5_ref as K

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


def new_store(dim):
    import gpismap_amd
    return gpismap_amd.OnGPIS(dim, Cs.GEOM[dim]["scale"])


def new_probe(st, half, thre, prior):
    import gpismap_amd
    return gpismap_amd.MapQueryProbe(st, half, thre, prior)


def train(st, dim, centres, rng, sizes=None, spread=None):
    """One model per centre: sizes[i] points (3..12 by default) with unit normals around it.  Returns the slots."""
    from test_gpu_ongpis import soa9
    g = Cs.GEOM[dim]
    m = centres.shape[0]
    sizes = rng.integers(3, 13, m) if sizes is None else np.asarray(sizes)
    spread = np.full(m, 0.8 * float(g["cluster_half"])) if spread is None else np.asarray(spread, dtype=np.float64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    own = np.repeat(np.arange(m), sizes)
    n = int(off[-1])
    pos = (centres[own, :dim].astype(np.float64) + rng.uniform(-1, 1, (n, dim)) * spread[own, None]).astype(F)
    nrm = rng.normal(0, 1, (n, dim)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    val = rng.uniform(-0.3, 0.3, n).astype(F) * F(g["scale"])
    sx = rng.uniform(1e-3, 5e-3, n).astype(F); sg = rng.uniform(0.01, 0.1, n).astype(F)
    return st.train(soa9(dim, pos, nrm, val, sx, sg), off, np.arange(n, dtype=np.int32))


def give_models(st, tab, rng, big=True, pick=None):
    """A small model per cell, and models at K ~ 20, 140 and 300 (three K4 size classes in one pass, the side-stream fork) on
    the cells `pick` (six random ones by default).  tab["slotK"]: K of every slot."""
    dim = tab["dim"]
    ncl = tab["c"].shape[0]
    sizes = rng.integers(3, 13, ncl)
    spread = np.full(ncl, 0.8 * float(Cs.GEOM[dim]["cluster_half"]))
    if big and ncl >= 12:
        pick = rng.choice(ncl, 6, replace=False) if pick is None else pick
        per = (5, 35, 75) if dim == 3 else (7, 47, 100)           # K = N (1 + dim)
        for i, c in enumerate(pick):
            sizes[c] = per[i % 3]
            spread[c] = 2.0 * Cs.GEOM[dim]["scale"] if i % 3 else spread[c]
    tab["model"] = train(st, dim, tab["c"], rng, sizes, spread).astype(np.int32)
    tab.setdefault("slotK", {}).update({int(m): int(k) * (1 + dim) for m, k in zip(tab["model"], sizes)})
    return tab


def size_classes(tab, models):
    """K4 size classes (ongpis_class_of_nbx of ceil(K / 32)) of the given model slots."""
    nbx = {-(-tab["slotK"][int(m)] // 32) for m in np.unique(models) if m >= 0}
    return {0 if b <= 4 else 1 if b <= 8 else 2 if b <= 9 else 3 if b <= 16 else 4 if b <= 32 else 5 if b <= 48 else 6 for b in nbx}


def records(st, x, R):
    """[n, 3, 8]: the record of every (query, candidate) pair that has a model, through K4's full layout."""
    n = x.shape[0]
    rec = np.zeros((n, 3, 8), dtype=F)
    k, q = np.nonzero(R["cand"] >= 0)
    if q.size:
        rec[q, k] = st.eval(x, q, R["cand"][k, q], layout=0)
    return rec


def set_table(probe, tab):
    probe.set_table(tab["c"], tab["lo"], tab["hi"], tab["model"], tab["parent"], tab["anc_lo"], tab["anc_hi"], tab["anc_parent"],
                    tab["pitch"])


def reference(tab, x, half, st, stable_above=128):
    """lookup_ref; above 128 candidates the kernels do not emulate std::sort: the pinned result there
    is the (distance, traversal rank) order."""
    R = K.lookup_ref(tab, x, half)
    over = R["count"] > stable_above
    if over.any():
        S = K.lookup_ref(tab, x, half, stable_sort=True)
        for key in ("cand", "cell"):
            R[key][:, over] = S[key][:, over]
    return R, records(st, x, R)


def check(name, probe, x, R, rec, thre, prior, dim, prefills=(0.0, 12345.0)):
    n = x.shape[0]
    out = None
    for pf in prefills:
        prefill = np.full((n, 2 * (1 + dim)), pf, dtype=F)
        exp, branch, jobs = K.blend_ref(R["ncand"], R["cand"], rec, prefill, thre, prior, dim)
        got = probe.run(x, prefill)
        nc, cd = probe.candidates()
        bad = np.nonzero((nc != R["ncand"]) | (cd != R["cand"]).any(axis=0))[0]
        assert bad.size == 0, "%s: %d queries with other candidates, first %d: %s / %s against %s / %s (count %d)" % (
            name, bad.size, bad[0], nc[bad[0]], cd[:, bad[0]], R["ncand"][bad[0]], R["cand"][:, bad[0]], R["count"][bad[0]])
        assert probe.pass_jobs() == jobs, (name, probe.pass_jobs(), jobs)
        diff = np.nonzero((got.view(U) != exp.view(U)).any(axis=1))[0]
        assert diff.size == 0, "%s (pre-fill %g): %d results differ, first %d (branch %s): %s against %s" % (
            name, pf, diff.size, diff[0], K.BRANCH_NAMES[int(branch[diff[0]])], got[diff[0]], exp[diff[0]])
        out = (exp, branch, jobs)
    exp, branch, jobs = out
    h = K.branch_histogram(branch)
    print("\n%s: %d queries, candidates %s (max %d), ties %d (std::sort differs %d), jobs %s, branches %s" % (
        name, n, np.bincount(np.minimum(R["count"], 4), minlength=5), R["count"].max() if n else 0, R["tie"].sum(), R["unstable"].sum(), jobs,
        {k: v for k, v in h.items() if v}))
    return exp, branch, jobs, h


LOOKUP = [(3, "sparse"), (3, "dense"), (2, "sparse"), (2, "dense")]


@pytest.mark.parametrize("dim,kind", LOOKUP, ids=["%dd_%s" % c for c in LOOKUP])
def test_lookup(dim, kind):
    """Random, lattice-aligned, face +- 1 ulp, outside (more than / exactly / just under the search half, far) queries and the
    crafted ancestor one ulp short of its child."""
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(100 + dim)
    tab = Cs.table(dim, kind)
    x, cell = Cs.lookup_queries(tab, 7)
    st = new_store(dim)
    give_models(st, tab, rng)
    probe = new_probe(st, g["half"], g["var_thre"], g["prior"])
    set_table(probe, tab)
    R, rec = reference(tab, x, g["half"], st)
    assert R["tie"].sum() > 300 and R["unstable"].sum() > 100 and (R["pruned"] > 0).sum() > 50 and (R["count"] == 0).sum() > 10
    assert R["pruned"][-1] >= 1 and cell not in R["cell"][:, -1]
    assert len(size_classes(tab, R["cand"][0])) >= 3                    # pass 1 launches three size classes: the fork is taken
    exp, branch, jobs, h = check("lookup %d-D %s" % (dim, kind), probe, x, R, rec, g["var_thre"], g["prior"], dim)
    assert jobs[0] > 2000 and jobs[2] > 0
    probe.close(); st.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_tie_kernel_strides_its_list(dim):
    """More tie queries than one grid stride of lookup_tie_kernel (512 workgroups x 32 lanes) on the dense table."""
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(200 + dim)
    tab = Cs.table(dim, "dense")
    x = K.queries_aligned(tab, rng, 30000)
    st = new_store(dim)
    give_models(st, tab, rng, big=False)
    probe = new_probe(st, g["half"], g["var_thre"], g["prior"])
    set_table(probe, tab)
    R, rec = reference(tab, x, g["half"], st)
    listed = R["tie"] & (R["count"] > 1) & (R["count"] <= 128)
    assert listed.sum() > 512 * 32, listed.sum()
    assert R["unstable"].sum() > 5000 and R["count"].max() == (125 if dim == 3 else 64)
    check("tie %d-D" % dim, probe, x, R, rec, g["var_thre"], g["prior"], dim, prefills=(12345.0,))
    probe.close(); st.close()


def test_tie_kernel_at_its_128_candidate_guard():
    """Candidate counts of 127, 128 and 129 with ties (a wider search box over three L-shaped blocks of 121 + 6 / 7 / 8 cells).
    Up to 128 the order is std::sort's; above, the kernels do not emulate it and return the (distance, traversal) order."""
    dim = 2
    g = Cs.GEOM[dim]
    half = Cs.TIE_GUARD_HALF
    rng = np.random.default_rng(300)
    tab, x = Cs.tie_guard_case()
    st = new_store(dim)
    give_models(st, tab, rng, big=False)
    probe = new_probe(st, half, g["var_thre"], g["prior"])
    set_table(probe, tab)
    R, rec = reference(tab, x, half, st)
    for want in (127, 128, 129):
        m = R["count"] == want
        assert (m & R["tie"]).sum() >= 1, (want, np.unique(R["count"]))
    assert (R["unstable"] & (R["count"] <= 128) & (R["count"] >= 127)).sum() >= 1
    plain = K.lookup_ref(tab, x, half)
    assert (plain["cell"] != R["cell"])[:, R["count"] == 129].any(), "std::sort and the pinned order agree at 129: nothing pinned"
    check("tie guard", probe, x, R, rec, g["var_thre"], g["prior"], dim)
    probe.close(); st.close()


@pytest.mark.parametrize("slots,n", Cs.BINNING, ids=["m%d_n%d" % b for b in Cs.BINNING])
def test_binning(slots, n):
    """num_slots at the scan's 1024-thread edge and at the LDS / global-atomic switch (8192 / 8193), every slot a trained model;
    n and 2n at the 4096-job block seam; per model 0, 1, 7, 8, 9 ... 200 pass-1 jobs (tq = 8; the tile edges of the other
    passes: test_tile_edges_of_every_pass); waves of one model, of 64 distinct models, and with a jobless lane 0; the K ~ 20 /
    140 / 300 models among the cells that get jobs."""
    dim = 3
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(400 + slots)
    tab = Cs.n_cell_table(dim, slots)
    assert tab["c"].shape[0] == slots
    x, cells, counted = Cs.binning_queries(tab, n, rng)
    st = new_store(dim)
    give_models(st, tab, rng, big=slots >= 1023, pick=counted + np.arange(6))
    assert np.unique(tab["model"]).size == slots and tab["model"].max() == slots - 1         # num_slots == slots, all trained
    far = np.nonzero(cells < 0)[0]
    assert x.shape[0] == n and np.array_equal(far, np.arange(Cs.NFAR) * 64)
    R0 = K.lookup_ref(tab, x, g["half"])
    rec0 = records(st, x, R0)
    has0 = (R0["ncand"] >= 1)
    thre = F(np.median(rec0[has0, 0, 4]))
    probe = new_probe(st, g["half"], thre, g["prior"])
    set_table(probe, tab)
    R, rec = reference(tab, x, g["half"], st)
    jm = np.where(has0, R["cand"][0], -1)
    w = Cs.wave_populations(jm)
    per_model = np.bincount(jm[jm >= 0], minlength=slots)
    assert w["lane0"] >= 4 and w["one"] >= 1 and w["one_lane0"] >= 1 and (w["distinct"] >= 4 or slots == 1), w
    near = cells >= 0
    assert np.all(R["ncand"][far] == 0) and np.all(R["cand"][0][near] == tab["model"][cells[near]])
    if slots > 1:
        assert counted >= 11 and len(size_classes(tab, jm)) >= 3
        for c in Cs.CYCLE:
            assert (per_model[tab["model"][:counted]] == c).sum() >= counted // 11, (c, np.bincount(per_model)[:40])
    exp, branch, jobs, h = check("binning %d models" % slots, probe, x, R, rec, thre, g["prior"], dim)
    print("   pass-1 jobs per model: histogram %s; waves %s" % (np.bincount(per_model)[:40], w))
    assert jobs[0] == int(has0.sum()) and (slots == 1 or (jobs[2] > 0 and jobs[3] > 0))
    probe.close(); st.close()


def test_tile_edges_of_every_pass():
    """Jobs per model at 0, 1, tq - 1, tq, tq + 1 in the pass of each tile size: pass 2 (tq = 8, two-candidate queries), pass 2a
    (tq = 32, value column) and pass 2b (tq = 10, gradient columns).  Islands of three (two) cells A B C: a query inside B has
    exactly these candidates, B first.  var_thre = -1 opens the gate for every query and never picks, so pass 2 / 2a evaluate A
    and C of every query and pass 2b those of the two smallest variances; the queries are chosen from a pool, by the records
    the store returns, so that A of an island (in pass 2b: A or C) gets the wanted number of jobs.  Models of three K4 size classes get jobs in every
    pass (class tile offsets, the side-stream fork)."""
    dim = 3
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(450)
    thre = F(-1.0)
    tab, isl = Cs.islands_table()
    st = new_store(dim)
    A, B, C = isl[:, 0], isl[:, 1], isl[:, 2]
    give_models(st, tab, rng, pick=[A[2], A[3], A[4], A[19], A[20], A[21], A[10], A[11], A[12], C[10], C[11], C[12], B[5], B[6], B[7]])
    want = {2: (range(0, 5), [0, 1, 31, 32, 33]), 3: (range(8, 13), [0, 1, 9, 10, 11]), 1: (range(18, 23), [0, 1, 7, 8, 9])}

    def jobs_per_model(x):
        R, rec = reference(tab, x, g["half"], st)
        pairs = []
        K.blend_ref(R["ncand"], R["cand"], rec, np.zeros((x.shape[0], 8), dtype=F), thre, g["prior"], dim, pairs=pairs)
        return R, rec, pairs

    pool, own = Cs.island_queries(tab, isl, rng, 80)
    R, rec, pairs = jobs_per_model(pool)
    assert np.all(R["count"] == np.where(own < 18, 3, 2)) and np.all(R["cell"][0] == B[own])
    q3, s3 = pairs[3][:, 0], pairs[3][:, 1]
    target = A.copy()                                                 # the cell whose jobs are counted: A, or C where pass 2b reads C more often
    keep = []
    for i in range(27):
        mine = np.nonzero(own == i)[0]
        if i in want[3][0]:
            t = want[3][1][i - 8]
            reads = {c: np.isin(mine, q3[R["cell"][s3, q3] == c]) for c in (A[i], C[i])}
            target[i] = max(reads, key=lambda c: reads[c].sum())
            yes, no = mine[reads[target[i]]], mine[~reads[target[i]]]
            assert yes.size >= t, (i, yes.size)
            keep.append(np.concatenate([yes[:t], no[:3]]))
        else:
            t = want[2][1][i] if i in want[2][0] else want[1][1][i - 18] if i in want[1][0] else 3
            keep.append(mine[:t])
    x = pool[np.sort(np.concatenate(keep))]
    R, rec, pairs = jobs_per_model(x)
    per = [np.bincount(R["cand"][p[:, 1], p[:, 0]], minlength=tab["model"].max() + 1) for p in pairs]
    for p, (islands, counts) in want.items():
        got = [int(per[p][tab["model"][target[i]]]) for i in islands]
        assert got == counts, (p, got, counts)
        assert len(size_classes(tab, R["cand"][pairs[p][:, 1], pairs[p][:, 0]])) >= 3, p
    assert len(size_classes(tab, R["cand"][0])) >= 3
    probe = new_probe(st, g["half"], thre, g["prior"])
    set_table(probe, tab)
    exp, branch, jobs, h = check("tile edges", probe, x, R, rec, thre, g["prior"], dim)
    print("   jobs per model, histogram per pass: %s" % [np.bincount(c).tolist() for c in per])
    assert all(j > 0 for j in jobs) and not any(k.startswith(("2:pick", "3:pick")) and v for k, v in h.items())
    probe.close(); st.close()


def _blend_setup(dim, share):
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(500 + dim + share)
    tab = Cs.table(dim, "sparse", seed=2, occupancy=0.4 if share else 0.08)       # (sparse: many one- and two-candidate queries)
    st = new_store(dim)
    if share:       # three neighbouring cells (traversal order) share one model: exactly equal variances
        ncl = tab["c"].shape[0]
        slots = train(st, dim, tab["c"][::3], rng)
        tab["model"] = slots[np.arange(ncl) // 3].astype(np.int32)
    else:
        give_models(st, tab, rng)
    x = np.concatenate([Cs.queries_random(tab, rng, 9000, margin=0.5), K.queries_aligned(tab, rng, 1000)]).astype(F)
    R, rec = reference(tab, x, g["half"], st)
    return g, tab, st, x, R, rec


@pytest.mark.parametrize("dim", [3, 2])
def test_blend_branches_and_exact_thresholds(dim):
    """var_thre at the median first variance: every reachable branch (one candidate, gate closed, two candidates pick / blend,
    three candidates in each variance order pick / blend).  Then var_thre on the exact bits of one query's first variance (the
    gate's strict >) and of one query's best fall-back variance (the pick's strict <)."""
    g, tab, st, x, R, rec = _blend_setup(dim, 0)
    multi = R["ncand"] >= 2
    v0 = rec[:, 0, 4]
    med = F(np.median(v0[multi]))
    _, branch_med, _ = K.blend_ref(R["ncand"], R["cand"], rec, np.zeros((x.shape[0], 2 * (1 + dim)), dtype=F), med, g["prior"], dim)
    q_gate = int(np.nonzero(multi & (v0 > med))[0][0])
    q_pick = int(np.nonzero(branch_med >= 22)[0][0])                    # a three-candidate blend whose best is not the first: v0 > best >= med
    best = F(min(rec[q_pick, s, 4] for s in range(3)))
    for what, thre in (("median", med), ("first variance", F(v0[q_gate])), ("best fall-back variance", best)):
        probe = new_probe(st, g["half"], thre, g["prior"])
        set_table(probe, tab)
        exp, branch, jobs, h = check("blend %d-D, threshold = %s" % (dim, what), probe, x, R, rec, thre, g["prior"], dim)
        if what == "median":
            assert all(h[k] > 0 for k in K.REACHABLE), h
        elif what == "first variance":
            assert branch[q_gate] == 2                                   # v == thre does not open the gate
        else:
            assert branch[q_pick] >= 20                                  # v == thre is not picked alone: blended, w1 == 0
        probe.close()
    st.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_blend_equal_variances_and_zero_weight_sum(dim):
    """Neighbouring cells share a model: exactly equal variances (the stable order of decide and of the blend must agree), and
    with var_thre on that value w12 == 0: the NaN / inf of the float32 reference, bit for bit."""
    g, tab, st, x, R, rec = _blend_setup(dim, 1)
    same = (R["ncand"] == 3) & (R["cand"][1] == R["cand"][2]) & (R["cand"][0] != R["cand"][1])
    eq01 = (R["ncand"] >= 2) & (R["cand"][0] == R["cand"][1])
    open_ = same & (rec[:, 0, 4] > rec[:, 1, 4])
    assert open_.sum() > 20 and eq01.sum() > 20, (open_.sum(), eq01.sum())
    q = int(np.nonzero(open_)[0][0])
    for what, thre in (("median", F(np.median(rec[R["ncand"] >= 2, 0, 4]))), ("the shared variance", F(rec[q, 1, 4]))):
        probe = new_probe(st, g["half"], thre, g["prior"])
        set_table(probe, tab)
        exp, branch, jobs, h = check("equal variances %d-D, threshold = %s" % (dim, what), probe, x, R, rec, thre, g["prior"], dim)
        if what != "median":
            assert not np.isfinite(exp[q]).all() and branch[q] >= 20     # w1 = w2 = 0
        else:
            assert ((branch >= 3) & (same | eq01)).sum() > 20
        probe.close()
    st.close()


def test_cells_without_a_model():
    """model = -1 in candidate position 0, 1, 2, in two and in all three: the result is the reference's function of the pre-fill
    (first candidate: the pre-filled record and the prior variance; second / third: the prior), and the records an earlier,
    larger run left in the scratch do not show."""
    dim = 3
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(600)
    tab = Cs.table(dim, "dense")
    st = new_store(dim)
    give_models(st, tab, rng)
    x, _ = Cs.lookup_queries(tab, 7)
    big = Cs.queries_random(tab, rng, 3 * x.shape[0], margin=0.2)
    probe = new_probe(st, g["half"], F(0.05), g["prior"])
    set_table(probe, tab)
    probe.run(big, np.zeros((big.shape[0], 8), dtype=F))                 # fills the record scratch of every pass
    assert probe.pass_jobs()[0] > x.shape[0] and probe.pass_jobs()[2] > x.shape[0]
    Cs.punch_holes(tab, 3)
    set_table(probe, tab)
    R, rec = reference(tab, x, g["half"], st)
    holes = Cs.hole_positions(R["ncand"], R["cand"])
    assert all(v >= 10 for v in holes.values()), holes
    exp, branch, jobs, h = check("modelless cells", probe, x, R, rec, F(0.05), g["prior"], dim)
    print("   positions without a model:", holes)
    assert ((R["cand"][0] < 0) & (R["ncand"] >= 2) & (branch >= 3)).sum() > 20      # the pre-filled record went through the blend
    probe.close(); st.close()


def test_chunks_and_reuse():
    """One handle through growing and shrinking runs, chunk seams, a larger table and more models: the bits of a fresh handle's
    single-chunk run every time.  n = 0 and an empty table (prior only) included.  The chunk of 7 runs on the first 600 of the
    5000 queries, to keep the run short."""
    dim = 3
    g = Cs.GEOM[dim]
    rng = np.random.default_rng(700)
    tab = Cs.table(dim, "sparse")
    st = new_store(dim)
    give_models(st, tab, rng)
    xs = Cs.queries_random(tab, rng, 5000, margin=0.5)
    thre = F(0.3)
    probe = new_probe(st, g["half"], thre, g["prior"])
    set_table(probe, tab)

    def fresh(t, x):
        p = new_probe(st, g["half"], thre, g["prior"])
        set_table(p, t)
        R, rec = reference(t, x, g["half"], st)
        exp, branch, jobs, h = check("fresh handle, n = %d" % x.shape[0], p, x, R, rec, thre, g["prior"], dim, prefills=(12345.0,))
        p.close()
        return exp, jobs

    def same(x, want, jobs, chunk=0):
        probe.set_chunk(chunk)
        got = probe.run(x, np.full((x.shape[0], 8), 12345.0, dtype=F))
        assert np.array_equal(got.view(U), want.view(U)) and probe.pass_jobs() == jobs, (x.shape[0], chunk)

    e100, j100 = fresh(tab, xs[:100])
    e5000, j5000 = fresh(tab, xs)
    same(xs[:100], e100, j100)
    same(xs, e5000, j5000, chunk=1000)
    with pytest.raises(Exception):
        probe.candidates()                                               # more than one chunk: GPIS_ERR_STATE
    same(xs[:600], e5000[:600], fresh(tab, xs[:600])[1], chunk=7)        # (600 of the 5000: 86 chunks of 7)
    assert probe.run(np.zeros((0, 3), dtype=F), np.zeros((0, 8), dtype=F)).shape == (0, 8)
    # a larger table on the live handle, then more models in the store
    tab2 = Cs.table(dim, "dense")
    give_models(st, tab2, rng)
    x2 = Cs.queries_random(tab2, rng, 3000, margin=0.5)
    e2, j2 = fresh(tab2, x2)
    set_table(probe, tab2)
    same(x2, e2, j2)
    tab3 = Cs.n_cell_table(dim, 3000)
    give_models(st, tab3, rng)                                           # 703 + 512 + 3000 slots: the per-model arrays regrow
    x3 = Cs.queries_random(tab3, rng, 3000, margin=0.5)
    e3, j3 = fresh(tab3, x3)
    set_table(probe, tab3)
    same(x3, e3, j3, chunk=1024)
    set_table(probe, tab)
    same(xs[:100], e100, j100)
    # an empty table: the prior variance and nothing else
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in tab.items()}
    set_table(probe, empty)
    got = probe.run(xs[:100], np.full((100, 8), 12345.0, dtype=F))
    want = np.full((100, 8), 12345.0, dtype=F); want[:, 4] = g["prior"]
    assert np.array_equal(got.view(U), want.view(U)) and probe.pass_jobs() == [0, 0, 0, 0]
    probe.close(); st.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_real_maps_through_the_shipping_path(dim):
    """gpis3_test / gpis2_test on the bench map / the 2-D sequence equal blend_ref over the map's own candidates (the oracle's
    table and per-candidate records), where the oracle defines them: ties the probe's reference to the path the maps take."""
    import gpismap_amd
    import oracle_lib
    import replay
    g = Cs.GEOM[dim]
    if dim == 3:
        cam = np.array([568.0, 568.0, 310.0, 224.0, 640, 480])
        gm, om = gpismap_amd.GPisMap3(cam), oracle_lib.OracleMap3(cam, threads=8)
        gm.update(replay.synthetic_depth(0), replay.IDENTITY_POSE); om.update(replay.synthetic_depth(0), replay.IDENTITY_POSE)
        grid = replay.synthetic_grid(10)
    else:
        gm, om = gpismap_amd.GPisMap(), oracle_lib.OracleMap2()
        for f in replay.load_gazebo():
            gm.update(f["thetas"], f["ranges"], f["pose"]); om.update(f["thetas"], f["ranges"], f["pose"])
        grid = replay.demo2_grid()[::83]
    tab = om.k5_table()
    tab["pitch"] = 2.0 * float(g["cluster_half"])
    x = np.concatenate([grid, K.queries_aligned(tab, np.random.default_rng(5), 400)]).astype(F)
    count, idx, rec = om.k5_candidates(x)
    R = K.lookup_ref(tab, x, g["half"])
    assert np.array_equal(R["cell"].T, idx)
    full = np.all((R["cand"] >= 0) | (np.arange(3)[:, None] >= R["ncand"][None, :]), axis=0)
    exp, branch, jobs = K.blend_ref(R["ncand"], R["cand"], rec, np.zeros((x.shape[0], 2 * (1 + dim)), dtype=F), g["var_thre"], g["prior"], dim)
    got = gm.test(x)
    assert full.sum() > x.shape[0] // 2 and (branch[full] >= 3).sum() > 20 and R["tie"][full].sum() > 20
    assert np.array_equal(got[full].view(U), exp[full].view(U))
    # (jobs count only candidates with a model, so they are defined for every query; the maps report the passes by name)
    assert [gm.pass_jobs()[k] for k in gpismap_amd.GPisMap3.PASS_KEYS] == jobs
    print("\nreal map %d-D: %d queries (%d compared), ties %d, jobs %s, branches %s" % (
        dim, x.shape[0], full.sum(), R["tie"].sum(), jobs, {k: v for k, v in K.branch_histogram(branch).items() if v}))


def test_error_paths():
    """Checked on the host, before anything reaches a kernel."""
    import ctypes as C
    import gpismap_amd
    L = gpismap_amd.lib()
    ARG, STATE = -1, -3
    assert L.gpis_mapquery_create(None, 0.075, 0.5, 1.0) is None
    assert L.gpis_mapquery_set_table(None, 0, None, None, None, None, None, 0, None, None, None, 0.05) == ARG
    assert L.gpis_mapquery_run(None, None, 0, None) == ARG and L.gpis_mapquery_set_chunk(None, 0) == ARG
    assert L.gpis_mapquery_candidates(None, None, None) == ARG and L.gpis_mapquery_pass_jobs(None, None) == ARG
    assert L.gpis_mapquery_run_device(None, None, 0, None, None) == ARG
    st = new_store(3)
    tab = Cs.box_table(3, (2, 2, 2))
    give_models(st, tab, np.random.default_rng(1), big=False)
    probe = new_probe(st, 0.075, 0.5, 1.005)
    p = gpismap_amd._p
    i32 = lambda a: p(np.ascontiguousarray(a, dtype=np.int32), C.c_int)
    args = lambda model, parent, ap, ncl=8: (probe.h, ncl, p(tab["c"]), p(tab["lo"]), p(tab["hi"]), i32(model), i32(parent),
                                             tab["anc_parent"].size, p(tab["anc_lo"]), p(tab["anc_hi"]), i32(ap), C.c_double(0.05))
    nanc = tab["anc_parent"].size
    assert L.gpis_mapquery_set_table(*args(tab["model"], tab["parent"], tab["anc_parent"], ncl=-1)) == ARG
    assert L.gpis_mapquery_set_table(*args(tab["model"], np.full(8, nanc), tab["anc_parent"])) == ARG        # parent out of range
    assert L.gpis_mapquery_set_table(*args(tab["model"], np.full(8, -2), tab["anc_parent"])) == ARG
    assert L.gpis_mapquery_set_table(*args(tab["model"], tab["parent"], np.arange(nanc))) == ARG             # an ancestor its own parent
    assert L.gpis_mapquery_set_table(*args(np.full(8, 99), tab["parent"], tab["anc_parent"])) == ARG          # not a slot of the store
    assert L.gpis_mapquery_set_chunk(probe.h, -1) == ARG
    for entry, tail in ((L.gpis_mapquery_run, ()), (L.gpis_mapquery_run_device, (None,))):     # the same refusals in both forms
        assert entry(probe.h, None, -1, None, *tail) == ARG and entry(probe.h, None, 4, None, *tail) == ARG
        assert entry(probe.h, None, 0, None, *tail) == 0                                     # n = 0: nothing to do
    assert L.gpis_mapquery_candidates(probe.h, i32(np.zeros(8)), i32(np.zeros(24))) == STATE                  # nothing run yet
    assert L.gpis_mapquery_set_table(*args(tab["model"], tab["parent"], tab["anc_parent"])) == 0
    x = tab["c"][:, :3].copy()
    R, rec = reference(tab, x, F(0.075), st)
    check("after the refusals", probe, x, R, rec, F(0.5), F(1.005), 3)
    probe.close(); st.close()
