"""k5_ref (the plain reference of test()'s lookup, candidate order, gate and blend) against the CPU oracle on the three
committed scenes, the populations of the synthetic generators the GPU tests rely on, and the negative controls.  No GPU.

Populations found (seed 7; asserted below with room to spare), queries / 0,1,2,3,4+ candidates / tie / std::sort differs from a
stable sort in the first three / pruned only by an ancestor / more than 16 candidates:
  3-D sparse  3381 / 220 53 69 84 2955 / 915 / 389 / 314 / 1660      (largest count 60)
  3-D dense   3399 / 261 10 36 31 3061 / 1228 / 803 / 302 / 2132     (largest count 125)
  2-D sparse  3234 / 17 6 11 18 3182 / 672 / 252 / 155 / 2109        (largest count 34)
  2-D dense   3228 / 22 0 0 0 3206 / 1056 / 761 / 231 / 2761         (largest count 64)
Cells without a model (3-D dense, a fifth of the cells): position 0 / 1 / 2 alone 444 / 403 / 422, two of them 75 / 84 / 69,
all three 17."""
import numpy as np
import pytest

import k5_cases as Cs
import k5_ref as K
import oracle_lib
import replay

F = np.float32


def _scene(name):
    if name == "bigbird":
        fr = replay.load_bigbird()
        om = oracle_lib.OracleMap3(fr[0]["cam"], threads=8)
        for f in fr[:2]:
            om.set_camera(f["cam"]); om.update(f["depth"], f["pose"])
        return om, 3, replay.demo3_grid()[::23]
    if name == "bench":
        om = oracle_lib.OracleMap3(np.array([568.0, 568.0, 310.0, 224.0, 640, 480]), threads=8)
        om.update(replay.synthetic_depth(0), replay.IDENTITY_POSE)
        return om, 3, replay.synthetic_grid(10)
    om = oracle_lib.OracleMap2()
    for f in replay.load_gazebo():
        om.update(f["thetas"], f["ranges"], f["pose"])
    return om, 2, replay.demo2_grid()[::83]


@pytest.mark.parametrize("name", ["bigbird", "bench", "gazebo"])
def test_reference_matches_oracle_on_the_scenes(name):
    om, dim, grid = _scene(name)
    g = Cs.GEOM[dim]
    T = om.k5_table()
    T["pitch"] = 2.0 * float(g["cluster_half"])
    assert T["c"].shape[0] > 20 and (T["model"] >= 0).any()
    rng = np.random.default_rng(5)
    x = np.concatenate([grid, K.queries_aligned(T, rng, 600)]).astype(F)
    count, idx, rec = om.k5_candidates(x, maxc=8)
    R = K.lookup_ref(T, x, g["half"], max_keep=8)
    assert np.array_equal(R["count"], count)
    assert np.array_equal(R["cell"].T, idx)
    if dim == 3:        # (the 2-D oracle reports no tie / sort flags: there the reference's own, on candidates just shown equal)
        fl = om.test_flags(x)
        assert np.array_equal((fl & 1) != 0, R["tie"])
        assert np.array_equal((fl & 8) != 0, R["unstable"])
        assert np.array_equal((fl & 16) != 0, count > 16)
    assert R["tie"].sum() > 50 and (count > 16).sum() > 50, "the query set lost its ties / its large candidate sets"
    # blend: where every candidate the oracle reads has a GP (it dereferences a null one otherwise)
    full = np.all((R["cand"] >= 0) | (np.arange(3)[:, None] >= R["ncand"][None, :]), axis=0)
    assert full.sum() > x.shape[0] // 2
    ro = om.test(x)
    res, branch, jobs = K.blend_ref(R["ncand"], R["cand"], rec, np.zeros_like(ro), g["var_thre"], g["prior"], dim)
    assert np.array_equal(res[full].view(np.uint32), ro[full].view(np.uint32))
    assert (branch[full] >= 3).sum() > 20, "no query reached the blend"
    print("\n%s: %d cells, %d queries, candidates %s, ties %d, unstable %d, >16: %d, branches %s" % (
        name, T["c"].shape[0], x.shape[0], np.bincount(np.minimum(count, 4), minlength=5), R["tie"].sum(), R["unstable"].sum(),
        (count > 16).sum(), {k: v for k, v in K.branch_histogram(branch[full]).items() if v}))


def test_sort_perm_is_std_sort():
    """Up to 16 keys std::sort is an insertion sort (stable); beyond, equal keys move."""
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 4, 16 + 40 + 129).astype(F)
    off = np.array([0, 16, 56, 185])
    perm = oracle_lib.sort_perm(keys, off)
    moved = 0
    for a, b in zip(off[:-1], off[1:]):
        k, p = keys[a:b], perm[a:b]
        assert sorted(p) == list(range(b - a)) and np.all(np.diff(k[p]) >= 0)
        moved += int(np.any(p != np.argsort(k, kind="stable")))
    assert np.array_equal(perm[:16], np.argsort(keys[:16], kind="stable"))
    assert moved >= 1


CASES = [(3, "sparse"), (3, "dense"), (2, "sparse"), (2, "dense")]


@pytest.mark.parametrize("dim,kind", CASES, ids=["%dd_%s" % c for c in CASES])
def test_generator_populations_and_lookup_controls(dim, kind):
    T = Cs.table(dim, kind)
    x, cell = Cs.lookup_queries(T, 7)
    half = Cs.GEOM[dim]["half"]
    R = K.lookup_ref(T, x, half)
    hist = np.bincount(np.minimum(R["count"], 4), minlength=5)
    print("\n%d-D %s: %d cells, %d ancestors, %d queries, candidates %s (max %d), ties %d, unstable %d, pruned by an ancestor %d, >16: %d"
          % (dim, kind, T["c"].shape[0], T["anc_parent"].size, x.shape[0], hist, R["count"].max(), R["tie"].sum(), R["unstable"].sum(),
             (R["pruned"] > 0).sum(), (R["count"] > 16).sum()))
    assert R["tie"].sum() > 300 and R["unstable"].sum() > 100 and (R["pruned"] > 0).sum() > 50 and (R["count"] > 16).sum() > 500
    assert hist[0] > 10 and hist[4] > 1000
    if kind == "sparse":
        assert hist[1] > 3 and hist[2] > 5 and hist[3] > 5
    else:
        assert R["count"].max() == (125 if dim == 3 else 64)     # 2-D: search half 4.8 = 3 pitches: 7 x 7 aligned, 8 x 8 on a face
    # the crafted query (last): the cell's own box passes, its ancestor's does not
    assert R["pruned"][-1] >= 1 and cell not in R["cell"][:, -1]
    # negative controls: each defective variant changes the candidates
    assert (K.lookup_ref(T, x, half, stable_sort=True)["cell"] != R["cell"]).any(axis=0).sum() == R["unstable"].sum()
    assert (K.lookup_ref(T, x, half, exclusive_box=True)["count"] != R["count"]).sum() > 100
    Rn = K.lookup_ref(T, x, half, no_ancestors=True)
    assert np.array_equal(Rn["count"] != R["count"], R["pruned"] > 0) and Rn["count"][-1] > R["count"][-1]


def test_modelless_positions_and_blend_controls():
    """Cells without a model in every candidate position; the blend's defective variants change results on synthetic records
    that hold the exact equalities (variance == threshold, equal variances, w12 == 0)."""
    dim = 3
    g = Cs.GEOM[dim]
    T = Cs.punch_holes(Cs.table(dim, "dense"), 3)
    x, _ = Cs.lookup_queries(T, 7)
    R = K.lookup_ref(T, x, g["half"])
    holes = Cs.hole_positions(R["ncand"], R["cand"])
    print("\nmodelless positions", holes)
    assert all(v >= 10 for v in holes.values()), holes
    n = x.shape[0]
    rng = np.random.default_rng(11)
    rec = rng.normal(0, 1, (n, 3, 8)).astype(F)
    rec[:, :, 4] = rng.choice(np.array([0.25, 0.5, 0.75, 0.9], dtype=F), (n, 3))     # equal variances and v == thre abound
    for prefill in (np.zeros((n, 8), dtype=F), np.full((n, 8), 12345.0, dtype=F)):
        res, branch, jobs = K.blend_ref(R["ncand"], R["cand"], rec, prefill, g["var_thre"], g["prior"], dim)
        h = K.branch_histogram(branch)
        assert all(h[k] > 0 for k in K.REACHABLE) and sum(h.values()) == sum(h[k] for k in K.REACHABLE), h
        assert np.isnan(res).any()                                   # w12 == 0: both variances on the threshold
        untouched = (R["ncand"] == 0) | ((R["cand"][0] < 0) & (branch <= 2))
        cols = [c for c in range(8) if c != 4]
        assert untouched.sum() > 100 and np.array_equal(res[untouched][:, cols], prefill[untouched][:, cols])
        assert np.all(res[untouched, 4] == g["prior"])
        rge, bge, jge = K.blend_ref(R["ncand"], R["cand"], rec, prefill, g["var_thre"], g["prior"], dim, gate_ge=True)
        assert (bge != branch).sum() > 50 and jge != jobs
        rsw, bsw, jsw = K.blend_ref(R["ncand"], R["cand"], rec, prefill, g["var_thre"], g["prior"], dim, swap_weights=True)
        assert np.array_equal(bsw, branch) and jsw == jobs
        assert (rsw.view(np.uint32) != res.view(np.uint32)).any(axis=1).sum() > 50
        assert jobs[0] == int(((R["ncand"] >= 1) & (R["cand"][0] >= 0)).sum()) and jobs[2] >= jobs[3] > 0 and jobs[1] > 0


def test_tie_case_populations():
    """What the tie cases of the GPU tests rely on: more listed tie queries than one stride of the tie kernel (512 x 32) on the
    dense tables, and 127 / 128 / 129 candidates with ties under the wider search box, where std::sort and the stable order
    differ on both sides of 128."""
    for dim in (3, 2):
        tab = Cs.table(dim, "dense")
        x = K.queries_aligned(tab, np.random.default_rng(200 + dim), 30000)
        R = K.lookup_ref(tab, x, Cs.GEOM[dim]["half"])
        listed = R["tie"] & (R["count"] > 1) & (R["count"] <= 128)
        print("\n%d-D dense, 30000 aligned queries: %d listed tie queries, std::sort differs on %d" % (dim, listed.sum(), R["unstable"].sum()))
        assert listed.sum() > 512 * 32 and R["unstable"].sum() > 5000 and R["count"].max() == (125 if dim == 3 else 64)
    tab, x = Cs.tie_guard_case()
    assert tab["c"].shape[0] == 3 * 121 + 21
    R = K.lookup_ref(tab, x, Cs.TIE_GUARD_HALF)
    for want in (127, 128, 129):
        m = R["count"] == want
        assert (m & R["tie"]).sum() >= 1 and (m & R["unstable"]).sum() >= 1, (want, np.unique(R["count"]))


@pytest.mark.parametrize("slots,n", Cs.BINNING, ids=["m%d_n%d" % b for b in Cs.BINNING])
def test_binning_populations(slots, n):
    """Pass-1 jobs per model at every count of CYCLE, waves of one model (also behind a jobless lane 0), of 64 distinct models."""
    tab = Cs.n_cell_table(3, slots)
    assert tab["c"].shape[0] == slots
    x, cells, counted = Cs.binning_queries(tab, n, np.random.default_rng(400 + slots))
    R = K.lookup_ref(tab, x, Cs.GEOM[3]["half"])
    far = cells < 0
    assert x.shape[0] == n and np.array_equal(np.nonzero(far)[0], np.arange(Cs.NFAR) * 64)
    assert np.all(R["count"][far] == 0) and np.all(R["cell"][0][~far] == cells[~far])
    w = Cs.wave_populations(R["cell"][0])
    assert w["lane0"] >= 4 and w["one"] >= 1 and w["one_lane0"] >= 1 and (w["distinct"] >= 4 or slots == 1), w
    if slots > 1:
        per = np.bincount(cells[~far], minlength=slots)[:counted]
        assert counted >= 11 and all((per == c).sum() == counted // 11 for c in Cs.CYCLE)
        assert slots - counted >= 64 + 6                                 # room for the round robin and the six larger models


def test_island_populations():
    """A query inside B of an island has exactly the island's cells as candidates, B first."""
    tab, isl = Cs.islands_table()
    x, own = Cs.island_queries(tab, isl, np.random.default_rng(450), 80)
    R = K.lookup_ref(tab, x, Cs.GEOM[3]["half"])
    assert isl.shape == (27, 3) and (isl[:18] >= 0).all() and (isl[18:, 2] == -1).all()
    assert np.all(R["count"] == np.where(own < 18, 3, 2)) and np.all(R["cell"][0] == isl[own, 1])
    assert np.all(np.sort(R["cell"][1:, own < 18], axis=0) == np.sort(isl[own[own < 18]][:, [0, 2]].T, axis=0))
