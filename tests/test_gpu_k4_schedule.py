"""The K4 schedule of test() (gpis_mapquery_set_k4_schedule) and the chunk that follows the call (gpis_mapquery_set_chunk(mq, 0)):
schedule 1 = the whole call in one chunk where the device has the memory, so that a pass is one K4 launch per size class; schedule
0 = chunks of 2^22 queries.  Where a chunk ends enters no result: every comparison here is bit for bit.

Store: a row of nine cluster cells along x with one model each at 16, 17, 32, 33, 48 and 49 block rows (both sides of every edge
of the 8-wavefront classes 4, 5, 6; K = 32 nbx - 5), one at K = 1024 (a multiple of 32: the mean-alone path, 33 block rows) and
two small ones of 3 and 7 block rows, in an order that is not the size order.  The queries lie inside the cells, so that every
model is some query's first, second and third candidate; var_thre = -1 sends every query through pass 2.
Through the kernel-level C-ABI (OnGPIS.train, gpis_mapquery_*), as test_gpu_ongpis.py / test_gpu_k5.py."""
import ctypes as C
import time

import numpy as np
import pytest

import k5_cases as Cs
import k5_ref as K
from test_gpu_ongpis import soa9

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
DIM = 3
G = Cs.GEOM[DIM]
# block rows per cell, in cell order along x (= slot order: not the size order); 0 marks the K = 1024 cluster
NBX = [17, 3, 49, 32, 0, 16, 48, 7, 33]


def class_of(nbx):
    return 0 if nbx <= 4 else 1 if nbx <= 8 else 2 if nbx <= 9 else 3 if nbx <= 16 else 4 if nbx <= 32 else 5 if nbx <= 48 else 6


def cluster_points(rng, K_rows):
    """A surface patch of K_rows = N + 3 Ng rows: Ng points with a normal, N - Ng without (value-only)."""
    ng = K_rows // 4
    n = K_rows - 3 * ng
    scale = G["scale"]
    ext = 2.0 * scale
    pos = rng.uniform(-ext, ext, (n, 3)).astype(F)
    pos[:, 2] = (0.2 * ext * np.sin(3 * pos[:, 0] / ext) * np.cos(2 * pos[:, 1] / ext)).astype(F)
    nrm = np.stack([-0.3 * np.cos(3 * pos[:, 0] / ext), 0.2 * np.sin(2 * pos[:, 1] / ext), np.ones(n)], axis=1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nrm[ng:] = 0.0
    val = np.full(n, -0.2, dtype=F)
    sx = rng.uniform(1e-3, 5e-3, n).astype(F)
    sg = rng.uniform(0.01, 0.1, n).astype(F)
    return pos, nrm, val, sx, sg


def train_row(rows, seed=11):
    """One model per entry of rows (K each) on a row of len(rows) cells.  Returns (store, table, dims {slot: (N, K, ld)})."""
    import gpismap_amd
    rng = np.random.default_rng(seed)
    tab = Cs.box_table(DIM, (len(rows), 1, 1))
    order = np.argsort(tab["ijk"][:, 0], kind="stable")            # table index of the cell at x = 0, 1, ...
    cl = [cluster_points(rng, k) for k in rows]
    sizes = [c[2].size for c in cl]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cat = [np.concatenate([c[j] for c in cl]) for j in range(5)]
    # the points of cluster i around the centre of its cell (the predictor of pass 2F scores candidates by their points)
    cat[0] = cat[0] + np.repeat(tab["c"][order, :3], sizes, axis=0)
    st = gpismap_amd.OnGPIS(DIM, G["scale"])
    slots = st.train(soa9(DIM, *cat), off, np.arange(off[-1], dtype=np.int32))
    dims = {}
    for i, s in enumerate(slots):
        d = np.zeros(4, dtype=np.int32)
        assert st.L.gpis_ongpis_model_dims(st.h, int(s), d.ctypes.data_as(C.POINTER(C.c_int))) == 0
        dims[int(s)] = (int(d[0]), int(d[2]), int(d[3]))
        assert dims[int(s)][1] == rows[i] and dims[int(s)][2] == 32 * (rows[i] // 32 + 1), (rows[i], dims[int(s)])
    model = np.zeros(len(rows), dtype=np.int32)
    model[order] = slots
    tab["model"] = model
    return st, tab, dims


def queries(tab, rng, n):
    """n queries inside the cells (round robin over the cells, anywhere along x inside a cell, near its axis)."""
    ncl = tab["c"].shape[0]
    own = np.arange(n) % ncl
    jit = rng.uniform(-1, 1, (n, 3)) * np.array([0.98, 0.3, 0.3])
    return (tab["c"][own, :3].astype(np.float64) + jit * float(G["cluster_half"])).astype(F)


def new_probe(st, tab, thre=-1.0):
    import gpismap_amd
    p = gpismap_amd.MapQueryProbe(st, G["half"], F(thre), G["prior"])
    p.set_table(tab["c"], tab["lo"], tab["hi"], tab["model"], tab["parent"], tab["anc_lo"], tab["anc_hi"], tab["anc_parent"], tab["pitch"])
    return p


def run(probe, x, schedule, chunk=0, pass2=1):
    probe.set_k4_schedule(schedule); probe.set_chunk(chunk); probe.set_pass2_mode(pass2)
    res = probe.run(x, np.full((x.shape[0], 8), 12345.0, dtype=F))
    return res, probe.last_counts(), probe.pass_jobs()


@pytest.fixture(scope="module")
def row():
    rows = [1024 if b == 0 else 32 * b - 5 for b in NBX]
    st, tab, dims = train_row(rows)
    assert sorted(d[2] // 32 for d in dims.values()) == sorted(33 if b == 0 else b for b in NBX)
    assert {class_of(d[2] // 32) for d in dims.values()} == {0, 1, 3, 4, 5, 6}
    rng = np.random.default_rng(12)
    xs = {n: queries(tab, rng, n) for n in (300, 6000)}
    probe = new_probe(st, tab)
    yield dict(st=st, tab=tab, dims=dims, xs=xs, probe=probe)
    probe.close(); st.close()


def test_every_model_is_first_second_and_third_candidate(row):
    for n, x in row["xs"].items():
        run(row["probe"], x, 1)
        nc, cd = row["probe"].candidates()
        assert set(np.unique(nc)) == {2, 3}                          # (the outer halves of the end cells see two cells)
        for k in range(3):
            assert set(np.unique(cd[k][cd[k] >= 0])) == set(row["dims"]), (n, k)


@pytest.mark.parametrize("pass2", [0, 1])
@pytest.mark.parametrize("n", [300, 6000])
def test_schedules_give_the_same_bits(row, n, pass2):
    """~300 queries: most launches have fewer than 64 tiles (the untransposed remainder path of the kernel's tile index); ~6 000:
    launches above 64 tiles with a remainder."""
    x = row["xs"][n]
    r0, c0, j0 = run(row["probe"], x, 0, pass2=pass2)
    r1, c1, j1 = run(row["probe"], x, 1, pass2=pass2)
    assert np.isfinite(r0).all()
    assert np.array_equal(r0.view(np.int32), r1.view(np.int32))
    assert c0["last_test_evals"] == c1["last_test_evals"] and j0 == j1 and all(j > 0 for j in j0)
    assert c1["last_test_k4_launches"] == c0["last_test_k4_launches"]          # (one chunk in both at these sizes)
    assert (c0["k4_schedule"], c1["k4_schedule"]) == (0, 1)
    print("\nn %d pass2_mode %d: launches %d, jobs %s" % (n, pass2, c1["last_test_k4_launches"], j0))


def test_chunks_give_the_same_bits(row):
    x = row["xs"][6000]
    ref, c, j = run(row["probe"], x, 0)
    assert c["chunk"] == 1 << 22
    for chunk in (64, 1000, 4096, 0):
        got, c, jc = run(row["probe"], x, 1, chunk=chunk)
        assert c["chunk"] == (chunk if chunk else 1 << 22)           # (automatic: never below 2^22 queries, whatever the call)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)) and jc == j, chunk


def test_launch_counts(row):
    """pass2_mode 0, whose job lists follow from the records alone (k5_ref.blend_ref): one launch per (chunk, pass, class with a
    job in it) -- with the automatic chunk one per (pass, class), with chunks of 1000 the larger count from the chunks' class
    populations."""
    st, tab, dims, probe = row["st"], row["tab"], row["dims"], row["probe"]
    x = row["xs"][6000]
    r1, c1, j1 = run(probe, x, 1, pass2=0)
    nc, cd = probe.candidates()
    rec = np.zeros((x.shape[0], 3, 8), dtype=F)
    k, q = np.nonzero(cd >= 0)
    rec[q, k] = st.eval(x, q, cd[k, q], layout=0)
    pairs = []
    K.blend_ref(nc, cd, rec, np.full((x.shape[0], 8), 12345.0, dtype=F), F(-1.0), G["prior"], DIM, pairs=pairs)
    cls_of_slot = {s: class_of(d[2] // 32) for s, d in dims.items()}

    def count(chunk):
        total = 0
        for a in range(0, x.shape[0], chunk):
            for p in pairs:                                           # passes 1, 2 (all columns), 2a (value), 2b (gradient)
                sel = p[(p[:, 0] >= a) & (p[:, 0] < a + chunk)]
                total += len({cls_of_slot[int(m)] for m in np.unique(cd[sel[:, 1], sel[:, 0]])})
        return total

    whole = [len({cls_of_slot[int(m)] for m in np.unique(cd[p[:, 1], p[:, 0]])}) for p in pairs]
    assert whole[0] == 6 and c1["last_test_k4_launches"] == sum(whole) == count(1 << 22) <= 4 * 6
    r0, c0, j0 = run(probe, x, 0, chunk=1000, pass2=0)
    assert c0["last_test_k4_launches"] == count(1000) > c1["last_test_k4_launches"]
    assert c0["last_test_evals"] == c1["last_test_evals"] and j0 == j1 == [int(p.shape[0]) for p in pairs]
    assert np.array_equal(r0.view(np.int32), r1.view(np.int32))
    # with the prediction on: at most one launch per (pass, class)
    r2, c2, j2 = run(probe, x, 1, pass2=1)
    assert c2["last_test_k4_launches"] <= 4 * 6 and j2 == j1 and c2["last_test_evals"] == c0["last_test_evals"]
    print("\nlaunches: chunk 1000 %d, one chunk %d (%s per pass), with the prediction %d" % (
        c0["last_test_k4_launches"], c1["last_test_k4_launches"], whole, c2["last_test_k4_launches"]))


def test_a_call_above_2_22_queries_runs_in_one_chunk():
    """The smallest call at which the automatic chunk differs from 2^22: 2^22 + 1000 queries (three tiny models, pass 1 only).
    Schedule 1 takes it whole (its scratch, ~156 bytes per query, is far below an eighth of the device's memory), schedule 0 in two
    chunks with twice the launches; the same bits, across the seam too."""
    st, tab, dims = train_row([12, 20, 12], seed=15)
    n = (1 << 22) + 1000
    x = queries(tab, np.random.default_rng(16), n)
    probe = new_probe(st, tab, thre=1e9)
    r1, c1, j1 = run(probe, x, 1)
    r0, c0, j0 = run(probe, x, 0)
    assert c1["chunk"] == n and c0["chunk"] == 1 << 22
    assert j1 == [n, 0, 0, 0] == j0 and c1["last_test_evals"] == n == c0["last_test_evals"]
    assert c1["last_test_k4_launches"] == 1 and c0["last_test_k4_launches"] == 2      # (one size class)
    assert np.isfinite(r1).all() and np.array_equal(r0.view(np.int32), r1.view(np.int32))
    probe.close(); st.close()


@pytest.mark.parametrize("schedule", [1, 0])
def test_ring_wait_expiry_is_reported_under_the_schedule(row, schedule):
    """The ring-expiry hook (gpis_ongpis_set_debug bit 4: the first workgroup of every launch withholds one signal behind a bounded
    wait) as in test_gpu_ongpis.py::test_ring_wait_expiry_of_the_predictor_is_reported, through test(): the call fails with
    GPIS_ERR_STATE, exactly the queries of each launch's first workgroup are NaN in every column, everything else keeps its bits, the
    next call is clean.  var_thre above every variance keeps the call to pass 1, where a NaN record is the query's result.
    The first tile of a launch is the first of the lowest slot of its class."""
    st, tab, dims = row["st"], row["tab"], row["dims"]
    x = row["xs"][300]
    probe = new_probe(st, tab, thre=1e9)
    clean, c, j = run(probe, x, schedule)
    assert np.isfinite(clean).all() and j == [300, 0, 0, 0]
    nc, cd = probe.candidates()
    cls_of_slot = {s: class_of(d[2] // 32) for s, d in dims.items()}
    first = [min(s for s in dims if cls_of_slot[s] == k) for k in sorted(set(cls_of_slot.values()))]
    assert c["last_test_k4_launches"] == len(first) == 6
    L = probe.L
    fp = C.POINTER(C.c_float)
    out = np.full((300, 8), 12345.0, dtype=F)
    st.set_debug(inject=16)
    try:
        t0 = time.time()
        rc = L.gpis_mapquery_run(probe.h, x.ctypes.data_as(fp), 300, out.ctypes.data_as(fp))
        assert time.time() - t0 < 20.0                                # bounded
    finally:
        st.set_debug(inject=0)
    assert rc == -3                                                   # GPIS_ERR_STATE
    bad = np.isnan(out).any(axis=1)
    assert np.isnan(out[bad]).all()
    for s in first:
        mine = cd[0] == s
        assert bad[mine].sum() == min(8, mine.sum()) == 8, (s, bad[mine].sum())
    assert bad.sum() == 8 * len(first)
    assert np.array_equal(out[~bad].view(U), clean[~bad].view(U))
    again, c, j = run(probe, x, schedule)
    assert np.array_equal(again.view(U), clean.view(U))
    probe.close()
