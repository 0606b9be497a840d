"""test() calls whose chunk lies beyond 2^24 queries, where the 32-bit offsets of its scratch end.

Since the chunk follows the call (MapQuery::chunk_for), every index that grows with the chunk -- records cap + 2q + s, candidates
cand[k * cap + q], jobs jm[2q + s], the sorted record jo = rec_base + j -- is bounded by kMaxChunk = 2^28 alone, and the float and
byte offsets made from them pass 2^31 and 2^32 inside one record buffer (96 bytes per query):

    byte offset 2^31 of a record              at cap >= 22 369 622
    byte offset 2^32                          at cap >= 44 739 243
    float offset record * 8 >= 2^31           at cap >= 89 478 486 (a record index of 2^28)
    d_res + 8 * off at float offset 2^31      at off = 2^28 (the second chunk of a call above kMaxChunk)

A wrap there does not fault: it writes one query's record over another's.  Every comparison is bit for bit against the old path: a
FRESH probe over the same store under K4 schedule 0 (chunks of 2^22 at cap = 2^22, every index small; a probe that has run a large
call keeps its large cap), which test_gpu_k4_schedule.py / test_gpu_k5.py pin to k5_ref and the oracle at small sizes; one
comparison of the dense test goes to k5_ref.blend_ref directly.

Store: three tiny models on a row of three cells (one block row each: K4's work per query is negligible, the index paths are the
cost).  Inputs are made on the device (the construction of test_gpu_k4_schedule.queries: round robin over the cells, jitter inside
the cell) and compared there; only the named samples reach the host.  Through gpis_mapquery_run_device."""
import numpy as np
import pytest

import k5_ref as K
from test_gpu_k4_schedule import DIM, G, new_probe, train_row

pytestmark = pytest.mark.gpu
F = np.float32
FILL = 12345.0
FAR = 1e3                                   # a world point outside every cell's search box: no candidate, no job

N_DENSE = 86 * (1 << 20) + 37               # the smallest multiple of 2^20 above 89 478 486, and a partial tile
Q27, Q28 = 22020077, 89128941               # where cap + 2q + 1 is record 2^27 (= 2^32 / 32 bytes) and record 2^28 at cap = N_DENSE
N_SPARSE = (1 << 28) + (1 << 22) + 37
WIN = 4096
WINDOWS = [(0, WIN), ((1 << 27) - WIN, (1 << 27) + WIN), ((1 << 28) - WIN, (1 << 28) + WIN), (N_SPARSE - WIN, N_SPARSE)]
N_HALVED = 3 * (1 << 22) + 5


def device_queries(tab, n, seed, first=0):
    """[n, 3] float32 on the device: query i inside cell (first + i) % ncl, anywhere along x, near the cell's axis."""
    import torch
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    c = torch.tensor(tab["c"][:, :3].astype(np.float64), device=dev)
    w = torch.tensor([0.98, 0.3, 0.3], dtype=torch.float64, device=dev) * float(G["cluster_half"])
    x = torch.empty((n, 3), dtype=torch.float32, device=dev)
    for a in range(0, n, 1 << 24):
        b = min(n, a + (1 << 24))
        own = torch.arange(first + a, first + b, device=dev) % c.shape[0]
        jit = torch.rand((b - a, 3), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        x[a:b] = (c[own] + jit * w).to(torch.float32)
    return x


def prefilled(n):
    import torch
    return torch.full((n, 8), FILL, dtype=torch.float32, device="cuda")


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_dev(probe, x, res, schedule, chunk=0, pass2=1):
    """x [n, 3], res [n, 8] contiguous device tensors (slices of rows are); res is input and output."""
    import torch
    assert x.is_contiguous() and res.is_contiguous() and res.shape == (x.shape[0], 8)
    probe.set_k4_schedule(schedule); probe.set_chunk(chunk); probe.set_pass2_mode(pass2)
    torch.cuda.synchronize()
    probe.run_device(x.data_ptr(), x.shape[0], res.data_ptr())
    return probe.last_counts(), probe.pass_jobs()


@pytest.fixture(scope="module")
def small():
    st, tab, dims = train_row([12, 20, 12], seed=15)
    yield st, tab
    st.close()


@pytest.fixture(scope="module")
def dense(small):
    """The dense queries and their results on the old path (shared by both pass-2 modes: every mode gives the same bits, the same
    pass_jobs and the same last_test_evals -- test_gpu_pass2_pick.py)."""
    import torch
    st, tab = small
    x = device_queries(tab, N_DENSE, 21)
    ref = prefilled(N_DENSE)
    probe = new_probe(st, tab, thre=-1.0)
    counts, jobs = run_dev(probe, x, ref, 0, pass2=0)
    probe.close()
    assert counts["chunk"] == 1 << 22 and counts["k4_schedule"] == 0
    yield dict(x=x, ref=ref, counts=counts, jobs=jobs)
    del x, ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pass2", [0, 1])
def test_dense_call_across_every_32_bit_boundary_of_the_record_buffer(small, dense, pass2):
    """90 177 573 queries in ONE chunk, every one through pass 2 (var_thre = -1): records up to 3 cap = 270 532 719 > 2^28, so the
    byte offsets of d_out_ pass 2^31 and 2^32 and the float offset record * 8 passes 2^31 -- in K4's store (ongpis_test.hip,
    o = out + job_out * 8), in jobs_decide's and the blend's reads of records cap + 2q + s, and in cand[k * cap + q].
    Then two small calls on the same probe, whose scratch keeps cap = 90 177 573 (the production pattern: a full grid, then probes).
    The 4096 sampled queries -- both ends, and around the two q where cap + 2q crosses record 2^27 and record 2^28 -- are checked
    against k5_ref (lookup_ref, blend_ref over records from OnGPIS.eval): that comparison does not rest on the old path."""
    import torch
    st, tab = small
    n, x, ref = N_DENSE, dense["x"], dense["ref"]
    assert n % (1 << 20) == 37 and n - 37 - (1 << 20) < 89478486 < n
    assert n + 2 * Q27 + 1 == 1 << 27 and n + 2 * Q28 + 1 == 1 << 28 and Q28 < n
    probe = new_probe(st, tab, thre=-1.0)
    try:
        res = prefilled(n)
        c, j = run_dev(probe, x, res, 1, pass2=pass2)
        print("\npass2_mode %d: chunk %d, jobs %s, evals %d, launches %d" % (pass2, c["chunk"], j, c["last_test_evals"], c["last_test_k4_launches"]))
        assert c["chunk"] == n and c["k4_schedule"] == 1
        assert j[0] == n and j[1] > 0 and (j[2] > 0 or j[3] > 0)                 # pass 2 really ran, for both kinds of query
        assert bool(torch.isfinite(res).all())
        assert same_bits(res, ref)
        assert j == dense["jobs"] and c["last_test_evals"] == dense["counts"]["last_test_evals"]
        # small calls on the grown scratch: automatic chunk 2^22 for the first, the call for the second (which no longer asks for
        # more scratch than the probe holds)
        for a, m, chunk in ((0, 6000, 1 << 22), (Q27, (1 << 22) + 1000, (1 << 22) + 1000)):
            part = prefilled(m)
            cs, js = run_dev(probe, x[a:a + m], part, 1, pass2=pass2)
            assert cs["chunk"] == chunk and js[0] == m and js[1] > 0
            assert same_bits(part, res[a:a + m]) and same_bits(part, ref[a:a + m]), (a, m)
        # the samples against k5_ref
        idx = torch.cat([torch.arange(a, a + 1024, device="cuda") for a in (0, Q27 - 512, Q28 - 512, n - 1024)])
        xs, got = x[idx].cpu().numpy(), res[idx].cpu().numpy()
    finally:
        probe.close()
    R = K.lookup_ref(tab, xs, G["half"])
    nc, cd = R["ncand"], R["cand"]
    assert set(np.unique(nc)) == {2, 3}
    rec = np.zeros((xs.shape[0], 3, 8), dtype=F)
    k, q = np.nonzero(cd >= 0)
    rec[q, k] = st.eval(xs, q, cd[k, q], layout=0)
    exp, branch, jobs = K.blend_ref(nc, cd, rec, np.full((xs.shape[0], 8), FILL, dtype=F), F(-1.0), G["prior"], DIM)
    assert jobs[1] > 0 and jobs[2] > 0 and jobs[3] > 0
    assert np.array_equal(got.view(np.int32), exp.view(np.int32))


def test_sparse_call_across_the_largest_chunk(small):
    """2^28 + 2^22 + 37 queries with set_chunk(2^30): the chunk is clamped to kMaxChunk = 2^28, two chunks, the second written at
    d_res + 8 * 2^28 = float offset 2^31.  cap = 2^28: cand[2 cap + q] lies 2^31 .. 3 2^30 bytes into its array, pass-1 records up
    to float offset 2^31.  Real queries sit only in four windows -- both ends, around 2^27 (pass-2 records cap + 2q around 2^29)
    and across the seam at 2^28; everywhere else is one point with no candidate.
    Run twice: var_thre = 1e9 (pass 1 only) and var_thre = -1, which sends the windows through pass 2 at records cap + 2q + s up to
    3 2^28, record * 8 up to 6.4e9 floats.
    Outside the windows a query has no candidate: the call writes the prior variance into column 1 + dim (the reference does that
    before it looks anything up, GPisMap3.cpp:816) and nothing else, so the pre-fill must stand in the other seven columns of the
    whole buffer.  The windows are bit-equal to the same queries gathered into one small call on a fresh probe.
    About 42 GB of scratch and 12 GB of buffers: skipped only on a device whose TOTAL memory is below 96 GB."""
    import torch
    if torch.cuda.get_device_properties(0).total_memory < 96e9:
        pytest.skip("needs a device with at least 96 GB of memory")
    st, tab = small
    n = N_SPARSE
    assert WINDOWS[2][0] < 1 << 28 < WINDOWS[2][1] and WINDOWS[3][1] == n and WINDOWS[3][0] > WINDOWS[2][1]
    x = torch.full((n, 3), FAR, dtype=torch.float32, device="cuda")
    for i, (a, b) in enumerate(WINDOWS):
        x[a:b] = device_queries(tab, b - a, 31 + i, first=a)
    xs = torch.cat([x[a:b] for a, b in WINDOWS])
    res = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    untouched = torch.full((8,), FILL, dtype=torch.float32, device="cuda")
    untouched[1 + DIM] = float(G["prior"])
    for thre in (1e9, -1.0):
        rp = new_probe(st, tab, thre=thre)
        ref = prefilled(xs.shape[0])
        cr, jr = run_dev(rp, xs, ref, 0)
        rp.close()
        assert cr["chunk"] == 1 << 22 and jr[0] == xs.shape[0] and (jr[1] > 0 and jr[2] > 0) == (thre < 0)
        res.fill_(FILL)
        probe = new_probe(st, tab, thre=thre)
        try:
            c, j = run_dev(probe, x, res, 1, chunk=1 << 30)
        finally:
            probe.close()
        print("\nvar_thre %g: chunk %d, jobs %s, launches %d" % (thre, c["chunk"], j, c["last_test_k4_launches"]))
        assert c["chunk"] == 1 << 28                                             # the clamp: two chunks
        got = torch.cat([res[a:b] for a, b in WINDOWS])
        assert bool(torch.isfinite(got).all()) and same_bits(got, ref), thre
        assert j == jr and c["last_test_evals"] == cr["last_test_evals"]
        # everything else, over the whole buffer: blank the windows, then every row must be the untouched one
        for a, b in WINDOWS:
            res[a:b] = untouched
        assert bool((res.view(torch.int32) == untouched.view(torch.int32)).all()), thre


def test_chunk_halves_when_memory_is_short_and_never_below_2_22(small):
    """The automatic chunk under K4 schedule 1 of a call of n = 3 2^22 + 5 = 12 582 917 pass-1 queries, with a ballast that leaves a
    chosen amount of device memory free.  The rule (map_query.h / gpis_mapquery_set_chunk): the scratch of a chunk, 156 bytes per
    query (159 with the tile lists, 3 arrays of 2 (chunk / 8 + 1) ints), must fit in one eighth of the free memory; else the chunk is
    halved, (c + 1) / 2, and it is never below 2^22.
    12 GiB free: the room is 1.61 GB; the scratch of n is 1.96 GB (2.00 with the tile lists): too large; of (n + 1) / 2 = 6 291 459
    it is 0.98 GB (1.00): it fits.  The chunk is 6 291 459, an odd length: the seam falls inside a tile.  Any free amount from
    8.1 to 15.7 GB gives the same chunk.
    3 GiB free: the room is 0.40 GB, below the 0.65 GB (0.67) of 2^22 queries: halving goes 6 291 459, 3 145 730 and ends below the
    floor; the chunk is 2^22.  Any free amount below 5.2 GB that still holds the scratch gives the same.
    The same bits as the old path in both, each on a fresh probe (a probe keeps the scratch of its largest chunk, and chunk_for never
    halves below what the probe holds).  One ballast for both cases, grown by 9 GiB for the second: holding nearly the whole device
    is what this test's time goes to."""
    import torch
    st, tab = small
    n = N_HALVED
    x = device_queries(tab, n, 41)
    ref, res = prefilled(n), prefilled(n)
    probe = new_probe(st, tab, thre=1e9)
    c, j = run_dev(probe, x, ref, 0)
    probe.close()
    assert c["chunk"] == 1 << 22 and j == [n, 0, 0, 0] and bool(torch.isfinite(ref).all())
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    ballast = []
    try:
        for free_gib, lo, hi, chunk in ((12, 8.1e9, 15.7e9, 6291459), (3, 1.5e9, 5.2e9, 1 << 22)):
            free = torch.cuda.mem_get_info()[0]
            assert free > free_gib << 30, "the device has less free memory than the case leaves free: %d" % free
            ballast.append(torch.empty(free - (free_gib << 30), dtype=torch.uint8, device="cuda"))
            left = torch.cuda.mem_get_info()[0]
            assert lo <= left <= hi, left                                        # (of the test's own set-up)
            res.fill_(FILL)
            probe = new_probe(st, tab, thre=1e9)
            try:
                c, j = run_dev(probe, x, res, 1)
            finally:
                probe.close()
            print("\n%.2f GB free: chunk %d" % (left / 1e9, c["chunk"]))
            assert c["chunk"] == chunk and c["k4_schedule"] == 1, (free_gib, c)
            assert j == [n, 0, 0, 0] and c["last_test_evals"] == n
            assert same_bits(res, ref), free_gib
    finally:
        del ballast[:]
        torch.cuda.empty_cache()
