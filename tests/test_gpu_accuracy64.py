"""OnGPIS on the GPU against float64, at every size-class edge up to the largest cluster training accepts.

The parity tests pin the kernels to the oracle's `tiled` arithmetic, a CPU copy of their own operation order: a wrong intended
arithmetic would pass them.  Here the GPU's kernel matrix (K6 gather + K3 build), factor and alpha (K3), and predictions (K3b
inverse + K4) are held to ongpis_ref64's bound -- within 8 x the error of a plain float32 LAPACK pipeline on the same operands
(more for what is computed from the factor of clusters with many value-only points: ongpis_ref64.chain_ratio), plus 4 ulp --
both errors against float64.  Per cluster:
  build                      kernel_matrix against the float64 matrix
  factor, alpha              backward error of L and the residual of alpha, on the GPU's own matrix
  own_f .. own_var_g         K3b + K4 alone: predictions against float64 from the GPU's own L and alpha (baseline: strtrs with that L)
  f .. var_g                 end to end, against the float64 pipeline from the inputs
Queries 0.3 s, 1e-3 s and 1 s from training points and beyond a r = 104, plus one near a point of each of K4's row groups,
through layouts 0, 1 and 2 (the same bits per column)."""
import re
import time

import numpy as np
import pytest

import ongpis_ref64 as R
from test_gpu_ongpis import make_cluster, soa9

pytestmark = pytest.mark.gpu

S3, S2 = 0.04, 1.2


def cluster(rng, dim, scale, n, ng, dense):
    """n points, the first n - ng value-only (no normal), the rest with normals.  Above 300 points the patch grows to keep the
    density of a 300-point cluster: as sqrt(n) in 3-D (a surface), as n in 2-D (a curve); `dense` shrinks it."""
    grow = 1.0 if n <= 300 else (np.sqrt(n / 300.0) if dim == 3 else n / 300.0)
    pos, grad, val, sx, sg = make_cluster(rng, dim, n, scale * grow * dense, frac_nograd=0.0)
    grad[:n - ng] = 0.0
    return pos, grad, val, sx, sg


# (id, dim, scale, N, points with normals, patch density, OnGPIS options, cu reserve)
SHAPES = [
    ("K1", 3, S3, 1, 0, 1.0, {}, 0),
    ("K3_2d", 2, S2, 1, 1, 1.0, {}, 0),
    ("K4", 3, S3, 1, 1, 1.0, {}, 0),
    ("K31", 3, S3, 10, 7, 1.0, {}, 0),
    ("K32", 3, S3, 8, 8, 1.0, {}, 0),
    ("K33", 3, S3, 9, 8, 1.0, {}, 0),
    ("K31_2d", 2, S2, 11, 10, 1.0, {}, 0),
    ("K256_fused", 3, S3, 64, 64, 1.0, {}, 0),
    ("K256_separate", 3, S3, 64, 64, 1.0, {"fused": False}, 0),
    ("K257", 3, S3, 257, 0, 1.0, {}, 0),
    ("K260", 3, S3, 65, 65, 1.0, {}, 0),
    ("K600_dense", 3, S3, 150, 150, 0.2, {}, 0),
    ("K1200", 3, S3, 300, 300, 1.0, {}, 0),
    ("K1200_reserve64", 3, S3, 300, 300, 1.0, {}, 64),
    ("K1200_dense", 3, S3, 300, 300, 0.2, {}, 0),
    ("K1200_2d", 2, S2, 400, 400, 1.0, {}, 0),
    ("K2400", 3, S3, 600, 600, 1.0, {}, 0),
    ("K3600", 3, S3, 900, 900, 1.0, {}, 0),
    ("K3600_dense", 3, S3, 900, 900, 0.2, {}, 0),
    ("K9216", 3, S3, 2304, 2304, 1.0, {}, 0),          # the target vector just fits the back substitution's LDS buffer
    ("K9217", 3, S3, 2305, 2304, 1.0, {}, 0),          # one row more: the barrier path through global scratch
    ("K16384", 3, S3, 4096, 4096, 1.0, {}, 0),         # ONGPIS_MAX_K
    ("K7256_value_only", 3, S3, 7256, 0, 1.0, {}, 0),  # K4's LDS staging: 4 ld + 16 N bytes
    ("K7500_mixed", 3, S3, 3000, 1500, 1.0, {}, 0),    # half the points value-only
    ("K12000_mixed", 3, S3, 6000, 2000, 1.0, {}, 0),   # 4000 value-only rows among 8000 gradient rows
    ("K15549_2d", 2, S2, 5183, 5183, 1.0, {}, 0),
]


def gpu_outputs(st, p, slot):
    m = st.model(slot)
    assert (m["N"], m["K"]) == (p.pos.shape[0], p.K)
    np.testing.assert_array_equal(m["gidx"], p.gidx.astype(np.int32))
    Kmat = st.kernel_matrix(p.pos, m["gidx"], p.sigx.astype(np.float32), p.sg)
    nq = p.xq.shape[0]
    jq, jm = np.arange(nq, dtype=np.int32), np.full(nq, slot, dtype=np.int32)
    full = st.eval(p.xq, jq, jm, layout=0).copy()
    val = st.eval(p.xq, jq, jm, layout=1)
    grad = st.eval(p.xq, jq, jm, layout=2)
    nc = 1 + p.dim
    for cols, got in (([0, 4], val), (list(range(1, nc)) + list(range(5, 4 + nc)), grad)):
        assert np.array_equal(full[:, cols].view(np.uint32), got[:, cols].view(np.uint32))
    return dict(Kmat=Kmat, L=m["L"], alpha=m["alpha"], mean=full[:, :nc], var=full[:, 4:4 + nc])


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_cluster_against_float64(shape):
    import gpismap_amd
    name, dim, scale, n, ng, dense, opts, reserve = shape
    rng = np.random.default_rng(20261016 + n)
    pos, grad, val, sx, sg = cluster(rng, dim, scale, n, ng, dense)
    gidx = R.gather(pos, grad, val, sx, sg)[0]
    xq = np.concatenate([R.queries(rng, pos, scale), R.row_group_queries(rng, pos, gidx, n + dim * ng, scale)])
    p = R.Problem(dim, scale, pos, grad, val, sx, sg, xq)
    assert p.K == n + dim * ng
    t0 = time.time()
    st = gpismap_amd.OnGPIS(dim, scale, keep_factor=True, **opts)
    if reserve:
        st.set_cu_reserve(reserve)
    slots = st.train(soa9(dim, pos, grad, val, sx, sg), np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32))
    out = gpu_outputs(st, p, slots[0])
    st.close()
    t1 = time.time()
    rows, ok = R.assess(p, **out)
    print("\n%-17s K=%5d  %s  (GPU %.1fs, reference %.1fs)" % (name, p.K, R.format_rows(rows), t1 - t0, time.time() - t1))
    assert len(rows) == 11
    assert p.xq.shape[0] == 24 + -(-p.K // 1024)
    assert ok, R.format_rows(rows)


@pytest.mark.parametrize("dim,scale,n,ng,K", [(3, S3, 4096, 4096, 16384), (3, S3, 7256, 0, 7256), (2, S2, 5183, 5183, 15549)],
                         ids=["3d_normals", "value_only", "2d_normals"])
def test_one_point_more_is_refused(dim, scale, n, ng, K):
    """The largest clusters above are the largest training accepts: one point more is refused with GPIS_ERR_LIMIT."""
    import gpismap_amd
    rng = np.random.default_rng(7 + n)
    pos, grad, val, sx, sg = cluster(rng, dim, scale, n + 1, ng + (ng > 0), 1.0)
    st = gpismap_amd.OnGPIS(dim, scale)
    with pytest.raises(gpismap_amd.GpisError) as e:
        st.train(soa9(dim, pos, grad, val, sx, sg), np.array([0, n + 1], dtype=np.int32), np.arange(n + 1, dtype=np.int32))
    assert re.search(r"status -4$", str(e.value)), str(e.value)      # GPIS_ERR_LIMIT
    print("\nN=%d (K=%d) refused: %s" % (n + 1, n + 1 + dim * (ng + (ng > 0)), e.value))
