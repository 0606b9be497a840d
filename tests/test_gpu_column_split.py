"""test() evaluates candidates 2 and 3 by result column: pass 2a computes only the value column, pass 2b the gradient columns of
the records the blend reads.  Every column must keep its bits: K4's column layouts against the all-column layout on one model,
and the whole pipeline against the CPU oracle (tiled mode) on maps that hold every pass and every blend outcome."""
import numpy as np
import pytest

import oracle_lib
import replay

pytestmark = pytest.mark.gpu


def _cluster(rng, dim, n, scale):
    ext = scale * 2.0
    pos = rng.uniform(-ext, ext, (n, dim)).astype(np.float32)
    if dim == 3:
        pos[:, 2] = (0.2 * ext * np.sin(3 * pos[:, 0] / ext) * np.cos(2 * pos[:, 1] / ext)).astype(np.float32)
        nrm = np.stack([-0.3 * np.cos(3 * pos[:, 0] / ext), 0.2 * np.sin(2 * pos[:, 1] / ext), np.ones(n)], axis=1)
    else:
        pos[:, 1] = (0.2 * ext * np.sin(3 * pos[:, 0] / ext)).astype(np.float32)
        nrm = np.stack([-0.3 * np.cos(3 * pos[:, 0] / ext), np.ones(n)], axis=1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[: n // 5] = 0.0          # value-only points: derivative rows of every kind of tile
    P = np.zeros((9, n), dtype=np.float32)
    P[0:dim] = pos.T
    P[3:3 + dim] = nrm.T
    P[6] = -0.2
    P[7] = rng.uniform(1e-3, 5e-3, n)
    P[8] = rng.uniform(0.01, 0.1, n)
    return P


@pytest.mark.parametrize("dim,scale", [(3, 0.05), (2, 1.2)])
def test_column_layouts_match_the_full_layout(dim, scale):
    """Random subsets of queries through the value layout (32 per tile) and the gradient layout (10 per tile): the same bits per
    (query, component) as the 8 x 4 layout, in every K4 size class."""
    import gpismap_amd
    rng = np.random.default_rng(7 + dim)
    sizes = [12, 90, 200, 300, 600, 1200]
    st = gpismap_amd.OnGPIS(dim, scale, keep_factor=True)
    P = np.concatenate([_cluster(rng, dim, n, scale) for n in sizes], axis=1)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    models = st.train(P, off, np.arange(off[-1], dtype=np.int32))
    nq = 150
    xq = rng.uniform(-2 * scale, 2 * scale, (nq, dim)).astype(np.float32)
    jq, jm = [], []
    for m in models:
        sub = rng.choice(nq, size=int(rng.integers(1, nq)), replace=False)       # ragged tiles in every layout
        jq += list(sub); jm += [m] * sub.size
    jq, jm = np.array(jq, dtype=np.int32), np.array(jm, dtype=np.int32)
    full = st.eval(xq, jq, jm, layout=0)
    val = st.eval(xq, jq, jm, layout=1)
    grad = st.eval(xq, jq, jm, layout=2)
    u = lambda a: a.view(np.uint32)
    assert np.array_equal(u(val[:, [0, 4]]), u(full[:, [0, 4]]))
    g = [c for c in range(1, dim + 1)] + [4 + c for c in range(1, dim + 1)]
    assert np.array_equal(u(grad[:, g]), u(full[:, g]))
    # each layout leaves the other components' slots alone (zero here)
    assert not np.any(val[:, g]) and not np.any(grad[:, [0, 4]])


def _check_split(gm, om, grid, tag, two_candidate_jobs=True):
    rg, ro = gm.test(grid), om.test(grid)
    pj = gm.pass_jobs()
    st = gm.stats()
    print("%s: %d queries, jobs %s, evals %d" % (tag, grid.shape[0], pj, int(st["last_test_evals"])))
    assert rg.shape == ro.shape
    assert np.array_equal(rg.view(np.uint32), ro.view(np.uint32)), (tag, int(np.sum(np.any(rg != ro, axis=1))))
    # every pass ran; evaluations stay the reference's (query, candidate) pairs: pass 2b completes pass 2a's
    assert pj["pass1"] > 0 and pj["pass2a_value"] > 0 and pj["pass2b_grad"] > 0, pj
    assert pj["pass2_full"] > 0 or not two_candidate_jobs, pj
    assert pj["pass2b_grad"] <= pj["pass2a_value"]
    assert int(st["last_test_evals"]) == pj["pass1"] + pj["pass2_full"] + pj["pass2a_value"]


def test_split_on_the_bench_map_matches_oracle():
    """The benchmark's map (five synthetic frames) over a 32^3 sample of its query volume."""
    import gpismap_amd
    gm = gpismap_amd.GPisMap3()
    om = oracle_lib.OracleMap3()
    for f in range(5):
        d = replay.synthetic_depth(f)
        gm.update(d, replay.IDENTITY_POSE); om.update(d, replay.IDENTITY_POSE)
    _check_split(gm, om, replay.synthetic_grid(32), "bench map")


def test_split_on_the_3d_sequence_matches_oracle():
    """The bundled 3-D sequence after all 40 frames, on the demo grid."""
    import gpismap_amd
    frames = replay.load_bigbird()
    gm = gpismap_amd.GPisMap3(frames[0]["cam"])
    om = oracle_lib.OracleMap3(frames[0]["cam"])
    for i, fr in enumerate(frames[:40]):
        if i:
            gm.set_camera(fr["cam"]); om.set_camera(fr["cam"])
        gm.update(fr["depth"], fr["pose"]); om.update(fr["depth"], fr["pose"])
    _check_split(gm, om, replay.demo3_grid(), "3-D sequence frame 40")


def test_split_on_the_2d_sequence_matches_oracle():
    """The bundled 2-D laser sequence, on the demo grid."""
    import gpismap_amd
    gm = gpismap_amd.GPisMap()
    om = oracle_lib.OracleMap2()
    for fr in replay.load_gazebo():
        gm.update(fr["thetas"], fr["ranges"], fr["pose"]); om.update(fr["thetas"], fr["ranges"], fr["pose"])
    _check_split(gm, om, replay.demo2_grid(), "2-D sequence", two_candidate_jobs=False)   # (no query there has exactly two candidates)
