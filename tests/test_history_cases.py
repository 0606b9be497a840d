"""The sequences of tests/history_cases.py on the CPU, by the references alone: each has the property it is there for, so that
tests/test_gpu_handle_history.py cannot pass because a sequence never reached the branch.  Conditions, not measurements."""
import numpy as np

import history_cases as hc
import mppi_ref
from test_track_field_ref import field2, field3

CHUNK, BLOCK = 2048, 256                                 # csrc/cover.h: lattice points of a chunk, threads of a workgroup


def _sizes(seq, key):
    return [np.asarray(e[key]).shape[0] for e in seq]


def test_controller_tree_widths_and_columns():
    assert tuple(hc.mppi_segments(K) for _, K, _ in hc.CONTROLLER) == hc.CONTROLLER_P == (2, 4, 1, 32, 2)
    assert tuple(T * mppi_ref.ncontrols(dim) for dim, _, T in hc.CONTROLLER) == hc.CONTROLLER_COLUMNS == (66, 132, 2, 4, 66)
    assert hc.CONTROLLER[0] == hc.CONTROLLER[-1] and hc.CONTROLLER_SEEDS[0] == hc.CONTROLLER_SEEDS[-1]
    assert len(set(hc.CONTROLLER_SEEDS[:-1])) == len(hc.CONTROLLER) - 1
    (_, Ka, Ta), (_, Kb, Tb), (_, Kc, Tc) = hc.CONTROLLER[:3]
    assert Kb > Ka > Kc and Tb * 4 > Ta * 2 > Tc * 2 and {d for d, _, _ in hc.CONTROLLER} == {2, 3}
    # the larger entry leaves something other than zero in every array the smaller one after it reads back
    for r in hc.controller_ref(1):
        assert all(np.asarray(r[k]).any() for k in ("J", "q", "hits", "U", "nominal_states")), [k for k in r if not np.asarray(r[k]).any()]
        assert np.count_nonzero(r["J"][:Kc]) == Kc and np.count_nonzero(r["U"][:Tc]) > 0 and r["hits"][:Kc].any()


def test_controller_with_balls_and_a_footprint_grows_both_capacities():
    """The second controller sequence: every entry with balls has rollouts the balls hit, the plain entry reports none, and the
    per-rollout buffers of the balls have to grow under a K that init has served before (K of entry 4 == K of entry 3 > every K
    that stepped with balls before it)."""
    seq = hc.CONTROLLER_BODY
    assert seq[0] == seq[-1] and hc.CONTROLLER_BODY_SEEDS[0] == hc.CONTROLLER_BODY_SEEDS[-1] and {e[0] for e in seq} == {2, 3}
    assert seq[3][3:] == (0, 0) and seq[4][1] == seq[3][1] > max(e[1] for e in seq[:3]) and seq[4][3] > 0 and seq[4][4] > 0
    assert seq[1][1] > seq[0][1] > seq[2][1] and hc.mppi_segments(seq[2][1]) == 1 and seq[1][3] == 256 and seq[1][4] == 16
    for i, (dim, K, T, n, m) in enumerate(seq[:-1]):
        c = hc.controller_body_case(i)
        assert (c["obst"]["n"] if c["obst"] else 0) == n and (c["body"]["m"] if c["body"] else 0) == m
        for r in hc.controller_body_ref(i):
            if n:
                assert 0 < r["ndyn"] <= K and r["dyn_hits"].any() and np.isfinite(r["min_sep"]).all(), (i, r["ndyn"])
            else:
                assert r["ndyn"] == 0 and not r["dyn_hits"].any() and np.isposinf(r["min_sep"]).all(), i
            assert r["J"].size == K and r["U"].shape[0] == T


def test_filter_entries_resample_and_keep():
    dims = [d for d, _ in hc.FILTER]
    ms = [m for _, m in hc.FILTER]
    assert ms == [257, 4097, 1, 65, 300, 257] and dims == [2, 2, 2, 2, 3, 2] and hc.FILTER_SEEDS[0] == hc.FILTER_SEEDS[-1]
    for i, (dim, m) in enumerate(hc.FILTER[:-1]):
        steps = hc.filter_ref(i, field2() if dim == 2 else field3())
        resampled = [r for r, _ in steps]
        print("filter entry %d (dim %d, m %d): resampled %s" % (i, dim, m, resampled))
        assert any(resampled) == (m > 2)
        assert not resampled[1]                          # (resample_below 0: L is kept and read back)
        if i == 1:                                       # the largest: nothing it leaves is all zero where the next entry reads
            g = steps[1][1]
            assert all(g[k][:1].any() for k in ("state", "L", "q", "cost", "inliers")) and g["ancestors"].any()
            assert np.unique(g["ancestors"]).size < m


def test_coverage_entries():
    refs = [hc.coverage_ref(e, hc.ref_field(e["field"])[0]) for e in hc.COVERAGE[:3]]
    a, b, c = refs
    n = [r["seen"].size for r in refs]
    assert n[1] > n[0] > n[2] and n[1] > CHUNK
    fb = b["frontiers"]
    print("coverage: seen %s, frontier points %s, components %s, clusters %s"
          % ([int(r["seen"].sum()) for r in refs], [r["frontiers"]["points"].size for r in refs],
             [r["frontiers"]["clusters"] for r in refs], [r["frontiers"]["label"].size for r in refs]))
    assert fb["points"].size > BLOCK and fb["clusters"] >= 2 and fb["label"].size >= 2
    assert fb["points"].size > a["frontiers"]["points"].size > 0 and fb["label"].size > a["frontiers"]["label"].size > 0
    assert c["seen"].sum() == 0 and c["frontiers"]["points"].size == 0 and c["frontiers"]["clusters"] == 0
    # what B leaves in the mask's buffer is visible where C and the last A read: seen bytes among C's 63, and among A's 2400 where
    # A's own frame sees nothing
    assert b["seen"][:n[2]].any() and (b["seen"][:n[0]] & ~a["seen"]).any()
    assert 0 < a["seen"].sum() < n[0] and 0 < b["seen"].sum() < n[1]
    for k in ("points", "point_label", "label", "count", "sums", "box", "rep"):
        assert fb[k].any(), k
    assert np.isfinite(b["samples"][:, 0]).any() and np.isnan(b["samples"][-1, 0]) and np.isnan(c["samples"][-1, 0])
    assert np.isfinite(a["samples"][-4, 0])              # (the lattice's last point is inside)


def test_view_entries():
    outs = [hc.view_ref_call(e, hc.ref_field(e["field"])[0]) for e in hc.VIEW[:3]]
    (ga, ha, pa, ta, sa), (gb, hb, pb, tb, sb), (gc, hc_, pc, tc, sc) = outs
    print("view: targets %s, gain max %s, hits max %s, samples of the first pose %s" % ([ta, tb, tc], [ga.max(), gb.max(), gc.max()],
                                                                                      [ha.max(), hb.max(), hc_.max()], [sa, sb, sc]))
    assert _sizes(hc.VIEW, "poses") == [65, 3, 1, 65] and [p.shape[1] for p in (pa, pb, pc)] == [90, 91, 23]
    assert tc == 0 and gc.max() == 0
    for g, h, s, t in ((ga, ha, sa, ta), (gb, hb, sb, tb)):
        assert g.max() > 0 and h.max() > 0 and s > 0 and t > 0
    # the word after the gains of a smaller call lies inside the larger call's gains: what stands there must not be zero
    assert ga[3] > 0 and gb[1] > 0 and ha[:3].any() and hb[:1].any()
    assert [len(e["seen"]) for e in hc.VIEW[:3]] == [2400, 7680, 63]


def test_locator_tracker_renderer_entries():
    d2, d3 = field2(), field3()
    assert _sizes(hc.LOCATOR, "poses") == [300, 5000, 3, 1, 300]
    cost, inl, order = hc.locator_ref(hc.LOCATOR[1], d2)
    assert cost[:3].all() and inl[:3].any() and order.any() and order.size == 16
    pts = [hc.tracker_ref(e, d3 if e["dim"] == 3 else d2)["points"] for e in hc.TRACKER[:3]]
    print("tracker points per entry: %s" % pts)
    assert pts[0] > 2 * hc.SEGMENT and pts[1] > hc.SEGMENT > pts[2] > 0 and pts[0] > pts[1]
    first = hc.tracker_ref(hc.TRACKER[0], d3)
    assert first["inliers"] > 2 * hc.SEGMENT and first["H"].any() and first["b"].any() and np.isfinite(first["resid"]).sum() > 2 * hc.SEGMENT
    rays = []
    for e in hc.RENDERER[:4]:
        d, rec, st, stats = hc.renderer_ref(e, d3 if e["dim"] == 3 else d2)
        rays.append(d.size)
        if d.size >= 360:                                # the two larger entries
            assert (st == 0).sum() > 100 and np.isfinite(d).any() and rec[st == 0].any() and stats["samples"] > 0
    assert rays == [4800, 91, 360, 23] and [e["tiles"] for e in hc.RENDERER] == [True, False, True, True, True]


def test_dfield_sequence_and_session_fields():
    shapes = [hc.FIELDS[n][0]["shape"] for n in hc.DFIELD]
    assert shapes == [(60, 40), (24, 20, 16), (9, 7), (60, 40)]
    for name in hc.DFIELD[:3]:
        dist, site = hc.ref_field(name)
        if name == "tiny2":
            assert np.all(site == -1) and np.all(np.isinf(dist))          # the branch without a site
        else:
            assert (site >= 0).all() and (dist < 0).any() and (dist > 0).any()
    for names in (hc.SESSION2, hc.SESSION3):
        n = [int(np.prod(hc.FIELDS[k][0]["shape"])) for k in names]
        assert n[1] > n[0] > n[-1] or (len(n) == 2 and n[0] > n[1])
        for k in names:
            dist, _ = hc.ref_field(k)
            assert (dist < 0).any() and (dist > 0).any()
