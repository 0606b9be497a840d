"""K1 / K2 and the ObsGP host code against the float64 reference (obsgp_ref.py) at every partition edge: grid and scan sizes,
validity patterns, lookup boundaries and margins, launch shapes, the staging routes of update(), and one handle re-used
across sizes and modes.  Called through the C-ABI (gpismap_amd.ObsGP -> gpis_obsgp_*).

The bound (obsgp_ref.assess): error <= 8 x error(float32 LAPACK pipeline) + 4 ulp, both against float64 on the same operands.
Masks, group sizes, compacted inputs and everything "the same query in another batch / route / handle" are exact.

What fails where:
  wrong intended arithmetic (a term, the prior, exp)    every test through obsgp_ref.assess; controls in test_obsgp_ref.py
  ng = (n - 3) / 5 + 1, last tile 3 .. 7 wide           test_grid_shapes_small, test_grid_shapes_large
  grids narrower than one tile                          test_grid_shapes_small (ni, nj = 1, 2)
  the 1-D split of the last 20 .. 39 beams              test_scan_lengths; N < 20: test_scans_too_short_are_refused_and_query_needs_training
  re-partitioning on a live handle, ensure_groups /     test_one_handle_through_a_life
    cap_idx_ / cap_tab_ growth, stale tn
  `<` against vali[k], margins 0.005 / 0.0175, open     check_answers in every 2-D / 1-D test (queries on every table entry, one
    intervals, untrained tiles, val untouched / 1e6       ulp to either side, table ends +- margin +- 1 ulp; sentinel -7)
  ballot / popcount compaction, f = 0 / -1 / NaN        test_validity_patterns
  launch shapes, chunk loop, workgroups per group       test_launch_shapes_give_the_same_bits
  stage_q + query_staged, stage_qb + async + wait_b     test_staging_routes_give_the_same_bits, test_training_waits_for_a_pending_batch"""
import numpy as np
import pytest

import obsgp_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def _obsgp():
    import gpismap_amd
    return gpismap_amd.ObsGP()


def _status(exc):
    return int(str(exc.value).rsplit(" ", 1)[-1])


def check_partition(g, members, x_all, f, which=None):
    """num_groups, and per group n and the compacted inputs, exactly.  Returns the reference Groups (None: untrained) of `which`
    (default: all) and the device's (L, alpha) of them."""
    assert g.num_groups() == len(members)
    pick = set(range(len(members)) if which is None else which)
    groups, model = [None] * len(members), {}
    for t, m in enumerate(members):
        n, x, alpha, L = g.group(t)
        assert n == m.size, (t, n, m.size)
        if n == 0:
            continue
        np.testing.assert_array_equal(x[:n, :x_all.shape[1]], x_all[m])
        if t in pick:
            groups[t] = R.Group(x_all[m], f[m])
            model[t] = (L, alpha)
    return groups, model


def check_answers(tag, g, groups, model, which, gref, reach, q, worst):
    """Hit mask, the misses' sentinel and var = 1e6 exactly; the hits of the groups `which` and those groups' factor and alpha
    within the bound; every reachable trained group answered at least once."""
    val, var = g.query(q, val0=float(R.VAL0))
    hit = ~(var == R.MISS_VAR)
    np.testing.assert_array_equal(hit, gref >= 0, err_msg=tag)
    assert np.all(val[~hit] == R.VAL0) and np.all(var[~hit] == R.MISS_VAR), tag
    fin = ~np.isnan(q.reshape(len(gref), -1)).any(axis=1)
    answered = np.unique(gref[(gref >= 0) & fin])
    missing = np.setdiff1d(np.flatnonzero(reach), answered)
    assert missing.size == 0, (tag, "reachable trained groups without an answered query", missing[:8])
    R.assess_answers(groups, gref, q, val, var, which, worst, tag, model=lambda t: model[t])
    return val, var


def run2d(tag, ni, nj, worst, pattern="all", kind="smooth", g=None, **lat):
    vu = R.lattice(ni, nj, **lat)
    part = R.partition2d(vu, ni, nj)
    for tab, size in ((part.vali, ni), (part.valj, nj)):
        if size > 1:              # (a one-pixel axis has both table entries on the same pixel: its cell is swallowed whole)
            assert np.diff(tab.astype(np.float64)).min() > float(R.MARGIN2), (tag, "a boundary pair inside the margin")
    f = R.validity(pattern, part, R.field2d(vu, kind), seed=ni + nj)
    g = g or _obsgp()
    g.train2d(vu, f, ni, nj)
    px = vu.reshape(-1, 2)
    members = part.members(f)
    which = R.assessed_groups(part.ngroups, part.ng0)
    groups, model = check_partition(g, members, px, f, which)
    trained = np.array([m.size > 0 for m in members])
    r = part.reachable()
    assert r.reshape(part.ng1, part.ng0)[:-1, :-1].all(), tag        # at most the last row and the last column are unreachable
    q = R.queries2d(part, vu, seed=ni + 3 * nj)
    gref = R.lookup2d(part, trained, q)
    check_answers(tag, g, groups, model, [t for t in which if trained[t]], gref, r & trained, q, worst)
    return part, members, groups


def _verdict(title, worst):
    print("\n%s: %s" % (title, worst))
    assert worst.rows, title
    assert not worst.bad, worst.bad[:6]


# ------------------------------------------------------------------------------------------------------------- a. grid shapes
@pytest.mark.parametrize("nj", (1, 3, 7, 8, 12, 13))
def test_grid_shapes_small(nj):
    """ng = (n - 3) / 5 + 1 with a last tile of 3 to 7 pixels for every n mod 5, and grids narrower than one tile."""
    worst = R.Worst()
    for ni in range(1, 19):
        part, members, _ = run2d("%dx%d" % (ni, nj), ni, nj, worst, kind="step" if (ni + nj) % 2 else "smooth")
        assert part.ng0 == max(1, (ni - 3) // 5 + 1) and 1 <= part.i1[-1] - part.i0[-1] + 1 <= 7
        assert all(1 <= m.size <= 64 for m in members)
    _verdict("grids 1..18 x %d" % nj, worst)


@pytest.mark.parametrize("ni,nj", R.GRIDS_BIG)
def test_grid_shapes_large(ni, nj):
    worst = R.Worst()
    part, members, _ = run2d("%dx%d" % (ni, nj), ni, nj, worst)
    assert sum(m.size == 64 for m in members) >= (part.ng0 - 1) * (part.ng1 - 1)
    _verdict("grid %d x %d" % (ni, nj), worst)


def test_grid_non_square_pitch_and_non_uniform_pitch():
    worst = R.Worst()
    run2d("23x9", *R.GRID_NONSQUARE, worst, pitch=(0.03, 0.008))
    run2d("17x13w", *R.GRID_WARPED, worst, warp=0.3, kind="step")
    _verdict("non-square and non-uniform lattices", worst)


# -------------------------------------------------------------------------------------------------------- b. validity patterns
@pytest.mark.parametrize("pattern", R.VALIDITY)
def test_validity_patterns(pattern):
    """The ballot / popcount compaction of K1: full tiles, holes in random patterns, empty tiles, one pixel per tile, a
    checkerboard, and f = 0 / -1 / NaN (all invalid by f > 0)."""
    worst = R.Worst()
    for ni, nj in ((14, 12), (64, 48)):
        part, members, _ = run2d("%s/%dx%d" % (pattern, ni, nj), ni, nj, worst, pattern=pattern)
        sizes = np.array([m.size for m in members])
        if pattern == "all":
            assert (sizes.reshape(part.ng1, part.ng0)[:-1, :-1] == 64).all()
        elif pattern == "one":
            assert (sizes == 1).all()
        elif pattern == "tiles":
            assert ni < 64 or ((sizes == 0).any() and (sizes == 64).any())
        elif pattern == "checker":
            assert sizes.max() == 32
        else:
            assert sizes.min() < sizes.max() < 64 or pattern == "holes10"
    _verdict("validity %s" % pattern, worst)


# ------------------------------------------------------------------------------------------------------------------- d. 1-D
def run1d(tag, theta, worst, kind="smooth", g=None):
    part = R.partition1d(theta)
    f = R.field1d(theta, kind)
    g = g or _obsgp()
    g.train1d(theta, f)
    members = part.members()
    got = [g.group(t)[0] for t in range(g.num_groups())]
    assert got == list(part.length), (tag, got)
    groups, model = check_partition(g, members, theta.reshape(-1, 1), f)
    for t, m in enumerate(members):
        assert m[0] == part.start[t]
    q = R.queries1d(part, theta, seed=theta.size)
    trained = np.ones(part.ngroups, dtype=bool)
    gref = R.lookup1d(part, trained, q)
    assert (gref[np.isin(q, part.range)] == -1).all()                  # a boundary belongs to no group
    check_answers(tag, g, groups, model, range(part.ngroups), gref, part.reachable(), q, worst)
    return part


def test_scan_lengths():
    """The rule that splits the last 20 to 39 beams into two groups, for every remainder; strict open intervals and the
    0.0175 margin."""
    worst = R.Worst()
    for N in R.N_1D:
        part = run1d("N%d" % N, R.scan(N), worst, "step" if N % 2 else "smooth")
        assert part.ngroups == N // 20 + 1 and part.start[-1] + part.length[-1] == N
    run1d("N271w", R.scan(271, warp=0.3), worst)
    run1d("N64coarse", R.scan(64, pitch=0.0175), worst)
    _verdict("1-D scans", worst)


def test_scans_too_short_are_refused_and_query_needs_training():
    import gpismap_amd
    g = _obsgp()
    with pytest.raises(gpismap_amd.GpisError) as e:
        g.query(np.zeros(4, dtype=F32))
    assert _status(e) == -3                                            # GPIS_ERR_STATE
    for route in (1, 2):
        with pytest.raises(gpismap_amd.GpisError) as e:
            g.query_route(route, np.zeros(4, dtype=F32))
        assert _status(e) == -3
    for N in (19, 1):
        with pytest.raises(gpismap_amd.GpisError) as e:
            g.train1d(R.scan(N), R.field1d(R.scan(N)))
        assert _status(e) == -1                                        # GPIS_ERR_ARG
        with pytest.raises(gpismap_amd.GpisError) as e:
            g.query(np.zeros(4, dtype=F32))
        assert _status(e) == -3
    g.train1d(R.scan(20), R.field1d(R.scan(20)))
    assert g.num_groups() == 2
    with pytest.raises(gpismap_amd.GpisError) as e:                    # a refused training leaves no model behind
        g.train1d(R.scan(19), R.field1d(R.scan(19)))
    with pytest.raises(gpismap_amd.GpisError) as e:
        g.query(np.zeros(4, dtype=F32))
    assert _status(e) == -3


# ------------------------------------------------------------------------------------------------- e. one handle through a life
def _snapshot(g, q, stride):
    ng = g.num_groups()
    out = [ng]
    for t in sorted(set(range(0, ng, stride)) | {ng - 1}):
        n, x, alpha, L = g.group(t)
        out.append((n, x[:n].copy(), alpha[:n].copy(), np.tril(L[:n, :n])))
    out.append(g.query(q, val0=float(R.VAL0)))
    return out


def _same(a, b, tag):
    assert a[0] == b[0], tag
    for ga, gb in zip(a[1:-1], b[1:-1]):
        assert ga[0] == gb[0], tag
        for xa, xb in zip(ga[1:], gb[1:]):
            np.testing.assert_array_equal(xa, xb, err_msg=tag)
    np.testing.assert_array_equal(a[-1][0], b[-1][0], err_msg=tag)
    np.testing.assert_array_equal(a[-1][1], b[-1][1], err_msg=tag)


def test_one_handle_through_a_life():
    """train2d(12 x 8) -> train2d(640 x 480) -> train1d(270) -> train2d(12 x 8), another f -> train1d(45) on one handle: after
    every step the groups and the answers are the bits of a fresh handle given only that step (stale tn entries of the
    12 288-group step, the tables' growth and reuse, re-partitioning after a mode change)."""
    steps = [("2d", 12, 8, "smooth", "all"), ("2d", 640, 480, "smooth", "holes10"), ("1d", 270, 0, "smooth", None),
             ("2d", 12, 8, "step", "holes10"), ("1d", 45, 0, "step", None)]
    live = _obsgp()
    for k, (mode, a, b, kind, pattern) in enumerate(steps):
        fresh = _obsgp()
        if mode == "2d":
            vu = R.lattice(a, b)
            part = R.partition2d(vu, a, b)
            f = R.validity(pattern, part, R.field2d(vu, kind), seed=k)
            q = R.queries2d(part, vu, seed=k)
            for h in (live, fresh):
                h.train2d(vu, f, a, b)
            assert live.num_groups() == part.ngroups
        else:
            theta = R.scan(a)
            part = R.partition1d(theta)
            f = R.field1d(theta, kind)
            q = R.queries1d(part, theta, seed=k)
            for h in (live, fresh):
                h.train1d(theta, f)
            assert live.num_groups() == part.ngroups
        _same(_snapshot(live, q, 7), _snapshot(fresh, q, 7), "step %d" % k)
        fresh.close()


# ----------------------------------------------------------------------------------------------- f / g. launch shapes and routes
@pytest.fixture(scope="module")
def big():
    """One trained 640 x 480 configuration, a pool U of queries with their group by the reference lookup, and U's answers from
    batches of 64 queries."""
    ni, nj = 640, 480
    vu = R.lattice(ni, nj)
    part = R.partition2d(vu, ni, nj)
    f = R.validity("holes10", part, R.field2d(vu), seed=1)
    g = _obsgp()
    g.train2d(vu, f, ni, nj)
    trained = np.array([m.size > 0 for m in part.members(f)])
    rng = np.random.default_rng(17)
    allq = R.queries2d(part, vu, seed=9)
    G = 37 * part.ng0 + 41                                              # the chosen group: 300 extra queries inside its cell
    n_, m_ = G % part.ng0, G // part.ng0
    cell = np.stack([rng.uniform(part.vali[n_], part.vali[n_ + 1], 300), rng.uniform(part.valj[m_], part.valj[m_ + 1], 300)], axis=1)
    outside = np.stack([rng.uniform(part.vali[-1], part.vali[-1] + 1.0, 2000), rng.uniform(-1.0, 1.0, 2000)], axis=1)
    U = np.ascontiguousarray(np.concatenate([allq[rng.choice(allq.shape[0], 20000, replace=False)], cell, outside]), dtype=F32)
    U = U[~np.isnan(U).any(axis=1)]                                    # (NaN answers do not compare equal; their bits are checked in 3c)
    gref = R.lookup2d(part, trained, U)
    assert (gref == G).sum() >= 257 and (gref < 0).sum() > 1000
    val = np.empty(U.shape[0], dtype=F32); var = np.empty(U.shape[0], dtype=F32)
    for s in range(0, U.shape[0], 64):
        val[s:s + 64], var[s:s + 64] = g.query(U[s:s + 64], val0=0.0)
    np.testing.assert_array_equal(~(var == R.MISS_VAR), gref >= 0)
    assert np.all(val[gref < 0] == 0)
    return dict(g=g, part=part, U=U, gref=gref, val=val, var=var, G=G)


def _chunks(nq, ngroups):
    """Workgroups per group of the sorted launch (obsgp_launch_query_binned), to place batches on both sides of each switch."""
    return max(1, min(4, (3 * nq // max(1, ngroups) + 127) // 128))


def launch_batches(big):
    """Index lists into U: (name, idx)."""
    rng, gref, G = np.random.default_rng(23), big["gref"], big["G"]
    nU, ng = big["U"].shape[0], big["part"].ngroups
    out = [("n%d" % n, rng.choice(nU, n, replace=n > nU)) for n in (0, 1, 63, 64, 65, 4095, 4096, 4097)]
    inG, rest = np.flatnonzero(gref == G), np.flatnonzero(gref != G)
    for k in (0, 1, 64, 65, 257):
        idx = np.concatenate([inG[:k], rng.choice(rest, 8192 - k)])
        out.append(("G=%d" % k, rng.permutation(idx)))
    out.append(("miss5000", rng.choice(np.flatnonzero(gref < 0), 5000)))
    for c in (2, 3, 4):
        t = next(n for n in range((128 * c - 127) * ng // 3 - 64, (128 * c - 127) * ng // 3 + 64) if _chunks(n, ng) == c)
        assert _chunks(t - 1, ng) == c - 1
        out.append(("chunks%d-" % c, rng.choice(nU, t - 1)))
        out.append(("chunks%d" % c, rng.choice(nU, t)))
    return out


def test_launch_shapes_give_the_same_bits(big):
    """The unsorted kernel at 0 / 1 / 63 / 64 / 65 queries and up to 4095, the sorted path from 4096, one group holding 0, 1,
    64, 65 or 257 queries of a sorted batch (the chunk loop), a batch of misses only, and both sides of every workgroups-per-group
    switch: every answer equals the same query's answer from a batch of 64."""
    g, U = big["g"], big["U"]
    for name, idx in launch_batches(big):
        val, var = g.query(np.ascontiguousarray(U[idx]).reshape(-1, 2), val0=0.0)
        np.testing.assert_array_equal(val, big["val"][idx], err_msg=name)
        np.testing.assert_array_equal(var, big["var"][idx], err_msg=name)
        if name == "miss5000":
            val, var = g.query(np.ascontiguousarray(U[idx]), val0=float(R.VAL0))
            assert np.all(val == R.VAL0) and np.all(var == R.MISS_VAR)


@pytest.mark.parametrize("route", (1, 2))
def test_staging_routes_give_the_same_bits(big, route):
    """stage_q + query_staged (the kernel on the page-locked staging below 4096 queries, copies from 4096) and stage_qb +
    query_staged_b_async + wait_b: the bits of query() started from val = 0, the misses' val = 0 and var = 1e6 included.  Every
    batch of the launch-shape test goes through, up to the 1.6 M queries of four workgroups per group (the routes' own sort
    scratch and the growth of their staging)."""
    g, U = big["g"], big["U"]
    names = []
    for name, idx in launch_batches(big):
        names.append(name)
        val, var = g.query_route(route, np.ascontiguousarray(U[idx]).reshape(-1, 2), val0=float(R.VAL0))
        np.testing.assert_array_equal(val, big["val"][idx], err_msg=name)
        np.testing.assert_array_equal(var, big["var"][idx], err_msg=name)
        miss = big["gref"][idx] < 0
        assert np.all(val[miss] == 0) and np.all(var[miss] == R.MISS_VAR), name
    assert {"n0", "n4095", "n4096", "G=257", "miss5000", "chunks2", "chunks3", "chunks4-", "chunks4"} <= set(names)
    v0, r0 = g.query_route(0, np.ascontiguousarray(U[:100]), val0=float(R.VAL0))     # route 0 is query(): the sentinel stays
    np.testing.assert_array_equal(r0, big["var"][:100])
    assert np.all(v0[big["gref"][:100] < 0] == R.VAL0)


@pytest.mark.parametrize("retrain", ("train2d", "train1d"))
def test_training_waits_for_a_pending_batch(retrain):
    """A batch of the second staging set runs on a stream of its own; a training issued while it is pending rewrites the groups
    it reads, so both trainings wait for it first.  Deterministic part: the handle reports the batch pending after it was issued and
    collected once the training call returns.  On top: the batch's answers are those of the model it was issued against."""
    ni, nj = 321, 243
    vu = R.lattice(ni, nj)
    f = R.field2d(vu)
    g = _obsgp()
    g.train2d(vu, f, ni, nj)
    rng = np.random.default_rng(5)
    px = vu.reshape(-1, 2)
    q = np.ascontiguousarray(np.tile(px, (8, 1)) + rng.uniform(-0.002, 0.002, (8 * px.shape[0], 2)).astype(F32), dtype=F32)
    want = g.query(q, val0=0.0)
    assert (~(want[1] == R.MISS_VAR)).sum() > 400000
    assert not g.pending()
    for _ in range(3):
        n = g.query_begin_b(q)
        assert g.pending()
        if retrain == "train2d":
            g.train2d(vu, R.field2d(vu, "step") * F32(3), ni, nj)
        else:
            theta = R.scan(1081)
            g.train1d(theta, R.field1d(theta, "step"))
        assert not g.pending(), "the training call returned with the batch still pending"
        val, var = g.query_end_b(n)
        np.testing.assert_array_equal(val, want[0])
        np.testing.assert_array_equal(var, want[1])
        g.train2d(vu, f, ni, nj)


def test_collecting_a_batch_needs_the_batch():
    """Route 4 copies exactly the batch route 3 left behind: none pending is GPIS_ERR_STATE, another size GPIS_ERR_ARG (it would
    read past the staging), and a collected batch is gone."""
    import gpismap_amd
    vu = R.lattice(18, 13)
    g = _obsgp()
    g.train2d(vu, R.field2d(vu), 18, 13)
    q = np.ascontiguousarray(vu.reshape(-1, 2))
    with pytest.raises(gpismap_amd.GpisError) as e:
        g.query_end_b(q.shape[0])
    assert _status(e) == -3
    g.query_route(2, q)                                                # a whole route 2 leaves nothing to collect either
    with pytest.raises(gpismap_amd.GpisError) as e:
        g.query_end_b(q.shape[0])
    assert _status(e) == -3
    n = g.query_begin_b(q)
    for wrong in (n + 1, 100000, n - 1):
        with pytest.raises(gpismap_amd.GpisError) as e:
            g.query_end_b(wrong)
        assert _status(e) == -1
    val, var = g.query_end_b(n)
    want = g.query(q, val0=0.0)
    np.testing.assert_array_equal(val, want[0]); np.testing.assert_array_equal(var, want[1])
    with pytest.raises(gpismap_amd.GpisError) as e:
        g.query_end_b(n)
    assert _status(e) == -3
