"""A plain reference of K5, the driver of test(): cluster lookup, candidate order, gate and blend.

Written from the reference's sources (GPisMap3.cpp:794-902, GPisMap.cpp:665-763, octree.cpp:861-893 / octree.h:64-69,128-135,
quadtree.cpp / quadtree.h) and their restatement in oracle/map3.hpp, map2.hpp and tree.hpp -- not from the kernels.  float32
throughout (numpy float32 operations round once each and never fuse).  The candidate order is libstdc++'s std::sort itself
(oracle_lib.sort_perm), not an emulation of it.

A table is a dict: dim, c / lo / hi [ncl, 3] float32 (cells in traversal order; third column 0 in 2-D), model [ncl] (opaque id
or -1), parent [ncl] (first ancestor or -1), anc_lo / anc_hi [nanc, 3], anc_parent [nanc] (parents come first), pitch.

The keyword switches of lookup_ref / blend_ref select DEFECTIVE variants; they exist for the negative controls only.
"""
import numpy as np

import oracle_lib

F = np.float32


# ------------------------------------------------------------------------------------------------ lookup ----
def _box_hit(qlo, qhi, lo, hi, dim, exclusive):
    """[nq, nb]: the query box intersects the box -- AABB3::intersectsAABB octree.h:128-135, inclusive."""
    ok = np.ones((qlo.shape[0], lo.shape[0]), dtype=bool)
    for d in range(dim):
        if exclusive:
            ok &= ~((qhi[:, d, None] <= lo[None, :, d]) | (qlo[:, d, None] >= hi[None, :, d]))
        else:
            ok &= ~((qhi[:, d, None] < lo[None, :, d]) | (qlo[:, d, None] > hi[None, :, d]))
    return ok


def lookup_ref(table, x, search_half, stable_sort=False, exclusive_box=False, no_ancestors=False, max_keep=3):
    """The candidates of each query: cells whose box and whose every ancestor's box intersect the query box x -+ half, in
    traversal order, then ordered by std::sort on the squared centre distance.

    Returns a dict: count [n] (all candidates), ncand = min(count, 3), cand [3, n] (model ids, -1 beyond ncand), cell [3, n]
    (table indices, -1 beyond), tie [n] (an exact distance tie among the up to four nearest: the oracle's flag bit 1),
    unstable [n] (std::sort and a stable sort differ in the first three), pruned [n] (cells whose own box passes and an
    ancestor's fails)."""
    dim = table["dim"]
    x = np.ascontiguousarray(x, dtype=F).reshape(-1, dim)
    n = x.shape[0]
    half = F(search_half)
    qlo, qhi = (x - half).astype(F), (x + half).astype(F)          # AABB3 ctor, octree.h:64-69
    c, lo, hi = table["c"], table["lo"], table["hi"]
    ncl = c.shape[0]
    parent, ap = table["parent"], table["anc_parent"]
    nanc = ap.size
    qi_all, ci_all, pruned = [], [], np.zeros(n, dtype=np.int64)
    step = max(1, (1 << 24) // max(ncl, 1))
    for s in range(0, n, step):
        e = min(n, s + step)
        own = _box_hit(qlo[s:e], qhi[s:e], lo, hi, dim, exclusive_box) if ncl else np.zeros((e - s, 0), dtype=bool)
        ok = own
        if nanc and ncl and not no_ancestors:
            # the walk reaches a cell only through every node above it (octree.cpp:864-866)
            aok = _box_hit(qlo[s:e], qhi[s:e], table["anc_lo"], table["anc_hi"], dim, exclusive_box)
            for a in range(nanc):
                if ap[a] >= 0:
                    aok[:, a] &= aok[:, ap[a]]
            chain = np.ones((e - s, ncl), dtype=bool)
            hasp = parent >= 0
            chain[:, hasp] = aok[:, parent[hasp]]
            ok = own & chain
            pruned[s:e] = (own & ~chain).sum(axis=1)
        qi, ci = np.nonzero(ok)                # row-major: by query, then by cell index = traversal order
        qi_all.append(qi + s); ci_all.append(ci)
    qi = np.concatenate(qi_all) if qi_all else np.zeros(0, dtype=np.int64)
    ci = np.concatenate(ci_all) if ci_all else np.zeros(0, dtype=np.int64)
    count = np.bincount(qi, minlength=n).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    # squared distance box.c - range.c, octree.cpp:24-31: dx*dx, + dy*dy, + dz*dz
    d = (c[ci, :dim] - x[qi]).astype(F)
    key = (d[:, 0] * d[:, 0]).astype(F)
    for k in range(1, dim):
        key = (key + (d[:, k] * d[:, k]).astype(F)).astype(F)
    local = np.arange(qi.size, dtype=np.int64) - off[qi]
    stable = (np.lexsort((local, key, qi)) - off[qi]).astype(np.int64)       # positions within each query, (key, traversal) order
    perm = stable if stable_sort else oracle_lib.sort_perm(key, off).astype(np.int64)
    keep = max_keep
    cell = np.full((keep, n), -1, dtype=np.int64)
    first_std = np.full((4, n), -1, dtype=np.int64)
    first_stb = np.full((3, n), -1, dtype=np.int64)
    for k in range(4):
        m = count > k
        g = off[:-1][m] + perm[off[:-1][m] + k]
        first_std[k, m] = g
        if k < keep:
            cell[k, m] = ci[g]
        if k < 3:
            first_stb[k, m] = off[:-1][m] + stable[off[:-1][m] + k]
    for k in range(4, keep):
        m = count > k
        cell[k, m] = ci[off[:-1][m] + perm[off[:-1][m] + k]]
    tie = np.zeros(n, dtype=bool)
    for k in range(1, 4):
        m = count > k
        tie[m] |= key[first_std[k, m]] == key[first_std[k - 1, m]]
    unstable = (first_std[:3] != first_stb).any(axis=0)
    ncand = np.minimum(count, 3).astype(np.int32)
    model = table["model"]
    cand = np.where(cell[:3] >= 0, model[np.maximum(cell[:3], 0)] if ncl else -1, -1).astype(np.int32)
    return dict(count=count, ncand=ncand, cand=cand, cell=cell, tie=tie, unstable=unstable, pruned=pruned)


# ------------------------------------------------------------------------------------------------- blend ----
BRANCH_NAMES = {0: "none", 1: "one", 2: "gate-closed", 3: "2:pick0", 4: "2:pick1", 5: "2:blend01", 6: "2:blend10"}
_PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
for _i, _p in enumerate(_PERMS):
    BRANCH_NAMES[10 + _i] = "3:pick%d%d%d" % _p
    BRANCH_NAMES[20 + _i] = "3:blend%d%d%d" % _p
ALL_BRANCHES = sorted(BRANCH_NAMES)
# (a pick of candidate 1 cannot happen: the gate let the query through because that variance exceeds the threshold)
REACHABLE = [BRANCH_NAMES[b] for b in ALL_BRANCHES if b not in (3, 10, 11)]


def _insertion_sort(idx, less):
    """libstdc++ std::sort on at most 16 elements: __insertion_sort (bits/stl_algo.h)."""
    for i in range(1, len(idx)):
        v = idx[i]
        if less(v, idx[0]):
            idx[1:i + 1] = idx[0:i]
            idx[0] = v
        else:
            j = i
            while less(v, idx[j - 1]):
                idx[j] = idx[j - 1]
                j -= 1
            idx[j] = v
    return idx


def blend_ref(ncand, cand, rec, prefill, var_thre, prior_var, dim, gate_ge=False, swap_weights=False, pairs=None):
    """test_one after the lookup, in float32.  ncand [n]; cand [3, n] model ids (-1: the cell has no GP); rec [n, 3, 8] the
    record (mean 4, variances 4; 2-D 3 + 3) of each candidate that has a model; prefill [n, 2(1+dim)] the result array as the
    caller hands it in.

    A candidate without a model (the reference dereferences a null GP there): the first leaves the pre-filled record and the
    prior variance; the second / third contribute mean 0, gradient 0, value variance = prior, gradient variances 0.

    Returns (res, branch [n], jobs [4]): jobs = K4 evaluations of pass 1, pass 2 (two-candidate queries, all columns), 2a
    (three-candidate queries: value column of candidates 2 and 3), 2b (gradient columns of those the blend reads).
    pairs: a list that receives, per pass, the (query, candidate position) pairs evaluated, as an [njobs, 2] array."""
    NC = 1 + dim
    n = ncand.size
    thre, prior = F(var_thre), F(prior_var)
    res = np.array(prefill, dtype=F, copy=True).reshape(n, 2 * NC)
    rec = np.asarray(rec, dtype=F).reshape(n, 3, 8)
    branch = np.zeros(n, dtype=np.int32)
    jobs = [0, 0, 0, 0]
    res[:, NC] = prior                                         # GPisMap3.cpp:816
    has = (cand >= 0) & (np.arange(3)[:, None] < ncand[None, :])
    first = has[0]
    jobs[0] = int(first.sum())
    pl = [[(int(q), 0) for q in np.nonzero(first)[0]], [], [], []]
    res[first, :NC] = rec[first, 0, :NC]
    res[first, NC:] = rec[first, 0, 4:4 + NC]
    branch[ncand == 1] = 1
    multi = ncand >= 2
    v0 = res[:, NC]
    gate = multi & ((v0 >= thre) if gate_ge else (v0 > thre))
    branch[multi & ~gate] = 2
    with np.errstate(all="ignore"):
        for q in np.nonzero(gate)[0]:
            nc = int(ncand[q])
            f2 = np.zeros((3, NC), dtype=F); v2 = np.zeros((3, NC), dtype=F)
            f2[0] = res[q, :NC]; v2[0] = res[q, NC:]
            for s in range(1, nc):
                if has[s, q]:
                    f2[s] = rec[q, s, :NC]; v2[s] = rec[q, s, 4:4 + NC]
                else:
                    v2[s, 0] = prior
            if nc == 2:
                jobs[1] += int(has[1, q])
                pl[1] += [(int(q), 1)] * int(has[1, q])
            else:
                jobs[2] += int(has[1, q]) + int(has[2, q])
                pl[2] += [(int(q), s) for s in (1, 2) if has[s, q]]
            id2 = _insertion_sort(list(range(nc)), lambda a, b: v2[a, 0] < v2[b, 0])
            b0 = id2[0]
            read = [b0]
            if v2[b0, 0] < thre:
                res[q, :NC] = f2[b0]; res[q, NC:] = v2[b0]
                branch[q] = (3 + b0) if nc == 2 else 10 + _PERMS.index(tuple(id2))
            else:
                b1 = id2[1]
                read.append(b1)
                w1, w2 = F(v2[b0, 0] - thre), F(v2[b1, 0] - thre)
                if swap_weights:
                    w1, w2 = w2, w1
                w12 = F(w1 + w2)
                res[q, :NC] = ((w2 * f2[b0]).astype(F) + (w1 * f2[b1]).astype(F)).astype(F) / w12
                res[q, NC:] = ((w2 * v2[b0]).astype(F) + (w1 * v2[b1]).astype(F)).astype(F) / w12
                branch[q] = (5 + b0) if nc == 2 else 20 + _PERMS.index(tuple(id2))
            if nc == 3:
                jobs[3] += sum(1 for b in read if b >= 1 and has[b, q])
                pl[3] += [(int(q), b) for b in read if b >= 1 and has[b, q]]
    if pairs is not None:
        pairs[:] = [np.array(p, dtype=np.int64).reshape(-1, 2) for p in pl]
    return res, branch, jobs


def branch_histogram(branch):
    return {BRANCH_NAMES[b]: int((branch == b).sum()) for b in ALL_BRANCHES}


# -------------------------------------------------------------------------------------- synthetic tables ----
def build_table(dim, levels, occupied, cluster_half, root_c):
    """A genuine power-of-two hierarchy as the reference's tree builds it (octree.cpp:33-51, 670-712 / quadtree.cpp): root
    box of half cluster_half * 2^levels at root_c; child centres c -+ l with l = float32(double(h) / 2), child order NW(F),
    NE(F), SW(F), SE(F) [, NWB .. SEB] (bit 0 -> +x, bit 1 -> -y, bit 2 -> -z); every box is float32(c -+ h), rounded on its
    own.  occupied(ijk) says whether the cluster cell at integer lattice coordinates ijk (0 .. 2^levels - 1 per axis, x to the
    right, y and z up) is in the table.  Cells come out in traversal order; only nodes above a cell are kept as ancestors.
    Adds ijk [ncl, 3] and pitch to the table."""
    side = 1 << levels
    occ = np.zeros((side,) * dim, dtype=bool)
    for idx in np.ndindex(*occ.shape):
        occ[idx] = bool(occupied(idx))
    cells, parents, ancs, anc_parents, ijks = [], [], [], [], []

    def any_below(i0, size):
        sl = tuple(slice(i0[d], i0[d] + size) for d in range(dim))
        return occ[sl].any()

    def walk(c, h, lev, i0, up):
        size = 1 << lev
        if not any_below(i0, size):
            return
        c = np.asarray(c, dtype=F)
        box = ((c - F(h)).astype(F), (c + F(h)).astype(F))
        if lev == 0:
            cells.append((c, box)); parents.append(up); ijks.append(tuple(i0))
            return
        ancs.append(box); anc_parents.append(up)
        me = len(ancs) - 1
        l = F(np.float64(h) * 0.5)
        hs = size // 2
        for i in range(1 << dim):
            cc = c.copy(); j0 = list(i0)
            cc[0] = c[0] + l if (i & 1) else c[0] - l
            j0[0] += hs if (i & 1) else 0
            cc[1] = c[1] - l if (i & 2) else c[1] + l
            j0[1] += 0 if (i & 2) else hs
            if dim == 3:
                cc[2] = c[2] - l if (i & 4) else c[2] + l
                j0[2] += 0 if (i & 4) else hs
            walk(cc, l, lev - 1, j0, me)

    walk(np.asarray(root_c, dtype=F)[:dim], F(F(cluster_half) * F(side)), levels, [0] * dim, -1)
    ncl, nanc = len(cells), len(ancs)
    pad = lambda v: np.concatenate([v, np.zeros(3 - dim, dtype=F)])
    T = dict(dim=dim, pitch=2.0 * float(F(cluster_half)),
             c=np.array([pad(c) for c, _ in cells], dtype=F).reshape(ncl, 3),
             lo=np.array([pad(b[0]) for _, b in cells], dtype=F).reshape(ncl, 3),
             hi=np.array([pad(b[1]) for _, b in cells], dtype=F).reshape(ncl, 3),
             model=np.arange(ncl, dtype=np.int32), parent=np.array(parents, dtype=np.int32).reshape(ncl),
             anc_lo=np.array([pad(b[0]) for b in ancs], dtype=F).reshape(nanc, 3),
             anc_hi=np.array([pad(b[1]) for b in ancs], dtype=F).reshape(nanc, 3),
             anc_parent=np.array(anc_parents, dtype=np.int32).reshape(nanc),
             ijk=np.array(ijks, dtype=np.int64).reshape(ncl, dim))
    return T


def x_for_qlo(target, half):
    """A float32 x with float32(x - half) == target exactly (None if there is none nearby)."""
    half = F(half)
    x = F(F(target) + half)
    for _ in range(8):
        r = F(x - half)
        if r == F(target):
            return x
        x = np.nextafter(x, F(np.inf) if r < target else F(-np.inf), dtype=F)
    return None


def x_for_qhi(target, half):
    half = F(half)
    x = F(F(target) - half)
    for _ in range(8):
        r = F(x + half)
        if r == F(target):
            return x
        x = np.nextafter(x, F(np.inf) if r < target else F(-np.inf), dtype=F)
    return None


def craft_ancestor(table, cell, half, axis=0):
    """Lower the first ancestor's hi of `cell` along `axis` to one ulp below the cell's own hi and return a query whose qlo on
    that axis equals the cell's hi: the cell's box passes (inclusive), the ancestor's fails.  Changes the table in place; None
    (table untouched) when float32 has no such query for this cell."""
    a = int(table["parent"][cell])
    h = table["hi"][cell, axis]
    xa = x_for_qlo(h, half)
    if a < 0 or xa is None:          # (no float32 x gives that qlo: the caller tries another cell)
        return None
    table["anc_hi"][a, axis] = np.nextafter(h, F(-np.inf), dtype=F)
    x = table["c"][cell, :table["dim"]].copy()
    x[axis] = xa
    return x


def queries_aligned(table, rng, n):
    """Lattice-aligned queries: cell centres, face centres, edge midpoints and corners of the cells (float32 sums of a centre
    and multiples of the cell half, as a caller's own grid arithmetic gives them)."""
    dim = table["dim"]
    ch = F(table["pitch"] / 2.0)
    ci = rng.integers(0, table["c"].shape[0], n)
    k = rng.integers(-5, 6, (n, dim)).astype(F)       # steps of one cell half: -2.5 .. 2.5 cells around a centre
    return (table["c"][ci, :dim] + (k * ch).astype(F)).astype(F)


def queries_face_ulp(table, rng, n, half):
    """Queries whose box edge is one float32 ulp before, exactly on, and one ulp after a cell face (qlo against hi, qhi against
    lo), the other coordinates at the cell centre."""
    dim = table["dim"]
    out = []
    ci = rng.integers(0, table["c"].shape[0], n)
    for i, cidx in enumerate(ci):
        ax = i % dim
        x = table["c"][cidx, :dim].copy()
        if (i // dim) % 2 == 0:
            xa = x_for_qlo(table["hi"][cidx, ax], half)
        else:
            xa = x_for_qhi(table["lo"][cidx, ax], half)
        if xa is None:
            continue
        for step in (-1, 0, 1):
            y = x.copy()
            y[ax] = xa if step == 0 else np.nextafter(xa, F(np.inf * step), dtype=F)
            out.append(y)
    return np.array(out, dtype=F).reshape(-1, dim)


def queries_outside(table, half):
    """Queries off the lattice's faces by more than, exactly and just under the search half, and far away (the clamped cell
    window is empty)."""
    dim = table["dim"]
    lo = table["lo"][:, :dim].min(axis=0); hi = table["hi"][:, :dim].max(axis=0)
    mid = ((lo + hi) * F(0.5)).astype(F)
    out = []
    for ax in range(dim):
        for side in (0, 1):
            base = mid.copy()
            edge = hi[ax] if side else lo[ax]
            xa = x_for_qlo(edge, half) if side else x_for_qhi(edge, half)
            sgn = F(np.inf) if side else F(-np.inf)
            if xa is not None:
                for y in (xa, np.nextafter(xa, sgn, dtype=F), np.nextafter(xa, -sgn, dtype=F)):
                    b = base.copy(); b[ax] = y; out.append(b)
            for far in (2.0, 40.0, 1e4):
                b = base.copy(); b[ax] = F(edge + F(far * float(half)) * (1 if side else -1)); out.append(b)
    out.append((hi + F(1e3)).astype(F)); out.append((lo - F(1e3)).astype(F))
    return np.array(out, dtype=F).reshape(-1, dim)
