"""Synthetic cluster tables and query sets for the K5 tests (test_k5_ref.py asserts their populations from the reference alone,
test_gpu_k5.py runs them on the kernels).  Real geometry: 3-D cluster half 0.025 (pitch 0.05) with search half 0.075, 2-D
cluster half 0.8 (pitch 1.6) with search half 4.8 -- the maps' own parameters."""
import numpy as np

import k5_ref as K

F = np.float32
GEOM = {
    3: dict(cluster_half=F(0.025), half=F(np.float64(F(0.025)) * 3.0), var_thre=F(0.5), prior=F(1.0 + np.float64(F(5e-3))),
            scale=0.04, root=(0.4, 0.4, 0.4)),
    2: dict(cluster_half=F(0.8), half=F(np.float64(F(1.2)) * 4.0), var_thre=F(0.4), prior=F(1.0 + np.float64(F(1e-2))),
            scale=1.2, root=(12.8, 12.8)),
}


def table(dim, kind, seed=1, occupancy=0.4):
    """kind: "sparse" (`occupancy`, ~40 %, of a 12^3 / 40^2 block), "dense" (8^3 / 16^2, every cell)."""
    g = GEOM[dim]
    rng = np.random.default_rng(seed)
    if kind == "sparse":
        levels, block = (4, 12) if dim == 3 else (6, 40)
        side = 1 << levels
        occ = np.zeros((side,) * dim, dtype=bool)
        sl = (slice(2, 2 + block),) * dim
        occ[sl] = rng.random((block,) * dim) < occupancy
    else:
        levels = 3 if dim == 3 else 4
        occ = np.ones((1 << levels,) * dim, dtype=bool)
    return K.build_table(dim, levels, lambda ijk: occ[ijk], g["cluster_half"], g["root"])


def box_table(dim, shape):
    """Every cell of a shape[0] x shape[1] (x shape[2]) block at the lattice's low corner."""
    levels = int(np.ceil(np.log2(max(shape))))
    return K.build_table(dim, levels, lambda ijk: all(ijk[d] < shape[d] for d in range(dim)), GEOM[dim]["cluster_half"],
                         GEOM[dim]["root"])


def queries_random(tab, rng, n, margin=1.5):
    dim = tab["dim"]
    lo = tab["lo"][:, :dim].min(axis=0).astype(np.float64); hi = tab["hi"][:, :dim].max(axis=0).astype(np.float64)
    m = margin * tab["pitch"]
    return rng.uniform(lo - m, hi + m, (n, dim)).astype(F)


def lookup_queries(tab, seed, n_random=1500, n_aligned=1500, n_face=120):
    """Random, lattice-aligned, face +- 1 ulp and outside queries, plus one crafted ancestor (changes tab in place)."""
    rng = np.random.default_rng(seed)
    half = GEOM[tab["dim"]]["half"]
    # a cell in the interior of the table whose first ancestor gets a hi one ulp below the cell's own
    for cell in np.argsort(np.abs(tab["c"][:, :tab["dim"]] - tab["c"][:, :tab["dim"]].mean(axis=0)).sum(axis=1), kind="stable"):
        xc = K.craft_ancestor(tab, int(cell), half)
        if xc is not None:
            break
    assert xc is not None
    xs = [queries_random(tab, rng, n_random), K.queries_aligned(tab, rng, n_aligned), K.queries_face_ulp(tab, rng, n_face, half),
          K.queries_outside(tab, half), xc[None, :]]
    return np.concatenate(xs).astype(F), int(cell)


def punch_holes(tab, seed, frac=0.2):
    """model = -1 in a fraction of the cells."""
    rng = np.random.default_rng(seed)
    tab["model"] = np.where(rng.random(tab["model"].size) < frac, -1, tab["model"]).astype(np.int32)
    return tab


def hole_positions(ncand, cand):
    """Histogram of which of the candidate positions hold no model, per query: key = tuple of the positions (0-based)."""
    out = {}
    for k in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        m = np.ones(ncand.size, dtype=bool)
        for p in range(3):
            inpos = (ncand > p) & (cand[p] < 0)
            m &= inpos if p in k else ~inpos
        out[k] = int(m.sum())
    return out


# ---------------------------------------------------------------------------------------- tie guard (2-D) ----
TIE_GUARD_HALF = F(7.0 * 1.6)


def tie_guard_case():
    """Three L-shaped blocks of 11 x 11 + 6 / 7 / 8 cells under a search box of 7 pitches: lattice-aligned queries around each
    block's middle see 127, 128 and 129 candidates, with ties.  Returns (table, queries)."""
    g = GEOM[2]
    blocks = {(2, 2): 6, (2, 34): 7, (34, 2): 8}

    def occupied(ijk):
        for (bx, by), extra in blocks.items():
            i, j = ijk[0] - bx, ijk[1] - by
            if 0 <= i < 11 and (0 <= j < 11 or (j == 11 and i < extra)):
                return True
        return False

    tab = K.build_table(2, 6, occupied, g["cluster_half"], g["root"])
    mids = [i for b in blocks for i in range(tab["c"].shape[0]) if tuple(tab["ijk"][i] - np.array(b)) == (5, 5)]
    steps = np.array([(a, b) for a in range(-2, 3) for b in range(-2, 3)], dtype=F)
    x = np.concatenate([(tab["c"][m, :2] + steps * g["cluster_half"]).astype(F) for m in mids])
    return tab, x


# ------------------------------------------------------------------------------------------------ binning ----
BINNING = [(1, 4095), (1023, 4096), (1024, 4097), (1025, 2047), (8192, 2048), (8193, 2049)]
CYCLE = np.array([200, 0, 1, 7, 8, 9, 31, 32, 33, 10, 11])        # pass-1 jobs per model (200: whole waves on one model)
NFAR = 4


def n_cell_table(dim, ncells):
    """Exactly ncells cells: the first ncells in raster order of the smallest cube that holds them."""
    side = int(np.ceil(ncells ** (1.0 / dim) - 1e-9))
    levels = max(1, int(np.ceil(np.log2(side))))
    rank = lambda ijk: sum(int(ijk[d]) * side ** d for d in range(dim)) if all(v < side for v in ijk) else ncells
    return K.build_table(dim, levels, lambda ijk: rank(ijk) < ncells, GEOM[dim]["cluster_half"], GEOM[dim]["root"])


def binning_cycles(slots, n):
    return min((n // 2) // int(CYCLE.sum()), slots // 22)


def binning_queries(tab, n, rng):
    """n queries, each inside a cell (its centre is their nearest).  First the cells of whole cycles of CYCLE, in cell order
    (waves of one model); then round robin over the other cells (64 distinct models per wave); a far query (no candidate, no
    job) goes in front of every 63 of the first 252: lane 0 of those waves is jobless.  Returns (x, cells [n] (-1: far),
    counted = number of leading cells that got their CYCLE count)."""
    dim = tab["dim"]
    slots = tab["c"].shape[0]
    per = np.tile(CYCLE, binning_cycles(slots, n)) if slots > 1 else np.array([n - NFAR])
    cells = np.repeat(np.arange(per.size), per)
    first = per.size if slots > 1 else 0
    cells = np.concatenate([cells, first + np.arange(n - NFAR - cells.size) % max(slots - first, 1)])
    x = (tab["c"][cells, :dim] + rng.uniform(-0.4, 0.4, (n - NFAR, dim)).astype(F) * GEOM[dim]["cluster_half"]).astype(F)
    x = np.insert(x, np.arange(NFAR) * 63, F(1e3), axis=0)
    cells = np.insert(cells, np.arange(NFAR) * 63, -1)
    return x, cells, per.size


def wave_populations(jm):
    """Of the pass-1 job list jm (model per query, -1 none), per 64-lane wave: waves of one model, of one model behind a jobless
    lane 0, of 64 distinct models, with a jobless lane 0."""
    waves = [jm[i:i + 64] for i in range(0, jm.size - 63, 64)]
    return dict(one=sum(1 for w in waves if w[0] >= 0 and np.all(w == w[0])),
                one_lane0=sum(1 for w in waves if w[0] < 0 and w[1] >= 0 and np.all(w[1:] == w[1])),
                distinct=sum(1 for w in waves if np.unique(w[w >= 0]).size == 64),
                lane0=sum(1 for w in waves if w[0] < 0 and (w[1:] >= 0).any()))


# ------------------------------------------------------------------------------ tile edges of every pass ----
def islands_table():
    """3-D: 27 islands, six cells apart, of three cells in a row along x (A, B, C); the last nine islands lack C.  A query
    inside B sees exactly the island: three candidates (pass 2a / 2b) or two (pass 2, all columns), B nearest.  Returns
    (table, islands): islands[i] = table indices (A, B, C), C = -1 for a pair."""
    cells = {}
    for k, (z, y, x0) in enumerate((z, y, x0) for z in (0, 6, 12) for y in (0, 6, 12) for x0 in (0, 6, 12)):
        for j in range(3 if k < 18 else 2):
            cells[(x0 + j, y, z)] = (k, j)
    tab = K.build_table(3, 4, lambda ijk: tuple(ijk) in cells, GEOM[3]["cluster_half"], GEOM[3]["root"])
    isl = np.full((27, 3), -1, dtype=np.int64)
    for i, ijk in enumerate(tab["ijk"]):
        k, j = cells[tuple(int(v) for v in ijk)]
        isl[k, j] = i
    return tab, isl


def island_queries(tab, isl, rng, per_island):
    """per_island queries inside cell B of every island (jitter of 0.4 cell halves).  Returns (x, island index per query)."""
    own = np.repeat(np.arange(isl.shape[0]), per_island)
    x = (tab["c"][isl[own, 1], :3] + rng.uniform(-0.4, 0.4, (own.size, 3)).astype(F) * GEOM[3]["cluster_half"]).astype(F)
    return x, own
