"""Reference for the zero-level surface extraction (csrc/mesh.hip, DESIGN.md "Surface extraction"): a vectorised numpy float32
restatement of the algorithm with the same numbering, orientation and order, written independently of the product (it imports
nothing from gpismap_amd).

Lattice: point (i, j, k) has index p = (k ny + j) nx + i (x fastest) and coordinates o + float32(i) * s per axis, no FMA.
Inside iff f < level.  Triangulation: marching tetrahedra on the Freudenthal (Kuhn) split -- 6 tetrahedra per cell
0 -> e_a -> e_a + e_b -> (1,1,1) for the axis orders xyz, xzy, yxz, yzx, zxy, zyx; in 2-D 2 triangles per square,
0 -> e_x -> (1,1) and 0 -> e_y -> (1,1).  Every edge runs from a lattice point p to p + d, d a non-zero 0/1 vector numbered
x + 2y + 4z; edge id = (2^dim - 1) p + (d - 1).  One vertex per crossed edge (both ends finite, exactly one inside), numbered in
edge-id order, at t = (level - f_a) / (f_b - f_a), x = a + t (b - a), all float32.

The orientation here is derived from integer geometry of the unit simplex (the kernels use the permutation parity instead)."""
import numpy as np

F32 = np.float32
TETS3 = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]   # xyz, xzy, yxz, yzx, zxy, zyx
TRIS2 = [(0,), (1,)]                                                            # 0 -> e_x -> (1,1), 0 -> e_y -> (1,1)


def axes(shape, origin, step):
    return [F32(origin[a]) + np.arange(shape[a]).astype(F32) * F32(step[a]) for a in range(len(shape))]


def lattice(shape, origin, step):
    """[prod(shape), dim] float32, x fastest: the points extract() evaluates the map at."""
    ax = axes(shape, origin, step)
    g = np.meshgrid(*ax[::-1], indexing="ij")
    return np.stack([c.ravel() for c in g[::-1]], axis=1).astype(F32)


def _simplices(dim):
    """Corner lists (integer 0/1 vectors) of the simplices of one cell, in emission order."""
    out = []
    if dim == 3:
        for perm in TETS3:
            c = [np.zeros(3, int)]
            for a in perm:
                c.append(c[-1] + np.eye(3, dtype=int)[a])
            out.append(c)
    else:
        for (a,) in TRIS2:
            e = np.eye(2, dtype=int)[a]
            out.append([np.zeros(2, int), e, np.ones(2, int)])
    return out


def _table(dim):
    """table[s][code] = list of primitives, each a list of simplex edges (i, j), i < j, in output winding (quads as 4-cycles)."""
    tab = []
    for C in _simplices(dim):
        nc = dim + 1
        rows = []
        for code in range(1 << nc):
            ins = [(code >> i) & 1 for i in range(nc)]
            I = [i for i in range(nc) if ins[i]]
            O = [i for i in range(nc) if not ins[i]]
            if not I or not O:
                rows.append([])
                continue
            d = len(I) * sum(C[o] for o in O) - len(O) * sum(C[i] for i in I)     # inside -> outside
            M = lambda e: C[e[0]] + C[e[1]]                                     # 2 x edge midpoint
            E = lambda i, j: (min(i, j), max(i, j))
            if dim == 2:
                L = I[0] if len(I) == 1 else O[0]
                J = [j for j in range(nc) if j != L]
                seg = [E(L, J[0]), E(L, J[1])]
                t = M(seg[1]) - M(seg[0])
                if t[1] * d[0] - t[0] * d[1] < 0:          # right-hand normal (dy, -dx) . d
                    seg = seg[::-1]
                rows.append([seg])
            elif len(I) != 2:
                L = I[0] if len(I) == 1 else O[0]
                tri = [E(L, j) for j in range(nc) if j != L]
                if np.dot(np.cross(M(tri[1]) - M(tri[0]), M(tri[2]) - M(tri[0])), d) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                rows.append([tri])
            else:
                q = [E(I[0], O[0]), E(I[0], O[1]), E(I[1], O[1]), E(I[1], O[0])]
                if np.dot(np.cross(M(q[1]) - M(q[0]), M(q[2]) - M(q[0])), d) < 0:
                    q = q[::-1]
                rows.append([q])
        tab.append((C, rows))
    return tab


_TABLES = {2: _table(2), 3: _table(3)}


def _popcount8(x):
    x = x.astype(np.int64)
    return sum((x >> b) & 1 for b in range(8))


def extract(val, shape, origin, step, level):
    """val: prod(shape) float32 (x fastest).  Returns (verts [V, dim] f32, prims [P, dim] i32, mask [n] u8, vbase [n] i64)."""
    dim = len(shape)
    assert dim in (2, 3)
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    v = np.ascontiguousarray(val, dtype=F32).reshape(n)
    level = F32(level)
    strides = [1, shape[0], shape[0] * (shape[1] if dim == 3 else 1)][:dim]
    V = v.reshape(shape[::-1])
    fin = np.isfinite(V)
    ins = fin & (V < level)
    nd = (1 << dim) - 1
    dirs = [tuple((d >> a) & 1 for a in range(dim)) for d in range(1, nd + 1)]
    crossed = np.zeros(shape[::-1] + (nd,), bool)
    for di, dv in enumerate(dirs):
        lo = tuple(slice(0, shape[a] - dv[a]) for a in range(dim))[::-1]
        hi = tuple(slice(dv[a], shape[a]) for a in range(dim))[::-1]
        crossed[lo + (di,)] = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
    crossed = crossed.reshape(n, nd)
    mask = np.zeros(n, np.uint8)
    for di in range(nd):
        mask |= (crossed[:, di].astype(np.uint8) << di)
    cnt = _popcount8(mask)
    vbase = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)

    # vertices in edge-id order (np.nonzero on [n, nd] is p-major, d-minor)
    ep, ed = np.nonzero(crossed)
    idx = [(ep // strides[a]) % shape[a] for a in range(dim)]
    dvec = np.array(dirs, dtype=np.int64)[ed]
    off = (dvec * np.array(strides, dtype=np.int64)).sum(1)
    fa, fb = v[ep], v[ep + off]
    t = (level - fa) / (fb - fa)
    ax = axes(shape, origin, step)
    verts = np.empty((ep.size, dim), F32)
    for a in range(dim):
        xa = ax[a][idx[a]]
        xb = ax[a][idx[a] + dvec[:, a]]
        verts[:, a] = xa + t * (xb - xa)
    assert verts.dtype == F32

    # primitives: cells = lattice points that are not on an upper face
    cell_ok = np.ones(shape[::-1], bool)
    for a in range(dim):
        sl = [slice(None)] * dim
        sl[dim - 1 - a] = -1
        cell_ok[tuple(sl)] = False
    cells = np.nonzero(cell_ok.reshape(n))[0]
    finf, insf = fin.reshape(n), ins.reshape(n)

    def vidx(base, C, e):
        i, j = e
        ci = base + int(np.dot(C[i], strides))
        d = sum(int(C[j][a] - C[i][a]) << a for a in range(dim))
        return vbase[ci] + _popcount8(mask[ci] & ((1 << (d - 1)) - 1))

    keys_cell, keys_s, tris = [], [], []
    for s, (C, rows) in enumerate(_TABLES[dim]):
        corners = [cells + int(np.dot(c, strides)) for c in C]
        allfin = np.logical_and.reduce([finf[c] for c in corners])
        code = sum(insf[c].astype(np.int64) << i for i, c in enumerate(corners))
        for cd in range(1, (1 << (dim + 1)) - 1):
            sel = allfin & (code == cd)
            if not sel.any():
                continue
            base = cells[sel]
            for prim in rows[cd]:
                q = np.stack([vidx(base, C, e) for e in prim], axis=1)
                if dim == 2:
                    out = [q]
                elif q.shape[1] == 3:
                    out = [q]
                else:   # quad: split on the diagonal through its smallest index
                    r = np.argmin(q, axis=1)
                    qq = np.stack([q[np.arange(q.shape[0]), (r + k) % 4] for k in range(4)], axis=1)
                    out = [qq[:, [0, 1, 2]], qq[:, [0, 2, 3]]]
                for o in out:
                    if dim == 3:   # rotate: smallest index first (keeps the winding)
                        r = np.argmin(o, axis=1)
                        o = np.stack([o[np.arange(o.shape[0]), (r + k) % 3] for k in range(3)], axis=1)
                    keys_cell.append(base)
                    keys_s.append(np.full(base.size, s))
                    tris.append(o)
    if tris:
        kc, ks, T = np.concatenate(keys_cell), np.concatenate(keys_s), np.concatenate(tris)
        order = np.lexsort(tuple(T[:, a] for a in range(dim - 1, -1, -1)) + (ks, kc))
        prims = T[order].astype(np.int32)
    else:
        prims = np.zeros((0, dim), np.int32)
    return verts, prims, mask, vbase


# ---- analytic checks used by the tests ------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every directed edge exactly once, and its reverse exactly once (a closed, consistently oriented 2-manifold edge set)."""
    e = directed_edges(faces)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rkey = e[:, 1] * (1 << 32) + e[:, 0]
    if np.unique(key).size != key.size:
        return False
    return bool(np.array_equal(np.sort(key), np.sort(rkey)))


def euler_characteristic(faces):
    f = np.asarray(faces, np.int64)
    e = directed_edges(f)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return int(np.unique(f).size) - int(und.shape[0]) + int(f.shape[0])


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


__all__ = ["lattice", "axes", "extract", "is_closed_oriented", "euler_characteristic", "face_normals"]
