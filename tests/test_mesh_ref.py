"""Surface extraction, CPU side: the numpy reference (tests/mesh_ref.py) on analytic fields, a scalar restatement of the kernels'
winding rule (permutation parity, csrc/mesh.hip) against the reference's integer geometry, and the C-ABI symbols of the build."""
import ctypes as C
import os

import numpy as np

import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def sphere(shape, origin, step, r):
    X = mesh_ref.lattice(shape, origin, step).astype(np.float64)
    return (np.sqrt((X ** 2).sum(1)) - r).astype(F32)


def nondegenerate_outward(verts, faces, centre=0.0):
    N = mesh_ref.face_normals(verts, faces)
    a = np.linalg.norm(N, axis=1)
    c = verts[faces].astype(np.float64).mean(1) - centre
    ok = a > 1e-12
    return bool(np.all(np.einsum("ij,ij->i", N[ok], c[ok]) > 0)), N, a


def test_sphere_closed_oriented_area():
    """64^3 lattice, radius 20.3 steps: closed, every edge used once in each direction, Euler characteristic 2, every normal
    outward, area within 1 % of 4 pi r^2.  The radius 22 (integer: lattice points exactly on the level, f == level ties) as well."""
    shape, origin, step = (64, 64, 64), (-32.0, -32.0, -32.0), (1.0, 1.0, 1.0)
    for r in (20.3, 22.0):
        v, f, mask, vbase = mesh_ref.extract(sphere(shape, origin, step, r), shape, origin, step, 0.0)
        assert f.shape[0] > 1000
        assert mesh_ref.is_closed_oriented(f)
        assert mesh_ref.euler_characteristic(f) == 2
        out, N, a = nondegenerate_outward(v, f)
        assert out
        area = a.sum() / 2
        assert abs(area / (4 * np.pi * r * r) - 1) < 0.01, area
        # every vertex on its edge, numbered in edge order
        assert v.shape[0] == int(sum(bin(int(m)).count("1") for m in mask))
        assert np.all(np.abs(np.sqrt((v.astype(np.float64) ** 2).sum(1)) - r) < 0.5)


def test_plane_through_lattice_points():
    """f = z - z0 with z0 a lattice coordinate: the points on the plane count as outside (f == level), so every vertex lies
    exactly on them (t = 1), every non-degenerate face points to +z, and every interior edge is shared by two faces in
    opposite directions."""
    shape, origin, step = (9, 8, 10), (0.0, 0.0, 0.0), (0.5, 0.25, 0.125)
    X = mesh_ref.lattice(shape, origin, step)
    z0 = X[4 * 9 * 8, 2]
    val = (X[:, 2] - z0).astype(F32)
    v, f, _, _ = mesh_ref.extract(val, shape, origin, step, 0.0)
    assert f.shape[0] > 0
    assert np.all(v[:, 2] == z0)
    N = mesh_ref.face_normals(v, f)
    a = np.linalg.norm(N, axis=1)
    assert np.all(N[a > 0, 2] > 0)
    e = mesh_ref.directed_edges(f)
    key = set(map(tuple, e.tolist()))
    assert len(key) == e.shape[0]           # no directed edge twice
    # a level between the lattice planes cuts every tetrahedron of a layer: 8 triangles per cell (the two axis orders with z
    # in the middle give quads), all on one flat sheet
    v, f, _, _ = mesh_ref.extract(val, shape, origin, step, 0.0625)
    assert f.shape[0] == 8 * 8 * 7
    assert np.unique(v[:, 2]).size == 1
    N = mesh_ref.face_normals(v, f)
    assert np.all(N[:, 2] > 0)


def test_nan_corners_emit_nothing():
    """NaN lattice values: no crossed edge touches one, no simplex with a NaN corner emits, the rest is unchanged."""
    shape, origin, step = (24, 21, 19), (-12.0, -10.5, -9.5), (1.0, 1.0, 1.0)
    val = sphere(shape, origin, step, 7.3)
    rng = np.random.default_rng(5)
    nanp = rng.choice(val.size, 60, replace=False)
    bad = val.copy()
    bad[nanp] = np.nan
    v, f, mask, vbase = mesh_ref.extract(bad, shape, origin, step, 0.0)
    assert np.all(mask[nanp] == 0)
    assert np.all(np.isfinite(v))
    # fewer primitives than the NaN-free field, and the scalar restatement agrees exactly
    v0, f0, _, _ = mesh_ref.extract(val, shape, origin, step, 0.0)
    assert 0 < f.shape[0] < f0.shape[0]
    sv, sf = scalar_extract(bad, shape, origin, step, 0.0)
    assert np.array_equal(sv, v) and np.array_equal(sf, f)


def test_circle_closed_directed_cycles():
    shape, origin, step = (61, 47), (-30.0, -23.0), (1.0, 1.0)
    X = mesh_ref.lattice(shape, origin, step).astype(np.float64)
    for r in (15.4, 15.0):
        val = (np.sqrt((X ** 2).sum(1)) - r).astype(F32)
        v, s, _, _ = mesh_ref.extract(val, shape, origin, step, 0.0)
        assert s.shape[0] > 50
        # every vertex starts exactly one segment and ends exactly one: a union of directed cycles; here a single one
        assert np.array_equal(np.sort(s[:, 0]), np.arange(v.shape[0]))
        assert np.array_equal(np.sort(s[:, 1]), np.arange(v.shape[0]))
        nxt = dict(zip(s[:, 0].tolist(), s[:, 1].tolist()))
        cur, seen = int(s[0, 0]), 0
        while True:
            cur = nxt[cur]; seen += 1
            if cur == s[0, 0]:
                break
        assert seen == s.shape[0]
        d = (v[s[:, 1]] - v[s[:, 0]]).astype(np.float64)
        nrm = np.stack([d[:, 1], -d[:, 0]], 1)
        mid = (v[s[:, 1]] + v[s[:, 0]]).astype(np.float64) / 2
        ok = np.linalg.norm(d, axis=1) > 0
        assert np.all(np.einsum("ij,ij->i", nrm[ok], mid[ok]) > 0)


# ---- scalar restatement of csrc/mesh.hip (permutation-parity winding) ---------------------------------------------------------
TET = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
TET_SIGN = [1, -1, -1, 1, 1, -1]
TRI = [(0, 1, 3), (0, 2, 3)]
TRI_SIGN = [1, -1]


def scalar_extract(val, shape, origin, step, level):
    dim = len(shape)
    nx, ny = shape[0], shape[1]
    nz = shape[2] if dim == 3 else 1
    n = nx * ny * nz
    level = F32(level)
    ax = mesh_ref.axes(shape, origin, step)

    def off(c):
        return (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny

    def flags(p):
        i, j, k = p % nx, (p // nx) % ny, p // (nx * ny)
        fin = ins = 0
        for c in range(1 << dim):
            if i + (c & 1) >= nx or j + ((c >> 1) & 1) >= ny or k + ((c >> 2) & 1) >= nz:
                continue
            f = val[p + off(c)]
            if np.isfinite(f):
                fin |= 1 << c
                if f < level:
                    ins |= 1 << c
        return i, j, k, fin, ins

    mask = np.zeros(n, int)
    for p in range(n):
        _, _, _, fin, ins = flags(p)
        if fin & 1:
            for d in range(1, 1 << dim):
                if (fin >> d) & 1 and ((ins >> d) ^ ins) & 1:
                    mask[p] |= 1 << (d - 1)
    cnt = np.array([bin(m).count("1") for m in mask])
    vbase = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    verts = []
    for p in range(n):
        i, j, k, _, _ = flags(p)
        idx = (i, j, k)
        for d in range(1, 1 << dim):
            if not (mask[p] >> (d - 1)) & 1:
                continue
            fa, fb = val[p], val[p + off(d)]
            t = (level - fa) / (fb - fa)
            x = []
            for a in range(dim):
                xa = ax[a][idx[a]]
                xb = ax[a][idx[a] + ((d >> a) & 1)]
                x.append(xa + t * (xb - xa))
            verts.append(x)

    def ev(u, w, p):
        lo, d = u & w, u ^ w
        q = p + off(lo)
        return int(vbase[q] + bin(mask[q] & ((1 << (d - 1)) - 1)).count("1"))

    def rot(t):
        m = t.index(min(t))
        return t[m:] + t[:m]

    prims = []
    for p in range(n):
        i, j, k, fin, ins = flags(p)
        if i >= nx - 1 or j >= ny - 1 or (dim == 3 and k >= nz - 1):
            continue
        if dim == 2:
            for s in range(2):
                c = TRI[s]
                if not all((fin >> q) & 1 for q in c):
                    continue
                inn = [(ins >> q) & 1 for q in c]
                nin = sum(inn)
                if nin in (0, 3):
                    continue
                L = [q for q in range(3) if inn[q] == (1 if nin == 1 else 0)][0]
                J = [q for q in range(3) if q != L]
                par = -1 if L & 1 else 1
                fwd = TRI_SIGN[s] * par > 0 if nin == 1 else TRI_SIGN[s] * par < 0
                a, b = ev(c[L], c[J[0]], p), ev(c[L], c[J[1]], p)
                prims.append([a, b] if fwd else [b, a])
            continue
        for s in range(6):
            c = TET[s]
            if not all((fin >> q) & 1 for q in c):
                continue
            inn = [(ins >> q) & 1 for q in c]
            nin = sum(inn)
            if nin in (0, 4):
                continue
            if nin != 2:
                L = [q for q in range(4) if inn[q] == (1 if nin == 1 else 0)][0]
                J = [q for q in range(4) if q != L]
                par = -1 if L & 1 else 1
                fwd = TET_SIGN[s] * par > 0 if nin == 1 else TET_SIGN[s] * par < 0
                v = [ev(c[L], c[q], p) for q in J]
                prims.append(rot(v if fwd else [v[0], v[2], v[1]]))
            else:
                I = [q for q in range(4) if inn[q]]
                O = [q for q in range(4) if not inn[q]]
                par = -1 if tuple(I) in ((0, 2), (1, 3)) else 1
                q4 = [ev(c[I[0]], c[O[0]], p), ev(c[I[0]], c[O[1]], p), ev(c[I[1]], c[O[1]], p), ev(c[I[1]], c[O[0]], p)]
                if TET_SIGN[s] * par < 0:
                    q4 = [q4[0], q4[3], q4[2], q4[1]]
                q4 = rot(q4)
                prims.extend(sorted([[q4[0], q4[1], q4[2]], [q4[0], q4[2], q4[3]]]))
    return np.array(verts, F32).reshape(-1, dim), np.array(prims, np.int32).reshape(-1, dim)


def test_kernel_winding_rule_matches_reference():
    """The kernels' winding (permutation parity of the simplex and its inside corners) restated in scalar Python equals the
    reference's (integer geometry of the unit simplex), vertices and primitives, 3-D and 2-D, ties and NaNs included."""
    rng = np.random.default_rng(11)
    for shape in ((7, 6, 5), (5, 9, 4)):
        origin, step = (-1.0, 0.5, 2.0), (0.3, 0.2, 0.25)
        val = rng.standard_normal(int(np.prod(shape))).astype(F32)
        val[rng.choice(val.size, 6, replace=False)] = 0.0        # ties at the level
        val[rng.choice(val.size, 4, replace=False)] = np.nan
        v, f, _, _ = mesh_ref.extract(val, shape, origin, step, 0.0)
        sv, sf = scalar_extract(val, shape, origin, step, 0.0)
        assert np.array_equal(sv, v) and np.array_equal(sf, f)
    for shape in ((13, 11), (9, 17)):
        origin, step = (0.5, -2.0), (0.1, 0.3)
        val = np.round(rng.standard_normal(int(np.prod(shape))) * 2).astype(F32) / 2
        val[rng.choice(val.size, 5, replace=False)] = np.nan
        v, f, _, _ = mesh_ref.extract(val, shape, origin, step, 0.25)
        sv, sf = scalar_extract(val, shape, origin, step, 0.25)
        assert np.array_equal(sv, v) and np.array_equal(sf, f)


MESH_SYMBOLS = ("gpis_mesh_create", "gpis_mesh_destroy", "gpis_mesh_set_chunk", "gpis_mesh_from_grid", "gpis3_extract_mesh",
                "gpis2_extract_contour", "gpis_mesh_counts", "gpis_mesh_get", "gpis_mesh_get_grid", "gpis_mesh_device")


def test_surface_extraction_symbols_exported():
    """The library built here (it loads without a GPU) exports the surface-extraction entries, and the header declares them."""
    import gpismap_amd
    L = C.CDLL(gpismap_amd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gpismap_amd.h")).read()
    for n in MESH_SYMBOLS:
        assert hasattr(L, n), "missing symbol " + n
        assert n + "(" in hdr, "undeclared " + n
