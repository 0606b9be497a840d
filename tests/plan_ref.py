"""numpy / heapq reference of the path planner (csrc/plan.hip), written from the definitions in float32 without FMA.

Lattice: shape = (nx, ny[, nz]), index p = (k ny + j) nx + i, world point origin + (float)i * step.  Arrays are held as
[nz, ny, nx] (nz = 1 in 2-D); the results are flat, x fastest.  Direction index of the offset (dx, dy, dz):
k = ((dz + 1) 3 + (dy + 1)) 3 + (dx + 1), 13 = stay."""
import heapq

import numpy as np

F32 = np.float32
INF = F32(np.inf)
STAY, NONE = 13, 255


def offset(k):
    return k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1


def offsets(dim, connectivity):
    """[(k, (dx, dy, dz))] in ascending k."""
    out = []
    for k in range(27):
        dx, dy, dz = offset(k)
        nnz = (dx != 0) + (dy != 0) + (dz != 0)
        if nnz == 0 or (dim == 2 and dz != 0) or (connectivity == 0 and nnz != 1):
            continue
        out.append((k, (dx, dy, dz)))
    return out


def _nbr(a, o, fill):
    """b[p] = a[p + o], `fill` outside the lattice."""
    dx, dy, dz = o
    nz, ny, nx = a.shape
    p = np.pad(a, 1, constant_values=fill)
    return p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def snap(points, shape, origin, step):
    """(ok [m], ijk [m, 3]): i = (int)floorf(u + 0.5f), u = (x - origin) / step; ok = finite and inside the lattice."""
    dim = len(shape)
    x = np.ascontiguousarray(points, F32).reshape(-1, dim)
    ok = np.ones(x.shape[0], bool)
    ijk = np.zeros((x.shape[0], 3), np.int64)
    with np.errstate(all="ignore"):
        for a in range(dim):
            f = np.floor((x[:, a] - F32(origin[a])) / F32(step) + F32(0.5))
            good = np.isfinite(x[:, a]) & (f >= 0) & (f <= F32(shape[a] - 1))
            ijk[:, a] = np.where(good, f, 0).astype(np.int64)
            ok &= good
    return ok, ijk


class Problem:
    """Free mask, point costs, edges and goal points of one solve."""

    def __init__(self, dist, shape, origin, step, goals, clearance=0.0, margin=0.0, gain=4.0, connectivity=1):
        self.dim = len(shape)
        self.shape = tuple(int(v) for v in shape)
        self.origin = tuple(float(v) for v in origin)
        self.step = F32(step)
        nx, ny = self.shape[0], self.shape[1]
        nz = self.shape[2] if self.dim == 3 else 1
        self.n3 = (nz, ny, nx)
        d = np.ascontiguousarray(dist, F32).reshape(self.n3)
        cl, mg, gn = F32(clearance), F32(margin), F32(gain)
        self.free = d >= cl
        with np.errstate(all="ignore"):
            if mg > 0:
                t = np.maximum(F32(0), mg - (d - cl)) / mg
                c = F32(1) + gn * (t * t)
            else:
                c = np.ones(self.n3, F32)
        self.c = np.where(self.free, c, F32(0)).astype(F32)
        ls = [F32(1) * self.step, np.sqrt(F32(2)) * self.step, np.sqrt(F32(3)) * self.step]
        self.edges = []                                  # (k, o, exists [n3], weight [n3])
        for k, o in offsets(self.dim, connectivity):
            e = self.free.copy()
            for a in range(1, 8):
                s = (o[0] if a & 1 else 0, o[1] if a & 2 else 0, o[2] if a & 4 else 0)
                if s != (0, 0, 0):
                    e &= _nbr(self.free, s, False)
            nnz = sum(v != 0 for v in o)
            w = ls[nnz - 1] * (F32(0.5) * (self.c + _nbr(self.c, o, F32(0))))
            assert w.dtype == F32
            self.edges.append((k, o, e, w))
        ok, ijk = snap(goals, self.shape, self.origin, self.step)
        self.goal = np.zeros(self.n3, bool)
        self.goals_given = ok.size
        self.goals_kept = 0
        for g in range(ok.size):
            i, j, kk = ijk[g]
            if ok[g] and self.free[kk, j, i]:
                self.goal[kk, j, i] = True
                self.goals_kept += 1

    def start_cost(self):
        return np.where(self.goal, F32(0), INF).astype(F32)

    def world(self, ijk):
        ijk = np.asarray(ijk)
        return np.stack([F32(self.origin[a]) + ijk[..., a].astype(F32) * self.step for a in range(self.dim)], axis=-1).astype(F32)


def solve_sweep(pb):
    """Whole-array relaxations, one offset after the other, to the fixed point.  Flat float32 cost."""
    cost = pb.start_cost()
    while True:
        old = cost.copy()
        for k, o, e, w in pb.edges:
            cand = _nbr(cost, o, INF) + w
            cost = np.where(e & (cand < cost), cand, cost)
        if np.array_equal(old, cost):
            return cost.ravel()


def solve_dijkstra(pb):
    """heapq Dijkstra with the same float32 additions.  Flat float32 cost."""
    nz, ny, nx = pb.n3
    cost = pb.start_cost().ravel()
    ed = [(o[0] + nx * (o[1] + ny * o[2]), e.ravel(), w.ravel()) for k, o, e, w in pb.edges]
    heap = [(0.0, int(p)) for p in np.flatnonzero(pb.goal.ravel())]
    heapq.heapify(heap)
    done = np.zeros(cost.size, bool)
    while heap:
        d, p = heapq.heappop(heap)
        if done[p] or d > cost[p]:
            continue
        done[p] = True
        for dp, e, w in ed:
            if e[p]:
                q = p + dp
                nd = F32(cost[p] + w[p])
                if nd < cost[q]:
                    cost[q] = nd
                    heapq.heappush(heap, (float(nd), q))
    return cost


def policy(pb, cost):
    """Flat uint8 policy of a converged cost: 13 at goals, the k minimising fl(cost[q] + w) (ties: the smaller cost[q], then the
    smaller k) at free points of finite cost, 255 elsewhere."""
    cst = np.ascontiguousarray(cost, F32).reshape(pb.n3)
    best = np.full(pb.n3, INF, F32)
    bestq = np.full(pb.n3, INF, F32)
    pol = np.full(pb.n3, NONE, np.uint8)
    for k, o, e, w in pb.edges:
        cq = _nbr(cst, o, INF)
        v = cq + w
        take = e & ((v < best) | ((v == best) & (cq < bestq)))
        best = np.where(take, v, best)
        bestq = np.where(take, cq, bestq)
        pol = np.where(take, np.uint8(k), pol)
    pol = np.where(pb.free & np.isfinite(cst), pol, np.uint8(NONE))
    pol = np.where(pb.goal, np.uint8(STAY), pol)
    return pol.astype(np.uint8).ravel()


def paths(pb, cost, pol, starts, max_points):
    """(off int64 [m + 1], points f32 [off[m], dim], start_cost f32 [m], status u8 [m]) of the policy walks."""
    nz, ny, nx = pb.n3
    cst = np.ascontiguousarray(cost, F32).ravel()
    pol = np.ascontiguousarray(pol, np.uint8).ravel()
    free = pb.free.ravel()
    ok, ijk = snap(starts, pb.shape, pb.origin, pb.step)
    m = ok.size
    status = np.zeros(m, np.uint8)
    sc = np.full(m, np.nan, F32)
    cells = []
    for t in range(m):
        pts = []
        if not ok[t]:
            status[t] = 1
        else:
            i, j, k = (int(v) for v in ijk[t])
            p = (k * ny + j) * nx + i
            sc[t] = cst[p]
            if not free[p]:
                status[t] = 2
            elif not np.isfinite(cst[p]):
                status[t] = 3
            else:
                pts.append((i, j, k))
                while pol[p] != STAY:
                    if len(pts) >= max_points:
                        status[t] = 4
                        break
                    dx, dy, dz = offset(int(pol[p]))
                    i, j, k = i + dx, j + dy, k + dz
                    q = (k * ny + j) * nx + i
                    if not cst[q] < cst[p]:
                        status[t] = 4
                        break
                    p = q
                    pts.append((i, j, k))
        cells.append(np.array(pts, np.int64).reshape(-1, 3))
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([c.shape[0] for c in cells])
    allc = np.concatenate(cells) if m else np.zeros((0, 3), np.int64)
    return off, pb.world(allc).reshape(-1, pb.dim), sc, status


def check_path_invariants(pb, cost, path_points):
    """The three invariants of one path given as world points: consecutive points are lattice neighbours joined by an existing
    edge, every point is free, cost[p_i] == fl(cost[p_{i+1}] + w) bit for bit."""
    cst = np.ascontiguousarray(cost, F32).reshape(pb.n3)
    ok, ijk = snap(path_points, pb.shape, pb.origin, pb.step)
    assert ok.all()
    assert np.array_equal(pb.world(ijk).view(np.uint32), np.ascontiguousarray(path_points, F32).view(np.uint32))
    ed = {o: (e, w) for k, o, e, w in pb.edges}
    for a, b in zip(ijk[:-1], ijk[1:]):
        o = tuple(int(v) for v in (b - a))
        assert o in ed, o
        e, w = ed[o]
        assert e[a[2], a[1], a[0]]
        assert pb.free[a[2], a[1], a[0]] and pb.free[b[2], b[1], b[0]]
        lhs = cst[a[2], a[1], a[0]]
        rhs = F32(cst[b[2], b[1], b[0]] + w[a[2], a[1], a[0]])
        assert lhs.view(np.uint32) == rhs.view(np.uint32), (a, b, lhs, rhs)
    assert all(pb.free[k, j, i] for i, j, k in ijk)
