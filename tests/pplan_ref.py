"""numpy / heapq reference of the pose planner (csrc/pplan.hip, gpis_pplan_*), written from the definitions and
independently of the product (it imports nothing from gpismap_amd).  It is the path planner's reference (tests/plan_ref.py) on
the lattice nx x ny x H of poses (x, y, heading), with the free space and the point cost taken from the body rule
(tests/body_ref.py) at each heading layer.  float32 without FMA, except the body rule, which is double.

State s = (i, j, h), flat index (h ny + j) nx + i; arrays are held as [H, ny, nx] and results are flat, x fastest.
- D(i, j, h) = body_ref.body_rule at p = ((double)(ox + (float)i * step), (double)(oy + (float)j * step)) with the heading
  (c_h, s_h) of the caller's table, used as given.  d = (float)D; free iff d >= clearance (a NaN D -- a ball off the lattice,
  or a bilinear sample that met infinite dist values -- is not free); c = plan_ref's point cost on d, 0 where not free.
- Moves are directed.  Translation (p, h) -> (p + o, h), code k = 9 + (dy + 1) 3 + (dx + 1): exists iff bit k - 9 of moves[h]
  is set, the target is in the lattice and p + every non-empty subset of o's components is free in layer h; weight
  (len * step) * (0.5f * (c[s] + c[s'])), len = 1 or sqrtf(2).  Turn (p, h) -> (p, h +- 1 mod H), codes 27 (+1) and 28 (-1):
  exists iff both states are free; weight turn * (0.5f * (c[s] + c[s'])).
- cost = the greatest solution of cost[s] = min over moves s -> s' of fl(cost[s'] + w), 0 at the goals: a Dijkstra on the
  reversed graph.  Goals [g, 3] = (x, y, h): x, y snap as plan_ref.snap; h = -1 means every free heading at that point, each
  counted as a kept goal; a goal outside, non-finite or not free is dropped.
- policy: the code minimising fl(cost[s'] + w), ties to the smaller cost[s'], then the smaller code; 13 at goals; 255 where not
  free or unreachable.
- project(): cost2[p] = min_h cost[p, h], heading2[p] the first h attaining it (255 where cost2 is infinite), c2[p] the least c
  over free headings (0: none), policy2[p] = 13 where cost2 == 0, 255 where it is infinite, else the k in 9 .. 17 whose
  in-lattice neighbour has the least cost2 (ties: the smaller k).

The `variant` arguments build the defective variants tests/test_pplan_ref.py rejects; None is the contract: "rot_sign" (the
rotation's sign flipped), "no_wrap" (no turn between H - 1 and 0), "no_subset" (a diagonal needs only its target free),
"opposite_bit" (the move bit of the opposite direction), "along" (relaxing along the moves instead of against them),
"turn_step" (turn replaced by step), "nan_free" (a NaN body treated as free), "cast_first" (the (float) cast before
subtracting the radius), "ties_code" (policy ties by the smaller code only)."""
import heapq

import numpy as np

import body_ref
import dfield_ref
import plan_ref

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)
STAY, NONE, TURN_UP, TURN_DOWN = 13, 255, 27, 28
HS = (8, 16, 32, 64)
VARIANTS = ("rot_sign", "no_wrap", "no_subset", "opposite_bit", "along", "turn_step", "nan_free", "cast_first", "ties_code")
# a_k: the direction of code k as a multiple of 45 degrees anticlockwise from +x (a literal table, not atan2)
ANGLE8 = {14: 0, 17: 1, 16: 2, 15: 3, 12: 4, 9: 5, 10: 6, 11: 7}
TRANSLATIONS = tuple((k, ((k - 9) % 3 - 1, (k - 9) // 3 - 1)) for k in range(9, 18) if k != STAY)


def heading_table(H):
    """[H, 2] doubles (cos, sin) of 2 pi h / H, with exact 0 / +-1 at the quarter turns."""
    if H not in HS:
        raise ValueError("H outside {8, 16, 32, 64}")
    t = np.zeros((H, 2), F64)
    q = H // 4
    exact = {0: (1.0, 0.0), q: (0.0, 1.0), 2 * q: (-1.0, 0.0), 3 * q: (0.0, -1.0)}
    for h in range(H):
        t[h] = exact[h] if h in exact else (np.cos(2.0 * np.pi * h / H), np.sin(2.0 * np.pi * h / H))
    return t


def heading_moves(H, mode="any"):
    """uint16 [H]: bit k - 9 set iff the translation of code k is allowed at heading h.  "any": all 8; "forward": those whose
    direction index a_k H / 8 is within H / 16 heading steps of h (16 circdist <= H); "both": those or their opposites."""
    if H not in HS:
        raise ValueError("H outside {8, 16, 32, 64}")
    if mode not in ("any", "forward", "both"):
        raise ValueError("mode outside any / forward / both")
    out = np.zeros(H, np.uint16)
    for h in range(H):
        m = 0
        for k, a in ANGLE8.items():
            ok = mode == "any"
            for aa in ((a,) if mode == "forward" else (a, (a + 4) % 8)):
                dd = abs(h - aa * H // 8) % H
                ok = ok or 16 * min(dd, H - dd) <= H
            if ok:
                m |= 1 << (k - 9)
        out[h] = m
    return out


def _shift(a, o, fill, wrap=True):
    """b[s] = a[s + o] for o = (dx, dy, dh): `fill` outside the lattice in x and y; h wraps (wrap=False: `fill`)."""
    dx, dy, dh = o
    H, ny, nx = a.shape
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), constant_values=fill)[:, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    if dh:
        p = np.roll(p, -dh, axis=0).copy()
        if not wrap:
            p[H - 1 if dh > 0 else 0] = fill
    return p


def clearance_grid(dist, shape, origin, step, body, headings, variant=None):
    """D [H, ny, nx] f64 of the body rule at every state."""
    nx, ny = int(shape[0]), int(shape[1])
    H = headings.shape[0]
    X = (F32(origin[0]) + np.arange(nx, dtype=F32) * F32(step)).astype(F64)
    Y = (F32(origin[1]) + np.arange(ny, dtype=F32) * F32(step)).astype(F64)
    px, py = np.tile(X, ny), np.repeat(Y, nx)
    field = (np.ascontiguousarray(dist, F32).ravel(), tuple(shape), tuple(origin), step)
    D = np.zeros((H, ny, nx), F64)
    for h in range(H):
        c, s = np.full(px.size, float(headings[h, 0])), np.full(px.size, float(headings[h, 1]))
        if variant == "cast_first":
            W = body_ref.ball_positions(body, [px, py], c, s)
            best = np.full(px.size, INF, F32)
            off = np.zeros(px.size, bool)
            with np.errstate(invalid="ignore"):
                for j, w in enumerate(W):
                    smp = dfield_ref.sample(field[0], field[1], field[2], step, np.stack(w, axis=1).astype(F32))[:, 0].astype(F32)
                    d = smp - F32(body["rho"][j])
                    off |= np.isnan(d)
                    best = np.where(d < best, d, best)
            D[h] = np.where(off, np.nan, best.astype(F64)).reshape(ny, nx)
        else:
            D[h] = body_ref.body_rule(field, body, [px, py], c, s, "rot_sign" if variant == "rot_sign" else None)[0].reshape(ny, nx)
    return D


def check_opts(step, H, clearance, margin, gain, turn):
    """ValueError for what gpis_pplan_solve refuses with GPIS_ERR_ARG."""
    if H not in HS:
        raise ValueError("H outside {8, 16, 32, 64}")
    v = [float(x) for x in (clearance, margin, gain, turn)]
    if not np.isfinite(v).all() or v[1] < 0 or v[2] < 0 or v[2] > 1e4:
        raise ValueError("a non-finite option, a negative margin or gain, gain > 1e4")
    if not (F32(turn) >= F32(step) / F32(64) and F32(turn) <= F32(1e4) * F32(step)):
        raise ValueError("turn outside [step / 64, 1e4 step]")


class Problem:
    """Free mask, point costs, directed moves and goal states of one solve."""

    def __init__(self, dist, shape, origin, step, body, headings, moves, goals, clearance=0.0, margin=0.0, gain=4.0, turn=None,
                 variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.variant = variant
        self.shape = (int(shape[0]), int(shape[1]))
        self.origin = (float(origin[0]), float(origin[1]))
        self.step = F32(step)
        self.headings = np.ascontiguousarray(headings, F64).reshape(-1, 2)
        self.H = H = self.headings.shape[0]
        turn = self.step if turn is None else turn
        check_opts(step, H, clearance, margin, gain, turn)
        if len(shape) != 2:
            raise ValueError("the pose planner is 2-D")
        if body["m"] == 0 or body["dim"] != 2:
            raise RuntimeError("an empty footprint, or one of dimension 3")
        if not np.isfinite(self.headings).all() or (np.abs(self.headings).sum(axis=1) == 0).any():
            raise ValueError("a heading that is non-finite or (0, 0)")
        self.moves = np.ascontiguousarray(moves, np.uint16).ravel()
        assert self.moves.size == H
        if (self.moves & ~np.uint16(0x1ef)).any():
            raise ValueError("a move bit outside the 8 translations")
        nx, ny = self.shape
        self.n3 = (H, ny, nx)
        self.D = clearance_grid(dist, self.shape, self.origin, step, body, self.headings, variant)
        cl, mg, gn = F32(clearance), F32(margin), F32(gain)
        with np.errstate(all="ignore"):
            d = self.D.astype(F32)
            if variant == "nan_free":
                d = np.where(np.isnan(d), INF, d)
            self.d = d
            self.free = d >= cl
            if mg > 0:
                t = np.maximum(F32(0), mg - (d - cl)) / mg
                c = F32(1) + gn * (t * t)
            else:
                c = np.ones(self.n3, F32)
        self.c = np.where(self.free, c, F32(0)).astype(F32)
        ls = [F32(1) * self.step, np.sqrt(F32(2)) * self.step]
        tw = self.step if variant == "turn_step" else F32(turn)
        self.edges = []                                  # (code, (dx, dy, dh), exists [n3], weight [n3]) in ascending code
        for k, (dx, dy) in TRANSLATIONS:
            bit = (8 - (k - 9)) if variant == "opposite_bit" else (k - 9)
            e = self.free & (((self.moves >> np.uint16(bit)) & np.uint16(1)) == 1)[:, None, None]
            subs = [(dx, dy, 0)] if variant == "no_subset" else [(dx, 0, 0), (0, dy, 0), (dx, dy, 0)]
            for s in subs:
                if s != (0, 0, 0):
                    e = e & _shift(self.free, s, False)
            w = ls[(dx != 0) + (dy != 0) - 1] * (F32(0.5) * (self.c + _shift(self.c, (dx, dy, 0), F32(0))))
            assert w.dtype == F32
            self.edges.append((k, (dx, dy, 0), e, w))
        for k, dh in ((TURN_UP, 1), (TURN_DOWN, -1)):
            wrap = variant != "no_wrap"
            e = self.free & _shift(self.free, (0, 0, dh), False, wrap)
            w = tw * (F32(0.5) * (self.c + _shift(self.c, (0, 0, dh), F32(0), wrap)))
            assert w.dtype == F32
            self.edges.append((k, (0, 0, dh), e, w))
        if variant == "along":                           # the move into s from s - o taken as if it were the move out of s
            self.edges = [(k, (-o[0], -o[1], -o[2]), _shift(e, (-o[0], -o[1], -o[2]), False), _shift(w, (-o[0], -o[1], -o[2]), F32(0)))
                          for k, o, e, w in self.edges]
        g = np.ascontiguousarray(goals, F32).reshape(-1, 3)
        self.goals_given = g.shape[0]
        gh = goal_headings(g[:, 2], H)
        ok, ij = plan_ref.snap(g[:, :2], self.shape, self.origin, self.step)
        self.goal = np.zeros(self.n3, bool)
        self.goals_kept = 0
        self.goals_dropped = 0
        for t in range(g.shape[0]):
            i, j = int(ij[t, 0]), int(ij[t, 1])
            kept = 0
            for h in (range(H) if gh[t] < 0 else (gh[t],)):
                if ok[t] and self.free[h, j, i]:
                    self.goal[h, j, i] = True
                    kept += 1
            self.goals_kept += kept
            self.goals_dropped += kept == 0

    def start_cost(self):
        return np.where(self.goal, F32(0), INF).astype(F32)

    def world(self, ij):
        ij = np.asarray(ij)
        return np.stack([F32(self.origin[a]) + ij[..., a].astype(F32) * self.step for a in range(2)], axis=-1).astype(F32)


def goal_headings(h, H):
    """int headings of the float column h; ValueError unless each is an integer in -1 .. H - 1."""
    h = np.asarray(h, F32).ravel()
    if not np.isfinite(h).all() or (h != np.floor(h)).any() or (h < -1).any() or (h > H - 1).any():
        raise ValueError("a heading index that is not an integer in -1 .. H - 1")
    return h.astype(np.int64)


def solve_sweep(pb):
    """Whole-array relaxations, one move after the other, to the fixed point.  Flat float32 cost."""
    cost = pb.start_cost()
    wrap = pb.variant != "no_wrap"
    while True:
        old = cost.copy()
        for k, o, e, w in pb.edges:
            cand = _shift(cost, o, INF, wrap) + w
            cost = np.where(e & (cand < cost), cand, cost)
        if np.array_equal(old, cost):
            return cost.ravel()


def solve_dijkstra(pb):
    """heapq Dijkstra on the reversed graph with the same float32 additions.  Flat float32 cost."""
    H, ny, nx = pb.n3
    n = H * ny * nx
    idx = np.arange(n).reshape(pb.n3)
    src, dst, wt = [], [], []
    for k, o, e, w in pb.edges:
        s = idx[e]
        hh, r = np.divmod(s, ny * nx)
        src.append(s)
        dst.append(((hh + o[2]) % H) * (ny * nx) + r + o[1] * nx + o[0])
        wt.append(w[e])
    src, dst, wt = np.concatenate(src), np.concatenate(dst), np.concatenate(wt)
    order = np.argsort(dst, kind="stable")
    src, dst, wt = src[order], dst[order], wt[order]
    first = np.searchsorted(dst, np.arange(n + 1))
    cost = pb.start_cost().ravel()
    heap = [(0.0, int(p)) for p in np.flatnonzero(pb.goal.ravel())]
    heapq.heapify(heap)
    done = np.zeros(n, bool)
    while heap:
        d, q = heapq.heappop(heap)
        if done[q] or d > cost[q]:
            continue
        done[q] = True
        for e in range(first[q], first[q + 1]):          # every move s -> q
            s = src[e]
            nd = F32(cost[q] + wt[e])
            if nd < cost[s]:
                cost[s] = nd
                heapq.heappush(heap, (float(nd), int(s)))
    return cost


def policy(pb, cost, br=None):
    """Flat uint8 policy of a converged cost.  br: a dict whose tie_cost (a later code equalled the best value and won by the
    smaller cost[s']) and tie_code (it equalled both and lost to the smaller code) it counts."""
    cst = np.ascontiguousarray(cost, F32).reshape(pb.n3)
    best = np.full(pb.n3, INF, F32)
    bestq = np.full(pb.n3, INF, F32)
    pol = np.full(pb.n3, NONE, np.uint8)
    live = pb.free & np.isfinite(cst) & ~pb.goal
    with np.errstate(invalid="ignore"):
        for k, o, e, w in pb.edges:
            cq = _shift(cst, o, INF)
            v = cq + w
            tie = e & (v == best) & np.isfinite(v)
            take = e & ((v < best) | (tie & (cq < bestq) & (pb.variant != "ties_code")))
            if br is not None:
                br["tie_cost"] = br.get("tie_cost", 0) + int((live & tie & (cq < bestq)).sum())
                br["tie_code"] = br.get("tie_code", 0) + int((live & tie & (cq == bestq)).sum())
            best = np.where(take, v, best)
            bestq = np.where(take, cq, bestq)
            pol = np.where(take, np.uint8(k), pol)
    pol = np.where(pb.free & np.isfinite(cst), pol, np.uint8(NONE))
    pol = np.where(pb.goal, np.uint8(STAY), pol)
    return pol.astype(np.uint8).ravel()


def move_of(code):
    """(dx, dy, dh) of a move code."""
    if code == TURN_UP:
        return 0, 0, 1
    if code == TURN_DOWN:
        return 0, 0, -1
    return (code - 9) % 3 - 1, (code - 9) // 3 - 1, 0


def paths(pb, cost, pol, starts, max_points):
    """(off int64 [m + 1], points f32 [off[m], 2], heading i32 [off[m]], start_cost f32 [m], status u8 [m]) of the policy walks
    from starts [m, 3] = (x, y, h); h = -1: the free heading of least cost at the snapped point (ties: the smaller h; none free:
    status 2 and start cost +inf)."""
    H, ny, nx = pb.n3
    cst = np.ascontiguousarray(cost, F32).ravel()
    pol = np.ascontiguousarray(pol, np.uint8).ravel()
    free = pb.free.ravel()
    st_ = np.ascontiguousarray(starts, F32).reshape(-1, 3)
    sh = goal_headings(st_[:, 2], H)
    ok, ij = plan_ref.snap(st_[:, :2], pb.shape, pb.origin, pb.step)
    m = ok.size
    status = np.zeros(m, np.uint8)
    sc = np.full(m, np.nan, F32)
    cells = []
    for t in range(m):
        pts = []
        if not ok[t]:
            status[t] = 1
        else:
            i, j, h = int(ij[t, 0]), int(ij[t, 1]), int(sh[t])
            if h < 0:
                h, bc = -1, INF
                for hh in range(H):
                    q = (hh * ny + j) * nx + i
                    if free[q] and (h < 0 or cst[q] < bc):
                        h, bc = hh, cst[q]
            if h < 0:
                status[t], sc[t] = 2, INF
            else:
                p = (h * ny + j) * nx + i
                sc[t] = cst[p]
                if not free[p]:
                    status[t] = 2
                elif not np.isfinite(cst[p]):
                    status[t] = 3
                else:
                    pts.append((i, j, h))
                    while pol[p] != STAY:
                        if pol[p] == NONE or len(pts) >= max_points:
                            status[t] = 4
                            break
                        dx, dy, dh = move_of(int(pol[p]))
                        i, j, h = i + dx, j + dy, (h + dh) % H
                        q = (h * ny + j) * nx + i
                        if not cst[q] < cst[p]:
                            status[t] = 4
                            break
                        p = q
                        pts.append((i, j, h))
        cells.append(np.array(pts, np.int64).reshape(-1, 3))
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([c.shape[0] for c in cells])
    allc = np.concatenate(cells) if m else np.zeros((0, 3), np.int64)
    return off, pb.world(allc[:, :2]).reshape(-1, 2), allc[:, 2].astype(np.int32), sc, status


def check_path_invariants(pb, cost, points, heading):
    """Every state of one pose path is free, consecutive states are joined by an existing move, and cost[s_i] ==
    fl(cost[s_i+1] + w) bit for bit (hence strictly cheaper)."""
    cst = np.ascontiguousarray(cost, F32).reshape(pb.n3)
    ok, ij = plan_ref.snap(points, pb.shape, pb.origin, pb.step)
    assert ok.all()
    assert np.array_equal(pb.world(ij[:, :2]).view(np.uint32), np.ascontiguousarray(points, F32).view(np.uint32))
    ed = {o: (e, w) for k, o, e, w in pb.edges}
    S = [(int(h), int(j), int(i)) for (i, j), h in zip(ij[:, :2], heading)]
    for a, b in zip(S[:-1], S[1:]):
        dh = (b[0] - a[0] + pb.H // 2) % pb.H - pb.H // 2
        o = (b[2] - a[2], b[1] - a[1], dh)
        assert o in ed, o
        e, w = ed[o]
        assert e[a] and pb.free[a] and pb.free[b]
        lhs, rhs = cst[a], F32(cst[b] + w[a])
        assert lhs.view(np.uint32) == rhs.view(np.uint32), (a, b, lhs, rhs)
        assert cst[b] < cst[a]
    assert all(pb.free[s] for s in S)


def project(pb, cost):
    """dict(cost2 f32, heading2 u8, c2 f32, policy2 u8 (all flat [ny nx]), free, reachable, max_cost) of a converged cost.
    Asserts that every point of finite positive cost2 has a strictly cheaper 8-neighbour."""
    H, ny, nx = pb.n3
    cst = np.ascontiguousarray(cost, F32).reshape(pb.n3)
    cost2 = cst.min(axis=0)
    heading2 = np.where(np.isfinite(cost2), np.argmax(cst == cost2[None], axis=0), NONE).astype(np.uint8)
    anyfree = pb.free.any(axis=0)
    c2 = np.where(anyfree, np.where(pb.free, pb.c, INF).min(axis=0), F32(0)).astype(F32)
    bestq = np.full((ny, nx), INF, F32)
    pol = np.full((ny, nx), NONE, np.uint8)
    for k, (dx, dy) in TRANSLATIONS:
        cq = _shift(cost2[None], (dx, dy, 0), INF)[0]
        take = cq < bestq
        bestq = np.where(take, cq, bestq)
        pol = np.where(take, np.uint8(k), pol)
    walk = np.isfinite(cost2) & (cost2 > 0)
    assert (bestq[walk] < cost2[walk]).all(), "a point of the projection without a cheaper neighbour"
    pol = np.where(np.isfinite(cost2), pol, np.uint8(NONE))
    pol = np.where(cost2 == 0, np.uint8(STAY), pol).astype(np.uint8)
    fin = np.isfinite(cost2)
    return dict(cost2=cost2.ravel(), heading2=heading2.ravel(), c2=c2.ravel(), policy2=pol.ravel(), free=int(anyfree.sum()),
                reachable=int(fin.sum()), max_cost=F32(cost2[fin].max()) if fin.any() else F32(0))


def greedy_walk(pj, shape, start_ij, limit=None):
    """Follow policy2 from a lattice point; returns the list of (i, j) visited.  Asserts that every step is strictly cheaper."""
    nx, ny = shape
    i, j = start_ij
    out = [(i, j)]
    limit = nx * ny if limit is None else limit
    while pj["policy2"][j * nx + i] != STAY:
        k = int(pj["policy2"][j * nx + i])
        assert k != NONE and len(out) <= limit
        dx, dy, _ = move_of(k)
        assert pj["cost2"][(j + dy) * nx + i + dx] < pj["cost2"][j * nx + i]
        i, j = i + dx, j + dy
        out.append((i, j))
    return out


__all__ = ["heading_table", "heading_moves", "clearance_grid", "check_opts", "Problem", "goal_headings", "solve_sweep", "solve_dijkstra",
           "policy", "move_of", "paths", "check_path_invariants", "project", "greedy_walk", "HS", "VARIANTS", "STAY", "NONE", "TURN_UP",
           "TURN_DOWN", "ANGLE8", "TRANSLATIONS"]
