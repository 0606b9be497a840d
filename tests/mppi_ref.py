"""Reference for the sampling controller (csrc/mppi.hip, gpis_mppi_*): a numpy restatement of the contract,
written independently of the product (it imports nothing from gpismap_amd).  The generator and the deviate are the particle
filter's (tests/pf_ref.py), the field sample is the distance field's (tests/dfield_ref.py), the update's sum is the tracker's
tree (tests/track_ref.py); what is stated here is the model, the costs, the weights and the update of the nominal sequence.

Contract (every floating-point expression is double, written left to right, nothing contracted; division and sqrt are IEEE;
the field sample is float32 exactly as dfield_ref.sample, taken at the float32 cast of the position):
- Model, by the field's dim.  dim 2: state (x, y, c, s), U = 2 controls (v, w): a unicycle.  dim 3: state (x, y, z, c, s),
  U = 4 controls (vx, vy, vz, w): body-frame velocity and yaw rate about z.
- Controller state: the nominal sequence Ubar [T][U] (zero after init), a uint32 tick (0 after init), the uint64 seed, K
  rollouts (1 .. 65536) and T steps (1 .. 256).
- Noise: Philox4x32-10 keyed (seed & 0xffffffff, seed >> 32) on the counter (k, tick, t * U + u, 2); tags 0 and 1 are the
  filter's.  One block gives one deviate z by pf_ref.deviates' formula.  Rollout 0 has z = 0 throughout: the nominal itself.
- step(pose, goal): tick += 1; the start is pose [t, R]'s translation and (c, s) = (R[0], R[1]) / sqrt(R[0] R[0] + R[1] R[1]).
  For rollout k and t = 0 .. T - 1:
    e = sigma[u] * z;  v_u = min(max(Ubar[t][u] + e, umin[u]), umax[u]);  d_u = v_u - Ubar[t][u]
    translation with the heading from before the step:
      dim 2: bx = v0 * dt;  x += c * bx;  y += s * bx
      dim 3: bx = v0 * dt;  by = v1 * dt;  x += c * bx - s * by;  y += s * bx + c * by;  z += v2 * dt
    heading: a = (0.5 * dt) * w;  den = 1 + a a;  cn = (1 - a a) / den;  sn = (a + a) / den;
      (c, s) <- (c cn - s sn, s cn + c sn), each divided by n = sqrt(c c + s s) of the new pair
    stage cost j of d, the sampled distance at the new position: NaN (off the lattice) -> w_off; d < clearance -> w_col and
      hits += 1; d < clearance + margin -> r = ((clearance + margin) - d) / margin, j = (w_obs * r) * r; else 0
    control cost: g = gamma * sum over the u with sigma[u] > 0, ascending, of (Ubar[t][u] * d_u) / (sigma[u] * sigma[u])
      (the sum starts from 0.0)
    J = (J + j) + g
  Terminal term with a planner's cost-to-go `cost` on the field's lattice: per axis u_a = the sampler's float32 lattice
  coordinate ((float)p_a - origin_a) / step with the same inside test; i_a = min((int)floorf(u_a + 0.5f), n_a - 1);
  G = cost[i]; off the lattice -> J += w_off; G infinite -> J += w_col; else J += w_goal * (double)G.
  With a goal point instead: J += w_goal * sqrt(sum_a (p_a - g_a)^2), the sum in axis order from the first square.
- Weights: Jmin = min J; q_k = (uint64)floor(exp(-((J_k - Jmin) / lambda)) * 2^32) (the one inexact step: both exp are within
  1 ulp and 2^32 * 2^-51 < 1, so two implementations differ by at most 1 in q); T_q = sum q, Th = sum (q >> 16),
  S2 = sum (q >> 16)^2 as integers; neff = (double)Th * (double)Th / (double)S2; best = the lowest index of minimal J;
  hits = the number of rollouts with a hit count > 0.
- Update: S[t][u] = sum_k (double)q_k * d_u[k][t] by track_ref.tree_sum (256-rollout segments by the halving tree, the
  partials zero-padded to a power of two, the same tree); Ubar[t][u] = min(max(Ubar[t][u] + S[t][u] / (double)T_q, umin[u]),
  umax[u]).  Then the nominal rollout: rollout 0 (z = 0) of the new Ubar by the same code: its T + 1 states, its cost and its
  hit count.  u0 = the new Ubar[0].
- shift(): Ubar[t] = Ubar[t + 1]; the last row stays; the tick does not change.

The `variant` arguments build the defective variants tests/test_mppi_ref.py rejects; None is the contract."""
import math

import numpy as np

import dfield_ref
import pf_ref
import track_ref

F32 = np.float32
F64 = np.float64
U64 = np.uint64
TWO32 = 4294967296.0
MAX_K = 65536
MAX_T = 256
TAG = 2
OPT_KEYS = ("dt", "lam", "gamma", "sigma", "umin", "umax", "clearance", "margin", "w_obs", "w_col", "w_off", "w_goal")


def ncontrols(dim):
    return 4 if dim == 3 else 2


def default_opts(dim, step):
    """The library's defaults (gpis_mppi_default_opts) for a field of lattice step `step`; `lam` is the C field `lambda`."""
    step = float(F32(step))
    o = dict(dt=0.1, lam=1.0, gamma=0.1, clearance=step, margin=2.0 * step, w_obs=1.0, w_col=100.0, w_off=100.0, w_goal=1.0)
    if dim == 3:
        o.update(sigma=(0.25, 0.25, 0.25, 0.5), umin=(-1.0, -1.0, -1.0, -1.0), umax=(1.0, 1.0, 1.0, 1.0))
    else:
        o.update(sigma=(0.25, 0.5, 0.0, 0.0), umin=(0.0, -1.0, 0.0, 0.0), umax=(1.0, 1.0, 0.0, 0.0))
    return o


def check_opts(o, dim):
    """ValueError for what the library answers with GPIS_ERR_ARG."""
    flat = [o[k] for k in ("dt", "lam", "gamma", "clearance", "margin", "w_obs", "w_col", "w_off", "w_goal")]
    flat += list(o["sigma"]) + list(o["umin"]) + list(o["umax"])
    if not all(math.isfinite(float(v)) for v in flat):
        raise ValueError("a non-finite option")
    if o["dt"] <= 0 or o["lam"] <= 0:
        raise ValueError("dt and lambda must be positive")
    if min(o["sigma"]) < 0 or o["margin"] < 0 or min(o[k] for k in ("w_obs", "w_col", "w_off", "w_goal")) < 0:
        raise ValueError("a negative sigma, weight or margin")
    if any(a > b for a, b in zip(o["umin"], o["umax"])):
        raise ValueError("umin above umax")


def start_state(pose, dim):
    """(x, y[, z], c, s) of a pose [t, R] (6 / 12 doubles): the heading is (R[0], R[1]) divided by its norm."""
    p = np.asarray(pose, F64).ravel()
    r0, r1 = float(p[dim]), float(p[dim + 1])
    n = math.sqrt(r0 * r0 + r1 * r1)
    return np.array([float(v) for v in p[:dim]] + [r0 / n, r1 / n], F64)


def pose_of_state(st, dim):
    """The pose [t, R] of a state: what the next step() takes (3-D: a rotation about z)."""
    st = np.asarray(st, F64)
    c, s = float(st[dim]), float(st[dim + 1])
    if dim == 2:
        return np.array([st[0], st[1], c, s, -s, c], F64)
    return np.array([st[0], st[1], st[2], c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0], F64)


def noise(seed, tick, ks, T, U, variant=None):
    """z [len(ks), T, U] float64: the deviates of the rollouts `ks` at `tick`; rollout 0's are zero."""
    ks = np.asarray(ks, U64)
    z = np.zeros((ks.size, T, U), F64)
    for t in range(T):
        for u in range(U):
            ctr = u * T + t if variant == "counter" else t * U + u
            z[:, t, u] = pf_ref.deviates(seed, ks, tick, ctr, tag=TAG)
    if variant != "noisy0":
        z[ks == U64(0)] = 0.0
    return z


def lattice_coord(p32, shape, origin, step):
    """(u [dim] of float32 arrays, inside): the sampler's lattice coordinates of float32 points [m, dim] and its inside test."""
    st = F32(step)
    u = [((p32[:, a] - F32(origin[a])) / st).astype(F32) for a in range(len(shape))]
    ok = np.ones(p32.shape[0], bool)
    for a in range(len(shape)):
        ok &= (u[a] >= 0) & (u[a] <= F32(shape[a] - 1))
    return u, ok


def rollouts(dist, shape, origin, step, start, Ubar, z, o, cost=None, goal=None, variant=None, states=False):
    """The rollouts of the deviates z [m, T, U] from `start` (start_state's) around Ubar [T, U].  Returns dict(J [m], hits [m]
    int32, d [m, T, U], branches: how many stage costs took each branch, terminal branches; states [m, T + 1, dim + 2] if
    asked).  Exactly one of `cost` (the planner's cost-to-go, flat, x fastest) and `goal` [dim] is given."""
    assert (cost is None) != (goal is None)
    dim = len(shape)
    U = ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    m = z.shape[0]
    dt, gamma = float(o["dt"]), float(o["gamma"])
    sig, lo, hi = ([float(v) for v in o[k]] for k in ("sigma", "umin", "umax"))
    clr, mar = float(o["clearance"]), float(o["margin"])
    w_obs, w_col, w_off, w_goal = (float(o[k]) for k in ("w_obs", "w_col", "w_off", "w_goal"))
    pos = [np.full(m, float(start[a]), F64) for a in range(dim)]
    c, s = np.full(m, float(start[dim]), F64), np.full(m, float(start[dim + 1]), F64)
    J = np.zeros(m, F64)
    hits = np.zeros(m, np.int32)
    d = np.zeros((m, T, U), F64)
    br = dict(off=0, col=0, band=0, free=0, clamped=0)
    hist = [np.stack(pos + [c, s], axis=1)] if states else None
    half = 0.5 * dt
    with np.errstate(invalid="ignore"):
        for t in range(T):
            v = []
            for u in range(U):
                ub = float(Ubar[t, u])
                e = sig[u] * z[:, t, u]
                vu = np.minimum(np.maximum(ub + e, lo[u]), hi[u])
                du = vu - ub
                br["clamped"] += int(np.count_nonzero(vu != ub + e))
                d[:, t, u] = e if variant == "unclamped_d" else du
                v.append(vu)
            w = v[U - 1]
            a = half * w
            den = 1.0 + a * a
            cn = (1.0 - a * a) / den
            sn = (a + a) / den
            c1, s1 = c * cn - s * sn, s * cn + c * sn
            n = np.sqrt(c1 * c1 + s1 * s1)
            c1, s1 = c1 / n, s1 / n
            ch, sh = (c1, s1) if variant == "heading_first" else (c, s)
            bx = v[0] * dt
            if dim == 2:
                pos = [pos[0] + ch * bx, pos[1] + sh * bx]
            else:
                by = v[1] * dt
                pos = [pos[0] + (ch * bx - sh * by), pos[1] + (sh * bx + ch * by), pos[2] + v[2] * dt]
            c, s = c1, s1
            if states:
                hist.append(np.stack(pos + [c, s], axis=1))
            dd = dfield_ref.sample(dist, shape, origin, step, np.stack(pos, axis=1).astype(F32))[:, 0].astype(F64)
            off = np.isnan(dd)
            col = ~off & (dd < clr)
            band = ~off & ~col & (dd < clr + mar)
            r = ((clr + mar) - dd) / mar if mar > 0.0 else np.zeros(m)
            j = np.where(off, w_off, np.where(col, w_col, np.where(band, (w_obs * r) * r, 0.0)))
            hits += col.astype(np.int32)
            br["off"] += int(off.sum()); br["col"] += int(col.sum()); br["band"] += int(band.sum())
            br["free"] += int((~off & ~col & ~band).sum())
            acc = np.zeros(m, F64)
            for u in range(U):
                if sig[u] > 0.0:
                    acc = acc + (float(Ubar[t, u]) * d[:, t, u]) / (sig[u] * sig[u])
            g = gamma * acc
            J = J + (j + g) if variant == "sum_order" else (J + j) + g
    if cost is not None:
        uu, ok = lattice_coord(np.stack(pos, axis=1).astype(F32), shape, origin, step)
        idx = np.zeros(m, np.int64)
        stride = 1
        for a in range(dim):
            ua = np.where(ok, uu[a], F32(0))
            ia = np.floor(ua).astype(np.int64) if variant == "floor_index" else np.floor((ua + F32(0.5)).astype(F32)).astype(np.int64)
            idx += np.minimum(ia, shape[a] - 1) * stride
            stride *= shape[a]
        G = np.asarray(cost, F32).ravel()[idx]
        blocked = ok & np.isinf(G)
        term = np.where(~ok, w_off, np.where(blocked, w_col, w_goal * np.where(blocked, F32(0), G).astype(F64)))
        br.update(term_off=int((~ok).sum()), term_blocked=int(blocked.sum()), term_cost=int((ok & ~blocked).sum()))
    else:
        gg = [float(v) for v in np.asarray(goal, F64).ravel()[:dim]]
        s2 = (pos[0] - gg[0]) * (pos[0] - gg[0])
        for a in range(1, dim):
            s2 = s2 + (pos[a] - gg[a]) * (pos[a] - gg[a])
        term = w_goal * np.sqrt(s2)
        br.update(term_goal=m)
    J = J + term
    out = dict(J=J, hits=hits, d=d, branches=br)
    if states:
        out["states"] = np.stack(hist, axis=1)
    return out


def weights(J, lam):
    """q [K] uint64 of the rollout costs."""
    w = np.exp(-((J - J.min()) / float(lam))) * TWO32
    return np.floor(w).astype(U64)


def best_index(J):
    """The lowest index of minimal J."""
    return int(np.argmin(J))


def update(Ubar, q, d, o, variant=None):
    """The new nominal sequence [T, U] from the weights q [K] and the clamped perturbations d [K, T, U]."""
    K, T, U = d.shape
    terms = q.astype(F64)[:, None] * d.reshape(K, T * U)
    if variant == "flat_sum":
        S = np.zeros(T * U, F64)
        for k in range(K):
            S = S + terms[k]
    else:
        S = track_ref.tree_sum(terms)
    Tq = float(pf_ref.totals(q)[0])
    lo, hi = np.array(o["umin"], F64)[:U], np.array(o["umax"], F64)[:U]
    return np.minimum(np.maximum(np.asarray(Ubar, F64).reshape(T, U) + S.reshape(T, U) / Tq, lo), hi)


def roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None):
    """The first half of a step at `tick` (the tick after its increment): the K rollouts around Ubar [T, U] and the
    reference's own weights.  Returns rollouts()' dict with q, Jmin and best added."""
    dim = len(shape)
    U = ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    z = noise(seed, tick, np.arange(K, dtype=U64), Ubar.shape[0], U, variant)
    r = rollouts(dist, shape, origin, step_, start_state(pose, dim), Ubar, z, o, cost, goal, variant)
    r.update(q=weights(r["J"], o["lam"]), Jmin=float(r["J"].min()), best=best_index(r["J"]))
    return r


def finish(r, q, dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost=None, goal=None, variant=None):
    """The second half from the weights q (the reference's own, or a device's): dict(T, Th, S2, neff, nhit, U (the new
    sequence), u0, nominal_states [T + 1, dim + 2], nominal_cost, nominal_hits)."""
    dim = len(shape)
    U = ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    q = np.asarray(q, U64)
    Tq, Th, S2 = pf_ref.totals(q)
    Un = update(Ubar, q, r["d"], o, variant)
    nz = np.zeros((1, T, U), F64) if variant != "noisy0" else noise(seed, tick, np.zeros(1, U64), T, U, variant)
    nom = rollouts(dist, shape, origin, step_, start_state(pose, dim), Un, nz, o, cost, goal, variant, states=True)
    return dict(T=Tq, Th=Th, S2=S2, neff=pf_ref.neff(Th, S2), nhit=int(np.count_nonzero(r["hits"])), U=Un, u0=Un[0].copy(),
                nominal_states=nom["states"][0], nominal_cost=float(nom["J"][0]), nominal_hits=int(nom["hits"][0]))


def step(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None):
    """One controller step at `tick` (the tick after its increment) from the nominal sequence Ubar [T, U]: roll's and finish's
    dicts merged."""
    r = roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost, goal, variant)
    r.update(finish(r, r["q"], dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost, goal, variant))
    return r


def shift(Ubar):
    Ubar = np.asarray(Ubar, F64)
    return np.concatenate([Ubar[1:], Ubar[-1:]], axis=0)


def advance(state, u, dim, dt):
    """The model applied once to one state with the control u (no noise, no clamp): what a closed loop does with u0."""
    z = np.zeros((1, 1, ncontrols(dim)), F64)
    o = dict(dt=dt, gamma=0.0, sigma=(0.0,) * 4, umin=(-np.inf,) * 4, umax=(np.inf,) * 4, clearance=0.0, margin=0.0, w_obs=0.0,
             w_col=0.0, w_off=0.0, w_goal=0.0)
    shape = (2,) * dim
    r = rollouts(np.zeros(2 ** dim, F32), shape, (0.0,) * dim, 1.0, state, np.asarray(u, F64)[None, :ncontrols(dim)], z, o,
                 goal=np.zeros(dim), states=True)
    return r["states"][0, 1]


class Controller:
    """The whole contract as an object: what the library's controller does, call by call."""

    def __init__(self, dim, K, T, seed=0):
        if not (1 <= K <= MAX_K and 1 <= T <= MAX_T):
            raise ValueError("K or T beyond the limits")
        self.dim, self.K, self.T, self.seed, self.tick = dim, int(K), int(T), int(seed), 0
        self.U = np.zeros((self.T, ncontrols(dim)), F64)
        self.last = None

    def set_nominal(self, U):
        self.U = np.asarray(U, F64).reshape(self.T, ncontrols(self.dim)).copy()

    def step(self, dist, shape, origin, step_, pose, o, cost=None, goal=None):
        check_opts(o, self.dim)
        self.tick += 1
        self.last = step(dist, shape, origin, step_, pose, self.U, self.seed, self.tick, self.K, o, cost, goal)
        self.U = self.last["U"]
        return self.last["u0"], self.last

    def shift(self):
        self.U = shift(self.U)


__all__ = ["default_opts", "check_opts", "ncontrols", "start_state", "pose_of_state", "noise", "lattice_coord", "rollouts",
           "weights", "best_index", "update", "roll", "finish", "step", "shift", "advance", "Controller", "MAX_K", "MAX_T", "TAG", "OPT_KEYS"]
