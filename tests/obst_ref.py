"""Reference for the moving obstacles (csrc/obst.hip, the OBST instantiations of csrc/mppi.hip, gpis_obst_*): a
numpy restatement of the contract, written independently of the product (it imports nothing from gpismap_amd).  The model, the
field's stage cost, the weights and the update are the sampling controller's (tests/mppi_ref.py); the rollout loop is restated
here with one more term, and with no balls it is mppi_ref.rollouts in every bit (tests/test_obst_ref.py holds it to that).

Contract (every floating-point expression is double, written left to right, nothing contracted; / and sqrt are IEEE):
- A set: n balls, 0 <= n <= 256 (discs in 2-D, spheres in 3-D), each a centre c[dim], a velocity v[dim] and a radius r >= 0,
  one epoch (the absolute time at which the centres hold) and the options clearance', margin', w_obs', w_col' (defaults: step,
  4 * step, 1, 100).  Ball i at elapsed time e is at o_a = c_a + v_a * e per axis; at(t) uses e = t - epoch.
- A step at absolute time t_now: E0 = t_now - epoch, once.  In rollout k at step t, after the state update, at the new
  position p:
    e = E0 + ((double)(t + 1) * dt);  q_a = p_a - (c_a + v_a * e);  s2 = q_0 q_0 + q_1 q_1 [+ q_2 q_2] from the first square;
    sep_i = sqrt(s2) - r_i;  D = the minimum over i ascending, from +inf, by (sep_i < D ? sep_i : D)
    j_dyn = w_col' and dyn_hits += 1 if D < clearance'; (w_obs' * r) * r with r = ((clearance' + margin') - D) / margin' if
      D < clearance' + margin'; else 0 (margin' = 0 leaves no band)
    J = ((J + j) + j_dyn) + g
  The term is charged off the lattice too (j is then w_off).  The field's hits keep their meaning.  Per rollout: dyn_hits and
  min_sep, the minimum over t of D from +inf by the same comparison.  The nominal rollout after the update charges the same
  term and reports its own dyn_hits and min_sep; nominal_cost includes it.  Weights, update, tick and shift are mppi_ref's.
- With no set or n = 0 a step is mppi_ref.step; dyn_hits are then 0, min_sep +inf.
- check(): timed trajectories (tests/timing_ref.py) against a set: the closest approach in continuous time while both bodies
  move in straight lines between two samples.  See the function.

The `variant` arguments build the defective variants tests/test_obst_ref.py rejects; None is the contract:
  "time_t" (the ball's time at t instead of t + 1), "no_radius" (sep = sqrt(s2)), "sum_order" (J + (j + j_dyn), then + g),
  "accumulate" (the ball's position accumulated as o += v * dt from its position at E0), "min_first" (D starts from the first
  ball's sep instead of +inf, so a NaN there is never replaced); check()'s are CHECK_VARIANTS."""
import math

import numpy as np

import dfield_ref
import mppi_ref
import pf_ref        # noqa: F401  (the generator behind mppi_ref.noise; imported so that the reference's sources are named here)
import timing_ref
import track_ref     # noqa: F401  (the update's tree)

F32 = np.float32
F64 = np.float64
U64 = np.uint64
MAX_N = 256
OPT_KEYS = ("clearance", "margin", "w_obs", "w_col")
VARIANTS = ("time_t", "no_radius", "sum_order", "accumulate", "min_first")
CHECK_VARIANTS = ("sample_only", "tie_last")


def default_opts(dim, step):
    """The library's defaults (gpis_obst_default_opts) for a field of lattice step `step`."""
    step = float(F32(step))
    return dict(clearance=step, margin=4.0 * step, w_obs=1.0, w_col=100.0)


def check_opts(o):
    """ValueError for what the library answers with GPIS_ERR_ARG."""
    for k in OPT_KEYS:
        if not math.isfinite(float(o[k])) or float(o[k]) < 0.0:
            raise ValueError("a non-finite or negative option: " + k)


def make(dim, centre, velocity, radius, epoch=0.0, step=0.25, check=True, **opts):
    """A set: dict(dim, n, c [n, dim], v [n, dim], r [n], epoch, opts).  ValueError for what gpis_obst_set refuses with
    GPIS_ERR_ARG, OverflowError for GPIS_ERR_LIMIT (check=False: a case feeds the rollouts what the library would refuse)."""
    if dim not in (2, 3):
        raise ValueError("dim outside {2, 3}")
    c = np.asarray(centre, F64).reshape(-1, dim).copy()
    v = np.asarray(velocity, F64).reshape(-1, dim).copy()
    r = np.asarray(radius, F64).ravel().copy()
    if not (c.shape[0] == v.shape[0] == r.size):
        raise ValueError("one row per ball")
    o = default_opts(dim, step)
    o.update(opts)
    if check:
        if r.size > MAX_N:
            raise OverflowError("more than 256 balls")
        if not (np.isfinite(c).all() and np.isfinite(v).all() and np.isfinite(r).all() and math.isfinite(float(epoch))):
            raise ValueError("a non-finite entry")
        if (r < 0).any():
            raise ValueError("a negative radius")
        check_opts(o)
    return dict(dim=dim, n=int(r.size), c=c, v=v, r=r, epoch=float(epoch), opts=o)


def at(S, t):
    """The centres [n, dim] at absolute time t."""
    e = float(t) - S["epoch"]
    return S["c"] + S["v"] * e


def rollouts(dist, shape, origin, step, start, Ubar, z, o, cost=None, goal=None, variant=None, states=False, obst=None, t_now=0.0):
    """mppi_ref.rollouts with the balls' term: the same arguments and the same dict, with dyn_hits [m] int32 and min_sep [m]
    added, and the counters dyn_col, dyn_band, dyn_free, dyn_off (the term charged at a position off the lattice), second_nearer
    (a step at which a ball after the first lowered D) and tie (a step at which a later ball's sep equalled D).  `variant` is
    one of this module's; mppi_ref's own variants are not restated."""
    assert (cost is None) != (goal is None)
    dim = len(shape)
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    m = z.shape[0]
    dt, gamma = float(o["dt"]), float(o["gamma"])
    sig, lo, hi = ([float(v) for v in o[k]] for k in ("sigma", "umin", "umax"))
    clr, mar = float(o["clearance"]), float(o["margin"])
    w_obs, w_col, w_off, w_goal = (float(o[k]) for k in ("w_obs", "w_col", "w_off", "w_goal"))
    n = 0 if obst is None else obst["n"]
    if n:
        assert obst["dim"] == dim
        oc, ov, orad = obst["c"], obst["v"], obst["r"]
        dclr, dmar, dw_obs, dw_col = (float(obst["opts"][k]) for k in OPT_KEYS)
        E0 = float(t_now) - obst["epoch"]
        acc_o = oc + ov * E0                             # (the "accumulate" variant's running position)
    pos = [np.full(m, float(start[a]), F64) for a in range(dim)]
    c, s = np.full(m, float(start[dim]), F64), np.full(m, float(start[dim + 1]), F64)
    J = np.zeros(m, F64)
    hits = np.zeros(m, np.int32)
    dyn_hits = np.zeros(m, np.int32)
    min_sep = np.full(m, np.inf, F64)
    d = np.zeros((m, T, U), F64)
    br = dict(off=0, col=0, band=0, free=0, clamped=0, dyn_col=0, dyn_band=0, dyn_free=0, dyn_off=0, second_nearer=0, tie=0)
    hist = [np.stack(pos + [c, s], axis=1)] if states else None
    half = 0.5 * dt
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            v = []
            for u in range(U):
                ub = float(Ubar[t, u])
                e = sig[u] * z[:, t, u]
                vu = np.minimum(np.maximum(ub + e, lo[u]), hi[u])
                br["clamped"] += int(np.count_nonzero(vu != ub + e))
                d[:, t, u] = vu - ub
                v.append(vu)
            a = half * v[U - 1]
            den = 1.0 + a * a
            cn = (1.0 - a * a) / den
            sn = (a + a) / den
            c1, s1 = c * cn - s * sn, s * cn + c * sn
            nn = np.sqrt(c1 * c1 + s1 * s1)
            c1, s1 = c1 / nn, s1 / nn
            bx = v[0] * dt
            if dim == 2:
                pos = [pos[0] + c * bx, pos[1] + s * bx]
            else:
                by = v[1] * dt
                pos = [pos[0] + (c * bx - s * by), pos[1] + (s * bx + c * by), pos[2] + v[2] * dt]
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
            if not n:
                J = (J + j) + g
                continue
            # the moving balls' term
            e = E0 + (float(t if variant == "time_t" else t + 1) * dt)
            if variant == "accumulate":
                acc_o = acc_o + ov * dt
            D = np.full(m, np.inf, F64)
            for i in range(n):
                ob = acc_o[i] if variant == "accumulate" else [float(oc[i, b]) + float(ov[i, b]) * e for b in range(dim)]
                q = pos[0] - ob[0]
                s2 = q * q
                for b in range(1, dim):
                    q = pos[b] - ob[b]
                    s2 = s2 + q * q
                sep = np.sqrt(s2) if variant == "no_radius" else np.sqrt(s2) - float(orad[i])
                if i == 0 and variant == "min_first":
                    D = sep
                    continue
                if i > 0:
                    br["second_nearer"] += int((sep < D).sum()); br["tie"] += int((sep == D).sum())
                D = np.where(sep < D, sep, D)
            dcol = D < dclr
            dband = ~dcol & (D < dclr + dmar)
            rr = ((dclr + dmar) - D) / dmar if dmar > 0.0 else np.zeros(m)
            jd = np.where(dcol, dw_col, np.where(dband, (dw_obs * rr) * rr, 0.0))
            dyn_hits += dcol.astype(np.int32)
            min_sep = np.where(D < min_sep, D, min_sep)
            br["dyn_col"] += int(dcol.sum()); br["dyn_band"] += int(dband.sum()); br["dyn_free"] += int((~dcol & ~dband).sum())
            br["dyn_off"] += int((off & (dcol | dband)).sum())
            J = (J + (j + jd)) + g if variant == "sum_order" else ((J + j) + jd) + g
    if cost is not None:
        uu, ok = mppi_ref.lattice_coord(np.stack(pos, axis=1).astype(F32), shape, origin, step)
        idx = np.zeros(m, np.int64)
        stride = 1
        for a in range(dim):
            ua = np.where(ok, uu[a], F32(0))
            ia = np.floor((ua + F32(0.5)).astype(F32)).astype(np.int64)
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
    out = dict(J=J, hits=hits, d=d, branches=br, dyn_hits=dyn_hits, min_sep=min_sep)
    if states:
        out["states"] = np.stack(hist, axis=1)
    return out


def roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0):
    """mppi_ref.roll with the set: the K rollouts and the reference's own weights."""
    dim = len(shape)
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    z = mppi_ref.noise(seed, tick, np.arange(K, dtype=U64), Ubar.shape[0], U)
    r = rollouts(dist, shape, origin, step_, mppi_ref.start_state(pose, dim), Ubar, z, o, cost, goal, variant, obst=obst, t_now=t_now)
    r.update(q=mppi_ref.weights(r["J"], o["lam"]), Jmin=float(r["J"].min()), best=mppi_ref.best_index(r["J"]))
    return r


def finish(r, q, dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0):
    """mppi_ref.finish with the set: the nominal rollout charges the term; adds ndyn (rollouts with dyn_hits > 0),
    nominal_dyn_hits and nominal_min_sep."""
    dim = len(shape)
    U = mppi_ref.ncontrols(dim)
    Ubar = np.asarray(Ubar, F64).reshape(-1, U)
    T = Ubar.shape[0]
    q = np.asarray(q, U64)
    Tq, Th, S2 = pf_ref.totals(q)
    Un = mppi_ref.update(Ubar, q, r["d"], o)
    nom = rollouts(dist, shape, origin, step_, mppi_ref.start_state(pose, dim), Un, np.zeros((1, T, U), F64), o, cost, goal, variant,
                   states=True, obst=obst, t_now=t_now)
    return dict(T=Tq, Th=Th, S2=S2, neff=pf_ref.neff(Th, S2), nhit=int(np.count_nonzero(r["hits"])), U=Un, u0=Un[0].copy(),
                nominal_states=nom["states"][0], nominal_cost=float(nom["J"][0]), nominal_hits=int(nom["hits"][0]),
                ndyn=int(np.count_nonzero(r["dyn_hits"])), nominal_dyn_hits=int(nom["dyn_hits"][0]),
                nominal_min_sep=float(nom["min_sep"][0]))


def step(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost=None, goal=None, variant=None, obst=None, t_now=0.0):
    """One controller step that sees the set: roll's and finish's dicts merged."""
    r = roll(dist, shape, origin, step_, pose, Ubar, seed, tick, K, o, cost, goal, variant, obst, t_now)
    r.update(finish(r, r["q"], dist, shape, origin, step_, pose, Ubar, seed, tick, o, cost, goal, variant, obst, t_now))
    return r


def check(x, v, t, tstatus, S, dt, steps, t0=0.0, t_begin=0.0, clearance=None, variant=None, trace=None):
    """Timed trajectories (x [m, N, dim] f32 with the timing v, t [m, N] f32 and its status [m], as timing_ref.time gives them)
    against the set S.  t_begin: the absolute time at which trajectory time 0 happens.  For each trajectory of timing status 0:
      for k = 0 .. steps: tau_k = t0 + (double)k * dt;  p_k = timing_ref.position (the robot rests at x_{N-1} after the
        duration);  e_k = (t_begin - epoch) + tau_k;  o_{i,k} = c_i + v_i * e_k
      for each interval k = 0 .. steps - 1 and ball i, ascending:
        a = p_k - o_{i,k};  b = (p_{k+1} - p_k) - (o_{i,k+1} - o_{i,k});  bb = sum_a b_a b_a;  ab = sum_a a_a b_a (axis order
        from the first product);  s = 0 unless bb > 0, else x = (-ab) / bb, s = (x > 0 ? x : 0), s = (s < 1 ? s : 1);
        q = a + s * b;  sep = sqrt(sum_a q_a q_a) - r_i
    Returns dict(min_sep [m] f64: the least sep by a strict comparison from +inf (ties: the smallest (k, i)), min_time =
    tau_k + s * dt, min_obstacle i, first_hit: the smallest k with some sep < clearance else -1, collides) -- the three
    integer arrays int32.  n = 0: +inf, NaN, -1, -1, 0; timing status 2 or 3: NaN, NaN, -1, -1, 0.  clearance None: the set's.
    Variants: "sample_only" (s forced to 0), "tie_last" (ties to the largest (k, i)).  trace counts rest (an interval after the
    duration), bb0 (bb = 0), inner (0 < s < 1)."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    steps = int(steps)
    clearance = S["opts"]["clearance"] if clearance is None else clearance
    args = (dt, t0, t_begin, clearance)
    if not (all(math.isfinite(float(a)) for a in args) and 1 <= steps <= 4096 and dt > 0 and t0 >= 0 and clearance >= 0):
        raise ValueError("bad arguments")
    if S["dim"] != dim:
        raise ValueError("a set of another dim")
    dt, t0, clearance = F64(dt), F64(t0), F64(clearance)
    TB = F64(t_begin) - F64(S["epoch"])
    out = dict(min_sep=np.full(m, np.nan, F64), min_time=np.full(m, np.nan, F64), min_obstacle=np.full(m, -1, np.int32),
               first_hit=np.full(m, -1, np.int32), collides=np.zeros(m, np.int32))
    n = S["n"]
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0:
                continue
            out["min_sep"][r] = np.inf
            if n == 0:
                continue
            xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
            tau = [t0 + F64(k) * dt for k in range(steps + 1)]
            p = np.stack([timing_ref.position(xs, vs, ts, tk) for tk in tau])                   # [steps + 1, dim]
            e = np.array([TB + tk for tk in tau], F64)
            o = S["c"][None, :, :] + S["v"][None, :, :] * e[:, None, None]                      # [steps + 1, n, dim]
            A = p[:-1, None, :] - o[:-1]                                                        # [steps, n, dim]
            B = (p[1:] - p[:-1])[:, None, :] - (o[1:] - o[:-1])
            bb, ab = B[..., 0] * B[..., 0], A[..., 0] * B[..., 0]
            for a in range(1, dim):
                bb = bb + B[..., a] * B[..., a]
                ab = ab + A[..., a] * B[..., a]
            xx = (-ab) / np.where(bb > 0, bb, F64(1.0))
            s = np.where(xx > 0, xx, F64(0.0))
            s = np.where(s < 1, s, F64(1.0))
            s = np.where(bb > 0, s, F64(0.0))
            if variant == "sample_only":
                s = np.zeros_like(s)
            q = A[..., 0] + s * B[..., 0]
            s2 = q * q
            for a in range(1, dim):
                q = A[..., a] + s * B[..., a]
                s2 = s2 + q * q
            sep = np.sqrt(s2) - S["r"][None, :]                                                 # [steps, n]
            best, bk, bi = F64(np.inf), -1, -1
            # the strict comparison from +inf over k ascending, then i: a NaN and +inf are never taken, the first of equals stays
            flat = np.where(np.isnan(sep), np.inf, sep).ravel()
            if flat.min() < np.inf:
                same = np.flatnonzero(flat == flat.min())
                idx = int(same[-1] if variant == "tie_last" else same[0])
                best, bk, bi = flat[idx], idx // n, idx % n
            out["min_sep"][r] = best
            if bk >= 0:
                out["min_time"][r] = tau[bk] + s[bk, bi] * dt
                out["min_obstacle"][r] = bi
            hit = np.flatnonzero((sep < clearance).any(axis=1))
            if hit.size:
                out["first_hit"][r], out["collides"][r] = int(hit[0]), 1
            if trace is not None:
                trace["rest"] = trace.get("rest", 0) + int(sum(1 for tk in tau[:-1] if tk >= ts[N - 1]))
                trace["bb0"] = trace.get("bb0", 0) + int((bb == 0).sum())
                trace["inner"] = trace.get("inner", 0) + int(((s > 0) & (s < 1)).sum())
    return out


class Controller(mppi_ref.Controller):
    """mppi_ref.Controller whose step takes a set and the absolute time."""

    def step(self, dist, shape, origin, step_, pose, o, cost=None, goal=None, obst=None, t_now=0.0):
        mppi_ref.check_opts(o, self.dim)
        if not math.isfinite(float(t_now)) or (obst is not None and obst["dim"] != self.dim):
            raise ValueError("a non-finite time or a set of another dim")
        self.tick += 1
        self.last = step(dist, shape, origin, step_, pose, self.U, self.seed, self.tick, self.K, o, cost, goal, None, obst, t_now)
        self.U = self.last["U"]
        return self.last["u0"], self.last


__all__ = ["default_opts", "check_opts", "make", "at", "rollouts", "roll", "finish", "step", "check", "Controller", "MAX_N", "OPT_KEYS", "VARIANTS",
           "CHECK_VARIANTS"]
