"""numpy reference of the time parametrisation and of the control sequences it gives (csrc/traj.hip, gpis_timing_*, DESIGN.md
§7p), written from the contract.  It imports nothing from the product.

Stage 1, time(): float32 without FMA, vectorised over the batch; only the prefixes and the j loop of the envelope are Python
loops.  Per trajectory of N waypoints x_0 .. x_{N-1} with the limits o (OPT_NAMES):
- ds_i = |x_{i+1} - x_i| (sqrtf of squares summed left to right), S_0 = 0, S_i = S_{i-1} + ds_{i-1} ascending.
- kappa_i = (2 |a x b|) / ((|a| |b|) |c|) at interior waypoints, a = x_i - x_{i-1}, b = x_{i+1} - x_i, c = x_{i+1} - x_{i-1}; the
  cross product is (a_0 b_1) - (a_1 b_0), its absolute value, in 2-D and ((a_1 b_2) - (a_2 b_1), (a_2 b_0) - (a_0 b_2),
  (a_0 b_1) - (a_1 b_0)) with the contract's norm in 3-D; 0 where the denominator is 0 and at both ends.
- Slow-down with a field and slow_dist > 0: d = the field's sample at x_i; not finite: no limit; e = d - clearance <= 0: v_min;
  else v_min + (v_max - v_min) * min(e / slow_dist, 1).
- L_i: v_max v_max (code 0); with kappa_i != 0: a_lat / kappa_i if a_lat > 0 (1), (w_max / kappa_i) squared if w_max > 0 (2);
  the slow-down speed squared (3); each replaces the value only where strictly smaller, in this order.  Interior waypoints
  below v_min v_min are raised to it (4).  Then L_0 takes v_start v_start and L_{N-1} takes v_end v_end where strictly smaller (5).
- u_i = the minimum of L_i, of L_j + (2 a_max) (S_i - S_j) over j < i (6) and of L_j + (2 d_max) (S_j - S_i) over j > i (7); the
  limiter byte is L_i's code unless a cone is strictly smaller, the acceleration cone before the braking cone.  v_i = sqrtf(u_i).
- dt_i = 0 where ds_i = 0, else (2 ds_i) / (v_i + v_{i+1}); t_0 = 0, t_{i+1} = t_i + dt_i ascending.  Status 0, 3 where a dt_i is
  not finite (the times stay as computed), 2 for a trajectory without input (NaN v, t and summaries, limiter bytes and counts 0).

Stage 2, controls(): double, left to right, plain loops; the float32 x, v, t are cast first.  See the function.

`variant` selects one of the deliberately defective forms (VARIANTS) that tests/test_timing_ref.py must tell from the contract."""
from fractions import Fraction

import numpy as np

import dfield_ref

F32 = np.float32
F64 = np.float64
VARIANTS = ("sweeps", "npsum", "search_lt", "heading_after", "fused_s")
OPT_NAMES = ("v_max", "v_min", "a_max", "d_max", "a_lat", "w_max", "v_start", "v_end", "clearance", "slow_dist")
CODES = ("v_max", "a_lat", "w_max", "clearance", "v_min", "end", "accelerate", "brake")
MAX_T = 256


def default_opts(dim, step):
    """The documented defaults of gpis_timing_default_opts: the controller's default command limits (§7l: v <= 1, |w| <= 1), its
    clearance, and a slow-down band of four lattice steps."""
    s = F32(step)
    return dict(v_max=F32(1), v_min=F32(0.05), a_max=F32(0.5), d_max=F32(0.5), a_lat=F32(0.5), w_max=F32(1), v_start=F32(0),
                v_end=F32(0), clearance=s, slow_dist=F32(4) * s)


def check_opts(o):
    """ValueError for what the library answers with GPIS_ERR_ARG."""
    v = {k: float(o[k]) for k in OPT_NAMES}
    if not all(np.isfinite(list(v.values()))):
        raise ValueError("a non-finite option")
    if not (v["v_max"] > 0 and 0 < v["v_min"] <= v["v_max"] and v["a_max"] > 0 and v["d_max"] > 0):
        raise ValueError("v_max, v_min, a_max, d_max must be positive and v_min <= v_max")
    if min(v["a_lat"], v["w_max"], v["v_start"], v["v_end"], v["slow_dist"]) < 0:
        raise ValueError("a negative limit")


def _norm(v):
    """sqrtf of the squares summed left to right over the last axis."""
    sq = v[..., 0] * v[..., 0]
    for a in range(1, v.shape[-1]):
        sq = sq + v[..., a] * v[..., a]
    return np.sqrt(sq)


def prefix(d, variant=None):
    """[m, n] -> [m, n + 1]: P_0 = 0, P_i = P_{i-1} + d_{i-1}, ascending."""
    m, n = d.shape
    P = np.zeros((m, n + 1), F32)
    if variant == "npsum":
        for i in range(1, n + 1):
            P[:, i] = np.sum(np.ascontiguousarray(d[:, :i]), axis=1, dtype=F32)
        return P
    for i in range(1, n + 1):
        P[:, i] = P[:, i - 1] + d[:, i - 1]
    return P


def curvature(x, ds):
    m, N, dim = x.shape
    a, b, c = x[:, 1:-1] - x[:, :-2], x[:, 2:] - x[:, 1:-1], x[:, 2:] - x[:, :-2]
    if dim == 2:
        cr = np.abs(a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])
    else:
        cr = _norm(np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                             a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1))
    num = F32(2) * cr
    den = (ds[:, :-1] * ds[:, 1:]) * _norm(c)
    k = np.zeros((m, N), F32)
    k[:, 1:-1] = np.where(den == 0, F32(0), num / np.where(den == 0, F32(1), den))
    return k


def limits(x, ds, kappa, o, field=None):
    """(L [m, N] f32, code [m, N] u8)."""
    m, N, dim = x.shape
    vmax, vmin = o["v_max"], o["v_min"]
    L = np.full((m, N), vmax * vmax, F32)
    code = np.zeros((m, N), np.uint8)

    def take(cand, on, cd):
        nonlocal L, code
        hit = on & (cand < L)
        L = np.where(hit, cand, L).astype(F32)
        code = np.where(hit, np.uint8(cd), code)

    curved = kappa != 0
    ksafe = np.where(curved, kappa, F32(1))
    if o["a_lat"] > 0:
        take(o["a_lat"] / ksafe, curved, 1)
    if o["w_max"] > 0:
        q = o["w_max"] / ksafe
        take(q * q, curved, 2)
    if field is not None and o["slow_dist"] > 0:
        dist, shape, origin, step = field
        d = dfield_ref.sample(np.ascontiguousarray(dist, F32).ravel(), tuple(shape), tuple(origin), F32(step),
                              x.reshape(-1, dim))[:, 0].reshape(m, N)
        fin = np.isfinite(d)
        e = (np.where(fin, d, F32(0)) - o["clearance"]).astype(F32)
        vs = np.where(e <= 0, vmin, vmin + (vmax - vmin) * np.minimum(e / o["slow_dist"], F32(1))).astype(F32)
        take(vs * vs, fin, 3)
    interior = np.zeros((m, N), bool)
    interior[:, 1:-1] = True
    low = interior & (L < vmin * vmin)
    L = np.where(low, vmin * vmin, L).astype(F32)
    code = np.where(low, np.uint8(4), code)
    first, last = np.zeros((m, N), bool), np.zeros((m, N), bool)
    first[:, 0] = True
    last[:, N - 1] = True
    take(np.full((m, N), o["v_start"] * o["v_start"], F32), first, 5)
    take(np.full((m, N), o["v_end"] * o["v_end"], F32), last, 5)
    return L, code


def envelope(L, code, S, ds, o, variant=None):
    """(u [m, N], limiter [m, N])."""
    m, N = L.shape
    ta, td = F32(2) * o["a_max"], F32(2) * o["d_max"]
    if variant == "sweeps":
        u = L.copy()
        for i in range(1, N):
            u[:, i] = np.minimum(u[:, i], u[:, i - 1] + ta * ds[:, i - 1])
        for i in range(N - 2, -1, -1):
            u[:, i] = np.minimum(u[:, i], u[:, i + 1] + td * ds[:, i])
        return u, code.copy()
    u, lim = L.copy(), code.copy()
    i = np.arange(N)[None, :]
    for j in range(N):
        cand = np.where(j < i, L[:, j, None] + ta * (S - S[:, j, None]), L[:, j, None] + td * (S[:, j, None] - S)).astype(F32)
        hit = (i != j) & (cand < u)
        u = np.where(hit, cand, u).astype(F32)
        lim = np.where(hit, np.where(j < i, np.uint8(6), np.uint8(7)), lim).astype(np.uint8)
    return u, lim


def time(x, status, opts, field=None, variant=None, parts=None):
    """Timing of trajectories x [m, N, dim] f32 with result status [m] (2: no input).  field: None or (dist, shape, origin,
    step).  Returns dict(v, t [m, N] f32, limiter [m, N] u8, status [m] u8, duration, max_speed, max_curvature [m] f32,
    limiter_counts [m, 8] i32).  parts: a dict that receives ds, S, kappa, L, u of the live trajectories and their indices."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    check_opts(opts)
    o = {k: F32(opts[k]) for k in OPT_NAMES}
    live = np.flatnonzero(np.asarray(status) != 2)
    out = dict(v=np.full((m, N), np.nan, F32), t=np.full((m, N), np.nan, F32), limiter=np.zeros((m, N), np.uint8),
               status=np.full(m, 2, np.uint8), duration=np.full(m, np.nan, F32), max_speed=np.full(m, np.nan, F32),
               max_curvature=np.full(m, np.nan, F32), limiter_counts=np.zeros((m, 8), np.int32))
    if live.size == 0:
        return out
    xs = x[live]
    with np.errstate(all="ignore"):
        ds = _norm(xs[:, 1:] - xs[:, :-1])
        S = prefix(ds, variant)
        kappa = curvature(xs, ds)
        L, code = limits(xs, ds, kappa, o, field)
        u, lim = envelope(L, code, S, ds, o, variant)
        v = np.sqrt(u)
        dt = np.where(ds == 0, F32(0), (F32(2) * ds) / (v[:, :-1] + v[:, 1:])).astype(F32)
        t = prefix(dt, variant)
    out["v"][live], out["t"][live], out["limiter"][live] = v, t, lim
    out["status"][live] = np.where(np.isfinite(dt).all(axis=1), 0, 3)
    out["duration"][live], out["max_speed"][live], out["max_curvature"][live] = t[:, N - 1], v.max(axis=1), kappa.max(axis=1)
    out["limiter_counts"][live] = np.stack([(lim == c).sum(axis=1) for c in range(8)], axis=1)
    if parts is not None:
        parts.update(ds=ds, S=S, kappa=kappa, L=L, u=u, live=live)
    return out


# ---- control sequences ----------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return F64(a) * F64(b) + F64(c)
    return F64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def position(xs, vs, ts, tau, variant=None, trace=None):
    """The timed position at tau >= 0 of one trajectory (float64 arrays xs [N, dim], vs, ts [N]):
    tau >= t_{N-1}: the last waypoint.  Else i = the largest index <= N - 2 with t_i <= tau (bisection), h = t_{i+1} - t_i,
    e = tau - t_i, acc = (v_{i+1} - v_i) / h, s = v_i e + ((0.5 acc) e) e, ds_i = sqrt of the squares of x_{i+1} - x_i summed left
    to right, w = s / ds_i limited to [0, 1], p = x_i + w (x_{i+1} - x_i)."""
    N = ts.shape[0]
    if tau >= ts[N - 1]:
        if trace is not None:
            trace["past"] = trace.get("past", 0) + 1
        return xs[N - 1].copy()
    lo, hi = 0, N - 2
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if (ts[mid] < tau) if variant == "search_lt" else (ts[mid] <= tau):
            lo = mid
        else:
            hi = mid - 1
    i = lo
    if trace is not None and ts[i] == tau and i > 0:
        trace["on_knot"] = trace.get("on_knot", 0) + 1
    h = ts[i + 1] - ts[i]
    e = tau - ts[i]
    acc = (vs[i + 1] - vs[i]) / h
    if variant == "fused_s":
        s = _fma((F64(0.5) * acc) * e, e, vs[i] * e)
    else:
        s = vs[i] * e + ((F64(0.5) * acc) * e) * e
    d = xs[i + 1] - xs[i]
    sq = d[0] * d[0]
    for a in range(1, d.shape[0]):
        sq = sq + d[a] * d[a]
    w = s / np.sqrt(sq)
    w = w if w > 0.0 else F64(0.0)
    w = w if w < 1.0 else F64(1.0)
    return xs[i] + w * d


def controls(x, v, t, tstatus, dt, T, t0=0.0, w_limit=0.0, min_move=1e-9, variant=None, trace=None):
    """Control sequences of the model of mppi_ref (translate with the heading from before the step, then turn) that take a robot
    from p_0, facing heading0, through the timed positions p_k at tau_k = t0 + (double)k * dt, k = 0 .. T.
    D_k = p_{k+1} - p_k, n_k = sqrt(Dx Dx + Dy Dy); step k moves iff n_k > min_move; h_k = (Dx, Dy) / n_k of the latest moving
    step <= k, of the first moving step before it, (1, 0) without one; h_T = h_{T-1}.  With (c, s) = h_k, (c', s') = h_{k+1}:
      dim 2: v_k = (c Dx + s Dy) / dt;  dim 3: ((c Dx + s Dy) / dt, ((-s) Dx + c Dy) / dt, Dz / dt)
      num = c s' - s c', den = 1 + (c c' + s s');  den <= 0: w_k = +-w_limit by the sign of num (num >= 0: +), 0 with
      w_limit = 0, counted as clamped;  else w_k = (num / den) / (0.5 dt), with w_limit > 0 limited to +-w_limit (counted).
    Returns dict(U [m, T, nu] f64, heading0 [m, 2], p0 [m, dim], clamped [m] i32, p [m, T + 1, dim]).  A trajectory whose timing
    status is not 0: zero controls, heading0 (1, 0), p0 = x_0, p = NaN."""
    x = np.ascontiguousarray(x, F32)
    m, N, dim = x.shape
    T = int(T)
    if not (dt > 0 and np.isfinite(dt) and 1 <= T <= MAX_T and t0 >= 0 and np.isfinite(t0) and w_limit >= 0 and
            np.isfinite(w_limit) and min_move >= 0 and np.isfinite(min_move)):
        raise ValueError("bad arguments")
    nu = 4 if dim == 3 else 2
    dt, t0, w_limit, min_move = F64(dt), F64(t0), F64(w_limit), F64(min_move)
    U = np.zeros((m, T, nu), F64)
    h0 = np.zeros((m, 2), F64)
    h0[:, 0] = 1.0
    p0 = x[:, 0].astype(F64)
    P = np.full((m, T + 1, dim), np.nan, F64)
    clamped = np.zeros(m, np.int32)
    half = F64(0.5) * dt
    with np.errstate(all="ignore"):
        for r in range(m):
            if tstatus[r] != 0:
                continue
            xs, vs, ts = x[r].astype(F64), np.asarray(v[r], F32).astype(F64), np.asarray(t[r], F32).astype(F64)
            p = [position(xs, vs, ts, t0 + F64(k) * dt, variant, trace) for k in range(T + 1)]
            D = [p[k + 1] - p[k] for k in range(T)]
            n = [np.sqrt(d[0] * d[0] + d[1] * d[1]) for d in D]
            mov = [n[k] > min_move for k in range(T)]
            first = mov.index(True) if any(mov) else -1
            H, last = [], -1
            for k in range(T):
                last = k if mov[k] else last
                j = last if last >= 0 else first
                H.append((F64(1.0), F64(0.0)) if j < 0 else (D[j][0] / n[j], D[j][1] / n[j]))
                if trace is not None and last < 0 and first >= 0:
                    trace["before_first"] = trace.get("before_first", 0) + 1
            H.append(H[T - 1])
            for k in range(T):
                c, s = H[k + 1] if variant == "heading_after" else H[k]
                c1, s1 = H[k + 1]
                c0, s0 = H[k]
                d = D[k]
                U[r, k, 0] = (c * d[0] + s * d[1]) / dt
                if dim == 3:
                    U[r, k, 1] = ((-s) * d[0] + c * d[1]) / dt
                    U[r, k, 2] = d[2] / dt
                num = c0 * s1 - s0 * c1
                den = F64(1.0) + (c0 * c1 + s0 * s1)
                if den <= 0:
                    w = (w_limit if num >= 0 else -w_limit) if w_limit > 0 else F64(0.0)
                    clamped[r] += 1
                    if trace is not None:
                        trace["reversal"] = trace.get("reversal", 0) + 1
                else:
                    w = (num / den) / half
                    if w_limit > 0 and w > w_limit:
                        w = w_limit
                        clamped[r] += 1
                    elif w_limit > 0 and w < -w_limit:
                        w = -w_limit
                        clamped[r] += 1
                U[r, k, nu - 1] = w
            h0[r] = H[0]
            p0[r] = p[0]
            P[r] = np.stack(p)
            if trace is not None:
                trace["still"] = trace.get("still", 0) + (0 if any(mov) else 1)
                trace["vertical"] = trace.get("vertical", 0) + sum(1 for k in range(T) if dim == 3 and not mov[k] and D[k][2] != 0)
    return dict(U=U, heading0=h0, p0=p0, clamped=clamped, p=P)
