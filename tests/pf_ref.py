"""Reference for the particle filter (csrc/pf.hip, gpis_pf_* / gpis2_pf_update_scan / gpis3_pf_update_depth): a
numpy restatement of the contract, written independently of the product (it imports nothing from gpismap_amd).  The cost of a
particle is the pose scorer's (tests/locate_ref.py); what is stated here is the state, the generator, the motion update, the
weights, their integer totals, the estimate and the systematic resampling.

Contract (every floating-point expression is double, written left to right, nothing contracted; division and sqrt are IEEE):
- State: 2-D (x, y, c, s); 3-D (t0, t1, t2, w, x, y, z), the quaternion of unit norm.  Per particle a negative log weight L;
  per filter a uint32 tick and a uint64 seed.
- Float32 pose (what the scorer reads): every component cast from the double state.  2-D [x, y, c, s, -s, c]; 3-D [t, R],
  R column-major from the quaternion (`quat_to_mat`).
- init: the state from float32 poses: 2-D (t, R[0], R[1]); 3-D t and `mat_to_quat` of R (trace / largest-diagonal branches,
  then normalised).  L = 0, tick = 0, q = 2^32 (uniform).
- Generator: Philox4x32-10 keyed (seed & 0xffffffff, seed >> 32) on the counter (slot, tick, k, tag); tag 0 motion noise, tag 1
  the resampling offset.  Deviate k: S = the sum of the eight 16-bit halves of the block, z = (double)(2 S - 8 * 65535) * KZ:
  integer until the last step, unit variance, |z| <= 4.899.
- predict: tick += 1, then `predict` below (noise in the body frame; the Cayley map for the heading; the quaternion product
  with (1, a0, a1, a2); the result divided by its norm).
- update: L += beta * cost; Lmin = min L; w = exp(-(L - Lmin)); q = floor(w * 2^32) as uint64 (the one inexact step: both exp
  are within 1 ulp, 2^32 * 2^-51 < 1, so two implementations differ by at most 1 in q).  T = sum q, Th = sum (q >> 16),
  S2 = sum (q >> 16)^2 as integers; neff = (double)Th * (double)Th / (double)S2.  Estimate: terms (double)q * column (3-D: every
  quaternion times +-1 so that its dot product with the quaternion of the lowest-index particle of maximal q is >= 0),
  reduced by track_ref.tree_sum, divided by (double)T, the heading / quaternion normalised.  Resample iff
  neff < resample_below * m.
- resample: tick += 1; C = the inclusive prefix sum of q; qs, rem = divmod(T, m); r = ((w0 << 32) | w1) mod qs from the block
  of counter (0xFFFFFFFF, tick, 0, 1); p_j = j qs + (j rem) div m + r; ancestor a_j = the first i with C_i > p_j; state and
  pose gathered, L = 0.  q stays the last update's.

The `variant` arguments build the defective variants tests/test_pf_ref.py rejects; None is the contract."""
import math

import numpy as np

import locate_ref
import track_ref

F32 = np.float32
F64 = np.float64
U64 = np.uint64
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KZ = float.fromhex("0x1.3988e1412ed76p-17")          # 1 / sqrt(8 (65536^2 - 1) / 3)
TWO32 = 4294967296.0
MAX_PARTICLES = 1 << 24


def default_opts(dim):
    """The library's defaults (gpis_pf_default_opts)."""
    if dim == 3:
        return dict(max_residual=0.05, beta=100.0, sigma_t=(0.003, 0.003, 0.003), sigma_r=0.003, resample_below=0.5, stride=8)
    return dict(max_residual=0.5, beta=2.0, sigma_t=(0.03, 0.03, 0.0), sigma_r=0.03, resample_below=0.5, stride=1)


# ---- the generator --------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counters: the four output words as uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(v, U64)) & U64(MASK) for v in (c0, c1, c2, c3)]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = U64(M0) * c[0]
        p1 = U64(M1) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & U64(MASK), (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & U64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK, seed >> 32


def deviates(seed, slots, tick, k, tag=0):
    """z [len(slots)] float64: deviate number k of every slot at this tick."""
    w = philox(slots, tick, k, tag, *key(seed))
    S = np.zeros(w[0].shape, np.int64)
    for v in w:
        S += (v & U64(0xFFFF)).astype(np.int64) + (v >> U64(16)).astype(np.int64)
    return (2 * S - 8 * 65535).astype(F64) * KZ


# ---- rotations ------------------------------------------------------------------------------------------------------------
def quat_to_mat(Q):
    """R [m, 9] float64 column-major of the quaternions Q [m, 4] = (w, x, y, z)."""
    w, x, y, z = (Q[:, a] for a in range(4))
    return np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z), 2.0 * (x * z - w * y),
                     2.0 * (x * y - w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + w * x),
                     2.0 * (x * z + w * y), 2.0 * (y * z - w * x), 1.0 - 2.0 * (x * x + y * y)], axis=1)


def mat_to_quat(R):
    """(w, x, y, z) floats of one column-major rotation matrix R[9] (element (row r, column c) at R[3 c + r]): the trace /
    largest-diagonal branches in double, then divided by the norm."""
    R = [float(v) for v in R]
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q = (0.25 * s, (R[5] - R[7]) / s, (R[6] - R[2]) / s, (R[1] - R[3]) / s)
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0
        q = ((R[5] - R[7]) / s, 0.25 * s, (R[3] + R[1]) / s, (R[6] + R[2]) / s)
    elif R[4] > R[8]:
        s = math.sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0
        q = ((R[6] - R[2]) / s, (R[3] + R[1]) / s, 0.25 * s, (R[7] + R[5]) / s)
    else:
        s = math.sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0
        q = ((R[1] - R[3]) / s, (R[6] + R[2]) / s, (R[7] + R[5]) / s, 0.25 * s)
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def qmul(p, q):
    """The Hamilton product of quaternion arrays [m, 4] (or [4], broadcast), every component left to right."""
    pw, px, py, pz = (p[..., a] for a in range(4))
    qw, qx, qy, qz = (q[..., a] for a in range(4))
    return np.stack([pw * qw - px * qx - py * qy - pz * qz,
                     pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw], axis=-1)


# ---- state ----------------------------------------------------------------------------------------------------------------
def init_state(poses, dim):
    """state [m, 4 / 7] float64 of float32 poses [m, 6 / 12]."""
    P = np.asarray(poses, F32).reshape(-1, 12 if dim == 3 else 6)
    if not np.all(np.isfinite(P)):
        raise ValueError("a non-finite pose")
    if dim == 2:
        return P[:, :4].astype(F64)
    Pd = P.astype(F64)
    Q = np.array([mat_to_quat(r[3:]) for r in Pd], F64).reshape(-1, 4)
    return np.concatenate([Pd[:, :3], Q], axis=1)


def pose32(state, dim):
    """The float32 poses [m, 6 / 12] the scorer reads."""
    if dim == 2:
        x, y, c, s = (state[:, a] for a in range(4))
        return np.stack([x, y, c, s, -s, c], axis=1).astype(F32)
    return np.concatenate([state[:, :3], quat_to_mat(state[:, 3:])], axis=1).astype(F32)


def pose64(est, dim):
    """The double pose [t, R] of one estimated state."""
    e = np.asarray(est, F64)
    if dim == 2:
        return np.array([e[0], e[1], e[2], e[3], -e[3], e[2]], F64)
    return np.concatenate([e[:3], quat_to_mat(e[None, 3:])[0]])


def motion_from_pose(motion, dim):
    """The relative pose [t, R] (double) as the kernel's arguments: 2-D (dx, dy, cu, su); 3-D (d(3), Qu(4))."""
    M = np.asarray(motion, F64).ravel()
    if dim == 2:
        return M[:4].copy()
    return np.concatenate([M[:3], np.array(mat_to_quat(M[3:]), F64)])


def predict(state, dim, seed, tick, motion, sigma_t, sigma_r, variant=None, slots=None):
    """The state after one motion update at `tick` (the tick after its increment); motion as motion_from_pose returns it."""
    m = state.shape[0]
    slots = np.arange(m, dtype=U64) if slots is None else np.asarray(slots, U64)
    st = state.astype(F32) if variant == "float32" else state
    one, two = (F32(1.0), F32(2.0)) if variant == "float32" else (1.0, 2.0)
    cast = (lambda v: F32(v)) if variant == "float32" else (lambda v: float(v))
    nz = 3 if dim == 2 else 6
    z = [deviates(seed, slots, tick, k) for k in range(nz)]
    if variant == "float32":
        z = [v.astype(F32) for v in z]
    half = cast(0.5) * cast(sigma_r)
    if dim == 2:
        x, y, c, s = (st[:, a] for a in range(4))
        dx, dy, cu, su = (cast(v) for v in motion)
        bx = dx + cast(sigma_t[0]) * z[0]
        by = dy + cast(sigma_t[1]) * z[1]
        a = half * z[2]
        den = one + a * a
        cn = (one - a * a) / den
        sn = (a + a) / den
        if variant == "world_noise":        # the noise added in the world frame: only the motion itself is rotated
            x1 = x + (c * dx - s * dy) + cast(sigma_t[0]) * z[0]
            y1 = y + (s * dx + c * dy) + cast(sigma_t[1]) * z[1]
        else:
            x1 = x + (c * bx - s * by)
            y1 = y + (s * bx + c * by)
        c1 = c * cu - s * su
        s1 = c * su + s * cu
        c2 = c1 * cn - s1 * sn
        s2 = c1 * sn + s1 * cn
        if variant != "no_renorm":
            n = np.sqrt(c2 * c2 + s2 * s2)
            c2, s2 = c2 / n, s2 / n
        return np.stack([x1, y1, c2, s2], axis=1).astype(F64)
    t, Q = st[:, :3], st[:, 3:]
    d = [cast(v) for v in motion[:3]]
    Qu = np.array([cast(v) for v in motion[3:]], st.dtype)
    R = quat_to_mat(Q) if variant != "float32" else quat_to_mat(Q).astype(F32)
    b = [d[a] + cast(sigma_t[a]) * z[a] for a in range(3)]
    if variant == "world_noise":
        tn = [t[:, a] + (R[:, a] * d[0] + R[:, 3 + a] * d[1] + R[:, 6 + a] * d[2]) + cast(sigma_t[a]) * z[a] for a in range(3)]
    else:
        tn = [t[:, a] + (R[:, a] * b[0] + R[:, 3 + a] * b[1] + R[:, 6 + a] * b[2]) for a in range(3)]
    A = np.stack([np.full(m, one, st.dtype)] + [half * z[3 + k] for k in range(3)], axis=1)
    Q2 = qmul(qmul(Q, Qu), A)
    if variant != "no_renorm":
        n = np.sqrt(Q2[:, 0] * Q2[:, 0] + Q2[:, 1] * Q2[:, 1] + Q2[:, 2] * Q2[:, 2] + Q2[:, 3] * Q2[:, 3])
        Q2 = Q2 / n[:, None]
    return np.concatenate([np.stack(tn, axis=1), Q2], axis=1).astype(F64)


# ---- weights --------------------------------------------------------------------------------------------------------------
def accumulate(L, cost, beta):
    return L + float(beta) * cost


def weights(L, variant=None):
    """q [m] uint64 of the accumulated negative log weights."""
    w = np.exp(-(L - L.min())) * TWO32
    return (np.round(w) if variant == "round" else np.floor(w)).astype(U64)


def totals(q):
    """(T, Th, S2) as Python integers."""
    h = q >> U64(16)
    return int(q.sum(dtype=U64)), int(h.sum(dtype=U64)), int((h * h).sum(dtype=U64))


def neff(Th, S2):
    return float(Th) * float(Th) / float(S2)


def best_index(q):
    """The lowest index of maximal q."""
    return int(np.argmax(q))


def estimate(q, state, dim, variant=None):
    """The estimated state [4 / 7] from the weights q and the states."""
    cols = state
    if dim == 3:
        Q = state[:, 3:]
        Q0 = Q[best_index(q)]
        dot = Q[:, 0] * Q0[0] + Q[:, 1] * Q0[1] + Q[:, 2] * Q0[2] + Q[:, 3] * Q0[3]
        sg = np.where(dot >= 0.0, 1.0, -1.0)
        cols = np.concatenate([state[:, :3], Q * sg[:, None]], axis=1)
    terms = q.astype(F64)[:, None] * cols
    S = np.sum(terms, axis=0) if variant == "np_sum" else track_ref.tree_sum(terms)
    E = S / float(totals(q)[0])
    k = 2 if dim == 2 else 3
    n = math.sqrt(sum(float(v) * float(v) for v in E[k:])) if dim == 2 else \
        math.sqrt(float(E[3]) * float(E[3]) + float(E[4]) * float(E[4]) + float(E[5]) * float(E[5]) + float(E[6]) * float(E[6]))
    E = E.copy()
    E[k:] = E[k:] / n
    return E


# ---- resampling -----------------------------------------------------------------------------------------------------------
def positions(q, seed, tick):
    """(p [m] uint64, C [m] uint64, T): the systematic sampling positions at `tick` (after its increment)."""
    m = q.shape[0]
    C = np.cumsum(q, dtype=U64)
    T = int(C[-1])
    qs, rem = divmod(T, m)
    w = philox(0xFFFFFFFF, tick, 0, 1, *key(seed))
    r = ((int(w[0][0]) << 32) | int(w[1][0])) % qs
    j = np.arange(m, dtype=U64)
    p = j * U64(qs) + (j * U64(rem)) // U64(m) + U64(r)
    return p, C, T


def ancestors(q, seed, tick, variant=None):
    p, C, _ = positions(q, seed, tick)
    return np.searchsorted(C, p, side="left" if variant == "left" else "right").astype(np.int32)


# ---- the filter -----------------------------------------------------------------------------------------------------------
class Filter:
    """The whole contract as an object: what ParticleFilter does, step by step."""

    def __init__(self, poses, dim, seed=0):
        self.dim, self.seed, self.tick = dim, int(seed), 0
        self.state = init_state(poses, dim)
        self.m = self.state.shape[0]
        self.L = np.zeros(self.m, F64)
        self.q = np.full(self.m, 1 << 32, U64)
        self.anc = np.arange(self.m, dtype=np.int32)
        self.cost = np.zeros(self.m, F64)
        self.inliers = np.zeros(self.m, np.int32)
        self.est = None
        self.neff = None
        self.resampled = False

    def poses(self):
        return pose32(self.state, self.dim)

    def predict(self, motion, sigma_t, sigma_r):
        """motion: the relative pose [t, R] (6 / 12 doubles)."""
        self.tick += 1
        self.state = predict(self.state, self.dim, self.seed, self.tick, motion_from_pose(motion, self.dim), sigma_t, sigma_r)

    def update(self, dist, shape, origin, step, loc, max_residual, beta, resample_below):
        self.cost, self.inliers, _ = locate_ref.score(dist, shape, origin, step, loc, self.poses(), max_residual)
        self.L = accumulate(self.L, self.cost, beta)
        self.q = weights(self.L)
        self.T, self.Th, self.S2 = totals(self.q)
        self.neff = neff(self.Th, self.S2)
        self.est = estimate(self.q, self.state, self.dim)
        self.resampled = self.neff < float(resample_below) * self.m
        if self.resampled:
            self.resample()
        return self.est

    def resample(self):
        self.tick += 1
        self.anc = ancestors(self.q, self.seed, self.tick)
        self.state = self.state[self.anc]
        self.L = np.zeros(self.m, F64)


__all__ = ["default_opts", "philox", "key", "deviates", "quat_to_mat", "mat_to_quat", "qmul", "init_state", "pose32", "pose64",
           "motion_from_pose", "predict", "accumulate", "weights", "totals", "neff", "best_index", "estimate", "positions",
           "ancestors", "Filter", "KZ"]
