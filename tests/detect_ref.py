"""Reference for the moving-obstacle detector (csrc/detect.hip, csrc/detect_host.h): a numpy restatement of the
contract, written independently of the product (it imports nothing from gpismap_amd).  Components come from a union-find over
the links, deliberately not from label propagation.

Contract:
- Samples: the tracker's.  2-D: track_ref.points2 (beams with 0.2 < (double)r < 30, input order), sample grid = the beams, g = n.
  3-D: track_ref.points3 at `stride`; sample grid = the strided pixels (col, row) = (gn stride, gm stride), gn < gw = W //
  stride, gm < gh = H // stride, q = gn gh + gm (column-major).  x = track_ref.world (the double pose cast to float32,
  pass_pose), d = dfield_ref.sample(dist, x)[:, 0].
- Foreign iff d is finite and (double)d >= min_dist, and, with a mask `seen` on the field's lattice, the byte of the lattice
  point nearest x is set: per axis i_a = min(int(floor(f32(f32(f32(x_a - o_a) / step) + 0.5))), n_a - 1), all in float32.  d NaN
  (off the lattice) is not foreign.
- Neighbours: 2-D beams k - 1 and k + 1 of the frame -- there is NO wrap from the last beam to the first, a component that ends
  on the last beam and one that begins on beam 0 stay two --; 3-D the 8 neighbours (gn + dn, gm + dm) inside gw x gh.  Two
  neighbouring foreign samples are linked iff s <= link * link where e_a = (double)x_a - (double)y_a and s = e_0 e_0 + e_1 e_1
  (+ e_2 e_2) from 0.0, left to right, in double.
- A component's label is its smallest grid index; components are ordered by label.  The label image holds it at every foreign
  sample and -1 elsewhere; the d image is NaN where the sample is not valid; x is 0 there.
- Per component: count; per axis lo_a, hi_a = the least and greatest float32 coordinate under the order of the integer key
  k(b) = b ^ (0xffffffff if b >> 31 else 0x80000000) of the float's bits b (the float order, with -0 below +0); centre c_a =
  0.5 * ((double)lo_a + (double)hi_a); r2 = the greatest s = sum_a ((double)x_a - c_a)^2 (from 0.0, left to right) over its samples.
- Selection: count < min_points: noise (flag 1); else sqrt(r2) > max_radius: too large (flag 2); of the rest at most 256 become
  balls (flag 0): the largest counts first, ties by the lower label; the others are dropped (flag 3).  Balls in label order,
  radius = sqrt(r2) + pad.
- Tracks (double): the previous call's balls with t_prev, velocity, id, age, missed.  dt = t - t_prev.  Candidate pairs (old i,
  new j): dist = sqrt(sum_a (c_j,a - (c_i,a + v_i,a dt))^2) <= gate + max_speed * dt; taken greedily in ascending (dist, i, j),
  each ball once.  Matched: v_raw = (c_j - c_i) / dt; v = v_raw if the old ball's age is 0 else alpha * v_raw + (1 - alpha) * v_i;
  id kept, age + 1, missed 0.  New: v = 0, id = the next fresh id (in label order), age 0.  Unmatched old ball: missed + 1; kept
  iff that is <= max_missed, at c_i + v_i dt with its v, radius, id and age; coasting balls follow the detected ones in id order
  while there are fewer than 256 balls.
- Defaults for a field of lattice step `step` (lengths of k steps are float64(float32(k) * float32(step))): min_dist 2 steps,
  link 3 steps, pad 1 step, gate 4 steps, max_radius 1, max_speed 2, alpha 0.5, min_points 3, max_missed 2, stride 1 (2-D) / 2
  (3-D), max_rounds 0.

`variant` builds defective variants: "gt" (d > min_dist), "link32" (the link measured in float32), "wrap" (2-D: the last beam
neighbours the first), "n4" (3-D: 4 instead of 8 neighbours), "mean" (the centre is the mean, not the box midpoint), "tie_high"
(ties of the cap by the higher label), "no_filter" (v = v_raw always)."""
import math

import numpy as np

import dfield_ref
import track_ref

F32 = np.float32
F64 = np.float64
MAX_BALLS = 256
BALL, NOISE, LARGE, DROPPED = 0, 1, 2, 3


def opts(dim, step, **kw):
    s = F32(step)
    o = dict(min_dist=float(F64(F32(2) * s)), link=float(F64(F32(3) * s)), pad=float(F64(F32(1) * s)), gate=float(F64(F32(4) * s)),
             max_radius=1.0, max_speed=2.0, alpha=0.5, min_points=3, max_missed=2, stride=2 if dim == 3 else 1, max_rounds=0)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def key(x):
    """The order-preserving integer key of float32 values."""
    b = np.asarray(x, F32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xffffffff), np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return (k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xffffffff)).astype(np.uint32)).view(F32)


def nearest_index(x, shape, origin, step):
    """The lattice index of the point nearest each x [m, dim] (x on the lattice), in float32."""
    dim = len(shape)
    idx = np.zeros(x.shape[0], np.int64)
    mul = 1
    for a in range(dim):
        u = ((x[:, a] - F32(origin[a])).astype(F32) / F32(step)).astype(F32)
        i = np.minimum(np.floor((u + F32(0.5)).astype(F32)).astype(np.int64), shape[a] - 1)
        idx += i * mul
        mul *= shape[a]
    return idx


def link_s(xa, xb, variant=None):
    """The squared distance of the contract between rows of xa and xb."""
    if variant == "link32":
        s = F32(0)
        for a in range(xa.shape[1]):
            e = (xa[:, a] - xb[:, a]).astype(F32)
            s = (s + e * e).astype(F32)
        return s.astype(F64)
    s = np.zeros(xa.shape[0], F64)
    for a in range(xa.shape[1]):
        e = xa[:, a].astype(F64) - xb[:, a].astype(F64)
        s = s + e * e
    return s


def samples(dist, shape, origin, step, dim, frame, pose, o, seen=None, variant=None):
    """The per-sample stage.  frame: (thetas, ranges, off2) or (depth, cam6).  Returns dict(g, gw, gh, x [g, dim] f32, d [g] f32,
    valid [g] bool, foreign [g] bool)."""
    if dim == 2:
        thetas, ranges, off = frame
        loc, k = track_ref.points2(thetas, ranges, off)
        g, gw, gh = int(np.asarray(ranges).size), 0, 0
        q = k
    else:
        depth, cam6 = frame
        st = int(o["stride"])
        W, H = int(cam6[4]), int(cam6[5])
        loc, k = track_ref.points3(depth, cam6, st)
        gw, gh = W // st, H // st
        g = gw * gh
        q = (k // H) // st * gh + (k % H) // st
    x = np.zeros((g, dim), F32)
    d = np.full(g, np.nan, F32)
    valid = np.zeros(g, bool)
    foreign = np.zeros(g, bool)
    if q.size:
        xw = track_ref.world(loc, pose, dim)
        dd = dfield_ref.sample(dist, shape, origin, step, xw)[:, 0]
        x[q], d[q], valid[q] = xw, dd, True
        with np.errstate(invalid="ignore"):
            f = np.isfinite(dd) & ((dd.astype(F64) > o["min_dist"]) if variant == "gt" else (dd.astype(F64) >= o["min_dist"]))
        if seen is not None and f.any():
            m = np.asarray(seen).ravel() != 0
            ff = np.nonzero(f)[0]
            f[ff] = m[nearest_index(xw[ff], tuple(int(v) for v in shape), origin, step)]
        foreign[q] = f
    return dict(g=g, gw=gw, gh=gh, x=x, d=d, valid=valid, foreign=foreign)


def neighbour_pairs(dim, g, gw, gh, variant=None):
    """Every unordered pair (p, q), p < q, of neighbouring grid indices."""
    if dim == 2:
        a = np.arange(g - 1, dtype=np.int64)
        p, q = a, a + 1
        if variant == "wrap" and g > 2:
            p, q = np.append(p, 0), np.append(q, g - 1)
        return p, q
    gn, gm = np.meshgrid(np.arange(gw), np.arange(gh), indexing="ij")
    ps, qs = [], []
    offs = ((1, 0), (0, 1)) if variant == "n4" else ((1, -1), (1, 0), (1, 1), (0, 1))
    for dn, dm in offs:
        ok = (gn + dn < gw) & (gm + dm >= 0) & (gm + dm < gh)
        ps.append((gn[ok] * gh + gm[ok]).ravel())
        qs.append(((gn[ok] + dn) * gh + gm[ok] + dm).ravel())
    return np.concatenate(ps).astype(np.int64), np.concatenate(qs).astype(np.int64)


def components(dim, s, o, variant=None):
    """Union-find over the links.  Returns (label image [g] i32, labels [c] ascending)."""
    g, x, f = s["g"], s["x"], s["foreign"]
    p, q = neighbour_pairs(dim, g, s["gw"], s["gh"], variant)
    both = f[p] & f[q]
    p, q = p[both], q[both]
    linked = link_s(x[p], x[q], variant) <= o["link"] * o["link"]
    p, q = p[linked], q[linked]
    parent = np.arange(g)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(p.tolist(), q.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    img = np.full(g, -1, np.int32)
    for a in np.nonzero(f)[0].tolist():
        img[a] = find(a)
    return img, np.unique(img[img >= 0]).astype(np.int32)


def table(dim, s, img, labels, variant=None):
    """dict(label, count [c] i32, box [c, 2, dim] f32, centre [c, dim] f64, r2 [c] f64)."""
    nc = labels.size
    out = dict(label=labels.astype(np.int32), count=np.zeros(nc, np.int32), box=np.zeros((nc, 2, dim), F32),
               centre=np.zeros((nc, dim), F64), r2=np.zeros(nc, F64))
    for c, lab in enumerate(labels.tolist()):
        xs = s["x"][img == lab]
        out["count"][c] = xs.shape[0]
        k = key(xs)
        lo, hi = unkey(k.min(axis=0)), unkey(k.max(axis=0))
        out["box"][c, 0], out["box"][c, 1] = lo, hi
        if variant == "mean":
            ctr = xs.astype(F64).sum(axis=0) / xs.shape[0]
        else:
            ctr = 0.5 * (lo.astype(F64) + hi.astype(F64))
        out["centre"][c] = ctr
        ss = np.zeros(xs.shape[0], F64)
        for a in range(dim):
            e = xs[:, a].astype(F64) - ctr[a]
            ss = ss + e * e
        out["r2"][c] = ss.max()
    return out


def select(tab, o, variant=None):
    """(flag [c] i32, sel: the indices of the balls, ascending)."""
    nc = tab["label"].size
    flag = np.zeros(nc, np.int32)
    cand = []
    for c in range(nc):
        if tab["count"][c] < o["min_points"]:
            flag[c] = NOISE
        elif math.sqrt(tab["r2"][c]) > o["max_radius"]:
            flag[c] = LARGE
        else:
            cand.append(c)
    if len(cand) > MAX_BALLS:
        order = sorted(cand, key=lambda c: (-int(tab["count"][c]), -c if variant == "tie_high" else c))
        for c in order[MAX_BALLS:]:
            flag[c] = DROPPED
        cand = sorted(order[:MAX_BALLS])
    return flag, cand


def associate(dim, det, t, o, tracks, variant=None):
    """det: list of dict(c [dim], r, comp).  tracks: dict(balls, t_prev, held, next_id), updated.  Returns the new ball list."""
    old = tracks["balls"] if tracks["held"] else []
    dt = t - tracks["t_prev"] if tracks["held"] else 0.0
    lim = o["gate"] + o["max_speed"] * dt
    pairs = []
    for i, p in enumerate(old):
        for j, b in enumerate(det):
            s = 0.0
            for a in range(dim):
                e = float(b["c"][a]) - (float(p["c"][a]) + float(p["v"][a]) * dt)
                s = s + e * e
            d = math.sqrt(s)
            if d <= lim:
                pairs.append((d, i, j))
    pairs.sort()
    of_old, of_new = {}, {}
    for d, i, j in pairs:
        if i not in of_old and j not in of_new:
            of_old[i], of_new[j] = j, i
    out = []
    for j, b in enumerate(det):
        nb = dict(c=[float(v) for v in b["c"]], r=float(b["r"]), comp=b["comp"], missed=0)
        if j in of_new:
            p = old[of_new[j]]
            v = []
            for a in range(dim):
                vr = (nb["c"][a] - float(p["c"][a])) / dt
                v.append(vr if (p["age"] == 0 or variant == "no_filter") else o["alpha"] * vr + (1.0 - o["alpha"]) * float(p["v"][a]))
            nb.update(v=v, id=p["id"], age=p["age"] + 1)
        else:
            nb.update(v=[0.0] * dim, id=tracks["next_id"], age=0)
            tracks["next_id"] += 1
        out.append(nb)
    coast = []
    for i, p in enumerate(old):
        if i in of_old or p["missed"] + 1 > o["max_missed"]:
            continue
        coast.append(dict(c=[float(p["c"][a]) + float(p["v"][a]) * dt for a in range(dim)], v=[float(v) for v in p["v"]], r=p["r"],
                          id=p["id"], age=p["age"], missed=p["missed"] + 1, comp=-1))
    coast.sort(key=lambda b: b["id"])
    for b in coast:
        if len(out) < MAX_BALLS:
            out.append(b)
    tracks.update(balls=out, t_prev=t, held=True)
    return out


class Detector:
    """The detector's state: the tracks.  detect() returns dict(samples=..., label (image), tab (every component, with flag),
    balls: dict of arrays as gpismap_amd.Detector.result(), counts)."""

    def __init__(self, variant=None):
        self.variant = variant
        self.reset_tracks()
        self.tracks["next_id"] = 0

    def reset_tracks(self):
        nid = getattr(self, "tracks", {}).get("next_id", 0)
        self.tracks = dict(balls=[], t_prev=0.0, held=False, next_id=nid)

    def detect(self, dist, shape, origin, step, dim, frame, pose, t, o, seen=None):
        v = self.variant
        if self.tracks["held"] and not t > self.tracks["t_prev"]:
            raise ValueError("t does not increase")
        s = samples(dist, shape, origin, step, dim, frame, pose, o, seen, v)
        img, labels = components(dim, s, o, v)
        tab = table(dim, s, img, labels, v)
        flag, sel = select(tab, o, v)
        tab["flag"] = flag
        det = [dict(c=tab["centre"][c], r=math.sqrt(tab["r2"][c]) + o["pad"], comp=c) for c in sel]
        balls = associate(dim, det, t, o, self.tracks, v)
        b = len(balls)
        res = dict(centre=np.array([x["c"] for x in balls], F64).reshape(b, dim), velocity=np.array([x["v"] for x in balls], F64).reshape(b, dim),
                   radius=np.array([x["r"] for x in balls], F64), id=np.array([x["id"] for x in balls], np.int32),
                   age=np.array([x["age"] for x in balls], np.int32), missed=np.array([x["missed"] for x in balls], np.int32),
                   count=np.array([tab["count"][x["comp"]] if x["comp"] >= 0 else 0 for x in balls], np.int32),
                   label=np.array([tab["label"][x["comp"]] if x["comp"] >= 0 else -1 for x in balls], np.int32),
                   box=np.array([tab["box"][x["comp"]] if x["comp"] >= 0 else np.zeros((2, dim), F32) for x in balls], F32).reshape(b, 2, dim),
                   samples=int(s["valid"].sum()), foreign=int(s["foreign"].sum()), components=int(labels.size),
                   noise=int((flag == NOISE).sum()), too_large=int((flag == LARGE).sum()), dropped=int((flag == DROPPED).sum()))
        return dict(samples=s, label=img, tab=tab, balls=res)


__all__ = ["opts", "key", "unkey", "nearest_index", "link_s", "samples", "neighbour_pairs", "components", "table", "select", "associate",
           "Detector", "MAX_BALLS"]
