"""numpy reference of the view scorer (csrc/view.hip, gpis*_view_gain_*): which unseen lattice points would a
sensor at each of m candidate poses reveal?  It composes two references and restates neither: render_field_ref predicts what the
sensor would measure of the field, cover_ref says which lattice points such a measurement sees.  It imports nothing from
gpismap_amd.  Every result is an integer.

Per pose k: 1. render_field_ref.render_depth / render_scan with the `march` options; d'[ray] = depth where status == 0, else `miss`
(float32; status 1 and 2 both miss); hits[k] = the rays of status 0.  2. mask_k = cover_ref.depth_mask / scan_mask of d' from
pose k, verbatim.  3. target[p] = not seen[p] and not (dist[p] < min_dist), a float32 compare (a NaN dist counts);
gain[k] = #{p : target[p] and mask_k[p]}."""
import math

import numpy as np

import cover_ref
import render_field_ref

F32 = np.float32


def default_opts(dim, step):
    """gpis_view_default_opts: march = render_field_ref.Opts(dim, step), the coverage's back_off and max_gap, a miss one cell short
    of the march's far end (the farthest measurement the coverage rule accepts, less one cell), no distance gate."""
    c = cover_ref.default_opts(dim, step)
    march = render_field_ref.Opts(dim, step)
    return dict(march=march, back_off=c["back_off"], max_gap=c["max_gap"], miss=float(F32(march.tfar) - F32(step)),
                min_dist=-math.inf)


def check_opts(o):
    """ValueError on what gpis*_view_gain_* refuses with GPIS_ERR_ARG past the march's own refusals."""
    # (cover's checks of back_off and max_gap; its other options are given values it accepts)
    cover_ref.check_opts(dict(back_off=o["back_off"], max_gap=o["max_gap"], clearance=float(np.finfo(F32).max), min_size=1, max_rounds=0))
    if math.isnan(o["min_dist"]):
        raise ValueError("min_dist")


MARCH = ("tnear", "tfar", "min_step", "max_step", "slack", "refine", "max_steps")


def _opts(dim, step, opts):
    """The defaults with the given options replaced; the march's fields are taken by name."""
    o = default_opts(dim, step)
    for k in opts:
        if k not in o and k not in MARCH:
            raise TypeError("unknown option %r" % k)
    o.update({k: v for k, v in opts.items() if k not in MARCH})
    mk = {k: v for k, v in opts.items() if k in MARCH}
    if mk:
        o["march"] = render_field_ref.Opts(dim, step, **mk)
    check_opts(o)
    return o


def predicted(depth, status, miss):
    """(d' float32, hits): the measurement a ray without a return is given, and the number of rays with one."""
    hit = np.asarray(status) == 0
    return np.where(hit, np.asarray(depth, F32), F32(miss)).astype(F32), int(hit.sum())


def targets(seen, dist, min_dist):
    with np.errstate(invalid="ignore"):
        return (np.asarray(seen).ravel() == 0) & ~(np.ascontiguousarray(dist, F32).ravel() < F32(min_dist))


def gain_depth(dist, seen, shape, origin, step, cam6, poses12, **opts):
    """(gain int64 [m], hits int32 [m], d' float32 [m, W*H]) of the poses [m, 12]."""
    o = _opts(3, step, opts)
    P = np.ascontiguousarray(poses12, F32).reshape(-1, 12)
    tg = targets(seen, dist, o["min_dist"])
    gain, hits, pred = np.zeros(len(P), np.int64), np.zeros(len(P), np.int32), []
    for k, p in enumerate(P):
        depth, _, status, _ = render_field_ref.render_depth(dist, shape, origin, step, cam6, p, opts=o["march"])
        d, hits[k] = predicted(depth, status, o["miss"])
        gain[k] = np.count_nonzero(tg & cover_ref.depth_mask(shape, origin, step, d, cam6, p, o["back_off"]))
        pred.append(d)
    return gain, hits, np.stack(pred)


def gain_scan(dist, seen, shape, origin, step, thetas, off2, poses6, **opts):
    """(gain int64 [m], hits int32 [m], d' float32 [m, n]) of the poses [m, 6]."""
    o = _opts(2, step, opts)
    P = np.ascontiguousarray(poses6, F32).reshape(-1, 6)
    tg = targets(seen, dist, o["min_dist"])
    gain, hits, pred = np.zeros(len(P), np.int64), np.zeros(len(P), np.int32), []
    for k, p in enumerate(P):
        rng, _, status, _ = render_field_ref.render_scan(dist, shape, origin, step, thetas, p, off2, opts=o["march"])
        d, hits[k] = predicted(rng, status, o["miss"])
        gain[k] = np.count_nonzero(tg & cover_ref.scan_mask(shape, origin, step, thetas, d, p, off2, o["back_off"], o["max_gap"]))
        pred.append(d)
    return gain, hits, np.stack(pred)
