"""Reference for tracking against a distance field (csrc/track.hip, gpis3_track_depth_field / gpis2_track_scan_field, DESIGN.md
§7f).  There is no arithmetic of its own to restate: the field tracker is the map tracker (tests/track_ref.py) whose test()
answers with the field's sampler (tests/dfield_ref.py).

Contract: track_ref.track_depth / track_scan with
- test_fn(x, res): res[:, 0] = d and res[:, 1:1+dim] = its gradient from dfield_ref.sample(dist, shape, origin, step, x) (all NaN
  outside the lattice), var_f = res[:, 1+dim] = 0;
- Opts(level=0.0, max_var=inf): r = d - 0 = d (the field's level is zero by construction), inlier iff d and the gradient are
  finite and |(double)r| <= max_residual (no variance test: the field applied max_var when it was built).
Everything else -- points, world points, terms, the reduction tree, the solve, the pose update, the loop, statuses and the
final pass -- is track_ref's, bit for bit."""
import math

import numpy as np

import dfield_ref
import track_ref


def field_fn(dist, shape, origin, step):
    """test_fn of track_ref answering from the field (dist of dfield_ref.distance_field or DistanceField.get(), x fastest)."""
    dim = len(shape)

    def fn(x, res):
        s = dfield_ref.sample(dist, shape, origin, step, x)
        res[:, :1 + dim] = s
        res[:, 1 + dim] = 0.0
        return res
    return fn


def opts(dim, **kw):
    return track_ref.Opts(dim, **dict(kw, level=0.0, max_var=math.inf))


def track_depth(dist, shape, origin, step, depth, cam6, pose0, **kw):
    return track_ref.track_depth(field_fn(dist, shape, origin, step), depth, cam6, pose0, opts(3, **kw))


def track_scan(dist, shape, origin, step, thetas, ranges, pose0, off2, **kw):
    return track_ref.track_scan(field_fn(dist, shape, origin, step), thetas, ranges, pose0, off2, opts(2, **kw))


__all__ = ["field_fn", "opts", "track_depth", "track_scan"]
