"""Clouds and cameras for tests/test_render_points.py (numpy only), on the analytic world of tests/depth_scenes.py.

scene(Vs, seed, shape, radius, ...): the cameras are depth_scenes.cameras(Vs + 1, seed, shape); the cloud is every pixel of the first
Vs analytic maps, lifted to the world and rounded to fp32, in the order (view, row, column) — what fuse_depth_maps would emit from
perfect maps without its ownership pass, so surfaces are drawn up to Vs times over.  View Vs contributes no points: it is held out.  The
cloud is drawn into all Vs + 1 views.

The builder runs the restatement (tests/render_points_ref.py) and ASSERTS that no projection lies within 1e-6 of a pixel border or of a
map's edge, that no q.z lies within 1e-6 of 0, that no visibility decision lies within 1e-6 (relative) of its limit, and that wherever a
pixel has a candidate less than 3 fp32 ulps behind its winner neither of the two depths lies within 1e-6 ulp of a point at which its
rounding to fp32 changes (the margin "order" of the restatement) — so that a device result, which differs from the plain chain by fp64
rounding order only, may be compared with it for equality.  Scenes are cached: callers read them and leave them as they are."""
from __future__ import annotations

import functools

import numpy as np

from tests import depth_scenes as DS
from tests import fuse_depth_ref as FR
from tests import render_points_ref as RR

MARGIN = 1e-6
HIDDEN = 1.2                                                       # "more than 20 % behind the surface on its ray"


def assert_margins(ref, what):
    for name, m in ref["margins"].items():
        assert len(m) == 0 or m.min() >= MARGIN, f"{what}: a `{name}` decision lies {m.min():.2e} from its threshold"


def assert_no_ties(ref, shape, radius):
    """no pixel has two candidates of the same fp32 depth: every winner is decided by depth alone, whatever the points' indices"""
    H, W = shape
    for v in range(len(ref["inside"])):
        n = np.flatnonzero(ref["inside"][v])
        pairs = []
        for di in range(-radius, radius + 1):
            for dj in range(-radius, radius + 1):
                ii, jj = ref["row"][v, n] + di, ref["col"][v, n] + dj
                on = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                pairs.append(np.stack([ii[on] * W + jj[on], ref["z32"][v, n[on]].view(np.uint32).astype(np.int64)], -1))
        pairs = np.concatenate(pairs)
        assert len(np.unique(pairs, axis=0)) == len(pairs), f"view {v}: two candidates of a pixel have the same depth"


def cloud_of(K, R, t, shape, views):
    """every pixel of the analytic maps of `views`, lifted; (N,3) fp32 in the order (view, row, column)"""
    H, W = shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pts = []
    for v in views:
        d, _ = DS.render(K[v], R[v], t[v], shape)
        assert (d > 0).all()
        pts.append(FR.lift((jj + 0.5).ravel(), (ii + 0.5).ravel(), d.ravel(), np.linalg.inv(K[v]), R[v], t[v]))
    return np.concatenate(pts).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(Vs, seed, shape=(24, 32), radius=0, depth_tol=0.05, check=True):
    """-> dict: points (N,3) fp32, K, R, t of the Vs + 1 views, shape, radius, depth_tol, ref (the restatement's result)"""
    K, R, t = DS.cameras(Vs + 1, seed, shape)
    points = cloud_of(K, R, t, shape, range(Vs))
    ref = RR.render_points_ref(points, R, t, K, shape, radius=radius, depth_tol=depth_tol)
    if check:
        assert_margins(ref, f"Vs={Vs} seed={seed} shape={shape} radius={radius}")
    return {"points": points, "K": K, "R": R, "t": t, "shape": shape, "radius": radius, "depth_tol": depth_tol, "ref": ref}


def hidden_projections(sc):
    """(V,N) bool: the projections inside a map that the analytic scene puts more than 20 % behind the surface on their ray"""
    ref, (K, R, t) = sc["ref"], (sc["K"], sc["R"], sc["t"])
    X = sc["points"].astype(np.float64)
    out = np.zeros_like(ref["inside"])
    for v in range(len(K)):
        idx = np.flatnonzero(ref["inside"][v])
        q = FR.project(X[idx], K[v], R[v], t[v])
        surf, _ = DS.render(K[v], R[v], t[v], None, pix=q[:, :2] / q[:, 2:])
        out[v, idx] = q[:, 2] > HIDDEN * surf
    return out
