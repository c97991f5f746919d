"""Analytic depth maps of V views for tests/test_fuse_depth.py (numpy only).

The world: a slanted plane z = 8 + 0.3 x + 0.2 y behind a nearer rectangle |x| < 1.3, |y| < 1.0 in the plane z = 5 + 0.1 x — occlusions
and depth discontinuities.  Every map is rendered by ray intersection: the ray of pixel (row i, column j) leaves the camera centre
through (j + 0.5, i + 0.5) and takes the nearer of the two surfaces; `surface` says which (0 the plane, 1 the rectangle).
Cameras: view 0 is the identity; the others have small general motions (a rotation of about 0.04 rad about a random axis, a translation
of about 0.35 in a random direction, the forward component included); every view has a K of its own with unequal focal lengths, skew and
principal point, given for an image of `image` = (H_img, W_img) while the map has `shape` — the default is the map's own shape.
Perturbations (perturb=True): multiplicative Gaussian depth noise of 0.3 %, then 5 % of the pixels scaled by 1.3 (wrong depths, `wrong`),
then 5 % holes (depth 0, `hole`); noise=False leaves the Gaussian noise out and keeps the other two.  `offset` moves the world's origin
by multiview_scenes.WORLD_OFFSET: X <- X + offset, t_v <- t_v - R_v offset — the same cameras and maps.

fuse_scene(...) also runs the restatement (tests/fuse_depth_ref.py) and ASSERTS that none of its decisions lies within 1e-6 of its
threshold (pixels, relative depth, q.z, p.z, the tap region) and that no ownership lookup lies within 1e-6 of a pixel border, so that a
device result may be compared with it for equality.  Scenes are cached: callers read them and leave them as they are."""
from __future__ import annotations

import functools

import numpy as np

from tests import fuse_depth_ref as FR
from tests import geometry_ref as G
from tests.multiview_scenes import WORLD_OFFSET

PLANE_N, PLANE_C = np.array([-0.3, -0.2, 1.0]), 8.0              # n . X = c
RECT_N, RECT_C, RECT_X, RECT_Y = np.array([-0.1, 0.0, 1.0]), 5.0, 1.3, 1.0
NOISE, WRONG_FRAC, WRONG_SCALE, HOLE_FRAC = 0.003, 0.05, 1.3, 0.05
MARGIN = 1e-6


def cameras(V, seed, image):
    """K (V,3,3) for an image of `image` = (H, W), R (V,3,3), t (V,3)"""
    rng = np.random.default_rng([seed, 3])
    H, W = image
    K, R, t = [], [], []
    for v in range(V):
        f = 0.95 * W * (1.0 + 0.08 * rng.uniform(-1, 1))
        K.append(np.array([[f, 0.01 * f * rng.uniform(-1, 1), W / 2 + 0.04 * W * rng.uniform(-1, 1)],
                           [0.0, f * (0.9 + 0.05 * rng.uniform(-1, 1)), H / 2 + 0.04 * H * rng.uniform(-1, 1)], [0.0, 0.0, 1.0]]))
        if v == 0:
            R.append(np.eye(3))
            t.append(np.zeros(3))
        else:
            w, c = rng.normal(size=3), rng.normal(size=3)
            Rv = G.rodrigues(0.04 * w / np.linalg.norm(w))
            R.append(Rv)
            t.append(-Rv @ (0.35 * (1.0 + 0.1 * (v % 4)) * c / np.linalg.norm(c)))
    return np.stack(K), np.stack(R), np.stack(t)


def render(K, R, t, shape, pix=None):
    """-> depth (H,W) fp64 (0 where a ray meets nothing in front), surface (H,W) int (0 plane, 1 rectangle, -1 nothing); with pix (...,2)
    the same for the rays through those pixel coordinates instead of the grid's"""
    if pix is None:
        H, W = shape
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pix = np.stack([jj + 0.5, ii + 0.5], -1)
    pix = np.concatenate([pix, np.ones(pix.shape[:-1] + (1,))], -1)
    d = (pix @ np.linalg.inv(K).T) @ R                           # R^T K^-1 pix: the camera's z grows by 1 per unit along it
    C = -R.T @ t
    lam_p = (PLANE_C - PLANE_N @ C) / (d @ PLANE_N)
    lam_r = (RECT_C - RECT_N @ C) / (d @ RECT_N)
    Xr = C + lam_r[..., None] * d
    on_rect = (lam_r > 0) & (np.abs(Xr[..., 0]) < RECT_X) & (np.abs(Xr[..., 1]) < RECT_Y)
    take_rect = on_rect & ((lam_r < lam_p) | (lam_p <= 0))
    depth = np.where(take_rect, lam_r, np.where(lam_p > 0, lam_p, 0.0))
    surface = np.where(take_rect, 1, np.where(lam_p > 0, 0, -1))
    return depth, surface


def surface_distance(X):
    """distance of world points (N,3) to the nearer of the two surfaces (the plane unbounded, the rectangle bounded)"""
    dp = np.abs(X @ PLANE_N - PLANE_C) / np.linalg.norm(PLANE_N)
    # the rectangle: parametrised by (x, y), z = RECT_C + 0.1 x; the closest point by clamping the foot point (exact up to the slant's
    # second order, far below the noise it is compared with)
    n = RECT_N / np.linalg.norm(RECT_N)
    foot = X - ((X @ RECT_N - RECT_C) / np.linalg.norm(RECT_N))[:, None] * n
    x, y = np.clip(foot[:, 0], -RECT_X, RECT_X), np.clip(foot[:, 1], -RECT_Y, RECT_Y)
    near = np.stack([x, y, RECT_C + 0.1 * x], -1)
    return np.minimum(dp, np.linalg.norm(X - near, axis=-1))


@functools.lru_cache(maxsize=None)
def fuse_scene(V, seed, shapes=((24, 32),), images=None, perturb=True, noise=True, offset=False, min_views=2, max_reproj_error=1.0,
               max_depth_error=0.01, check=True):
    """shapes: one map shape for all views or V of them; images: None (K refers to the map), one image shape or V of them.
    -> dict: depths (list of fp32 maps), clean (fp64, before the perturbations), surface, wrong, hole, K (for the images), R, t, sizes
    (None or the V image shapes), ref (the restatement's result with every emitted pixel in the cloud)."""
    shapes = list(shapes) * V if len(shapes) == 1 else list(shapes)
    assert len(shapes) == V
    sizes = None if images is None else (list(images) * V if len(images) == 1 else list(images))
    K, R, t = [], [], []
    for v in range(V):                                            # one camera draw per image shape, so that every view keeps its own K
        Kv, Rv, tv = cameras(V, seed, shapes[v] if sizes is None else sizes[v])
        K.append(Kv[v]); R.append(Rv[v]); t.append(tv[v])
    K, R, t = np.stack(K), np.stack(R), np.stack(t)
    Kmap = FR.scaled_intrinsics(K, shapes, sizes)
    rng = np.random.default_rng([seed, 5])
    depths, clean, surface, wrong, hole = [], [], [], [], []
    for v in range(V):
        d, s = render(Kmap[v], R[v], t[v], shapes[v])
        clean.append(d)
        surface.append(s)
        w, h = np.zeros(shapes[v], bool), np.zeros(shapes[v], bool)
        if perturb:
            g = rng.normal(size=d.shape)
            d = d * (1.0 + NOISE * g) if noise else d
            w = rng.random(d.shape) < WRONG_FRAC
            d = np.where(w, WRONG_SCALE * d, d)
            h = rng.random(d.shape) < HOLE_FRAC
            d = np.where(h, 0.0, d)
            w = w & ~h
        depths.append(d.astype(np.float32))
        wrong.append(w)
        hole.append(h)
    if offset:
        t = t - np.einsum("vij,j->vi", R, WORLD_OFFSET)
    ref = FR.fuse_depth_ref(depths, R, t, K, sizes=sizes, max_reproj_error=max_reproj_error, max_depth_error=max_depth_error,
                            min_views=min_views)
    if check:
        for name, m in ref["margins"].items():
            assert len(m) == 0 or m.min() >= MARGIN, f"V={V} seed={seed}: a `{name}` decision lies {m.min():.2e} from its threshold"
    return {"depths": depths, "clean": clean, "surface": surface, "wrong": wrong, "hole": hole, "K": K, "R": R, "t": t, "sizes": sizes,
            "shapes": shapes, "ref": ref}
