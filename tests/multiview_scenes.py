"""Multi-view scenes for tests/test_triangulate_nview.py (numpy only).

View 0 is the identity under general_scenes.K_A (1024 x 768).  Views 1, 2, ... cycle through general_scenes.MOTIONS and alternate
K_B (800 x 600) / K_A; each lap of the four motions has a longer baseline (BASELINE = 2, then 2.25, 2.5, ... times the unit translation),
and every second lap has its sign flipped (the camera on the other side).  The first baseline is 2 and not 1 because of the forward
motion: image B is less tall than image A, so points in the top and bottom strips of image 0 are seen by views 0 and 2 only, and at
depth 12, 340 px from the epipole, a forward baseline of 1 gives them 1.65 to 2 degrees of parallax — below what the tests compare.  Points are uniform over image 0 at depths 4-12.  An observation
exists where the point is in front of the view (z > 0.5) and inside its image, elsewhere it is NaN; noise sigma = 0.5 px on every
observation; a 10 % share of the observations of views >= 1 is replaced by outliers uniform over the image.  `offset` moves the world's
origin: X <- X + offset, t_v <- t_v - R_v offset — the same cameras, the same pixels."""
from __future__ import annotations

import numpy as np

from tests import general_scenes as GS
from tests import geometry_ref as G

BASELINE = 2.0
WORLD_OFFSET = np.array([1.0e4, -2.0e4, 5.0e3])


def cameras(V, seed):
    """K (V,3,3), R (V,3,3), t (V,3), sizes (V,2) = (W, H)"""
    rng = np.random.default_rng([seed, 7])
    names = list(GS.MOTIONS)
    K, R, t, sizes = [GS.K_A], [np.eye(3)], [np.zeros(3)], [(GS.W_A, GS.H_A)]
    for v in range(1, V):
        lap, which = divmod(v - 1, len(names))
        w, tt = GS.MOTIONS[names[which]]
        tt = np.array(tt) / np.linalg.norm(tt)
        R.append(G.rodrigues(np.array(w) + 0.01 * rng.normal(size=3)))
        t.append((-1.0 if lap % 2 else 1.0) * (BASELINE + 0.25 * lap) * tt)
        K.append(GS.K_B if v % 2 else GS.K_A)
        sizes.append((GS.W_B, GS.H_B) if v % 2 else (GS.W_A, GS.H_A))
    return np.stack(K), np.stack(R), np.stack(t), np.array(sizes, dtype=np.float64)


def multiview_scene(V, seed, N=2000, sigma=0.5, outlier_frac=0.1, offset=None):
    """-> dict: x (V,N,2) float32 observations (NaN = not seen), clean (V,N,2) fp64 exact projections where seen, seen (V,N) bool,
    outlier (V,N) bool, X (N,3) the true points in the world frame, K, R, t, sizes."""
    K, R, t, sizes = cameras(V, seed)
    rng = np.random.default_rng([seed, 11])
    u = np.stack([rng.uniform(0, GS.W_A, N), rng.uniform(0, GS.H_A, N)], -1)
    X = GS.backproject(u, rng.uniform(4, 12, N), GS.K_A)
    clean, seen = np.full((V, N, 2), np.nan), np.zeros((V, N), bool)
    for v in range(V):
        q = X @ R[v].T + t[v]
        with np.errstate(all="ignore"):
            p = GS.project(q, K[v])
        seen[v] = (q[:, 2] > 0.5) & (p[:, 0] >= 0) & (p[:, 0] < sizes[v, 0]) & (p[:, 1] >= 0) & (p[:, 1] < sizes[v, 1])
        clean[v] = np.where(seen[v, :, None], p, np.nan)
    x = clean + rng.normal(0, sigma, clean.shape)
    outlier = seen & (rng.random((V, N)) < outlier_frac)
    outlier[0] = False
    wild = np.stack([rng.uniform(0, 1, (V, N)) * sizes[:, 0:1], rng.uniform(0, 1, (V, N)) * sizes[:, 1:2]], -1)
    x = np.where(outlier[..., None], wild, x)
    if offset is not None:
        offset = np.asarray(offset, np.float64)
        X = X + offset
        t = t - np.einsum("vij,j->vi", R, offset)
    return {"x": x.astype(np.float32), "clean": clean, "seen": seen, "outlier": outlier, "X": X, "K": K, "R": R, "t": t, "sizes": sizes}
