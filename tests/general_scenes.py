"""Two-view scenes with two DIFFERENT, general cameras and four motion families, for tests/test_general_cameras.py (numpy only).

two_view_scene / planar_scene of tests/geometry_ref.py use one camera (fx = fy, no skew, centred principal point) for both images of
one size and one sideways motion.  Here image A is 1024 x 768 under K_A and image B is 800 x 600 under K_B, both with fx != fy, skew
and an off-centre principal point, and the motion is one of MOTIONS: sideways, forward (epipole inside both images), backward and
up, and a 25 degree turn.  The structure is that of two_view_scene: inliers uniform over image A at depths 4-12, kept if in front of
B (z > 0.5) and inside image B; outliers uniform over each image; noise added; everything permuted."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G

W_A, H_A = 1024, 768
W_B, H_B = 800, 600
K_A = np.array([[820.0, 1.5, 530.0], [0.0, 790.0, 370.0], [0.0, 0.0, 1.0]])
K_B = np.array([[610.0, -0.8, 390.0], [0.0, 655.0, 310.0], [0.0, 0.0, 1.0]])
# 1.5 px in calibrated units by the documented rule of estimate_relative_pose: (1/f_A + 1/f_B) / 2 with f = (fx + fy) / 2
THR_G = 1.5 * 0.5 * (1 / 805 + 1 / 632.5)

# rotation vector; t before normalisation
MOTIONS = {
    "sideways": ((0.02, -0.05, 0.03), (1.0, 0.1, -0.05)),
    "forward": ((0.03, 0.04, -0.06), (0.08, -0.05, 1.0)),
    "backward_up": ((-0.05, 0.02, 0.1), (0.1, 0.7, -0.7)),
    "turn": ((0.05, -0.45, 0.2), (1.0, 0.05, 0.35)),
}


def no_skew(K):
    K = np.array(K, dtype=np.float64)
    K[0, 1] = 0.0
    return K


def calibrated_threshold(px, KA, KB):
    """px pixels in calibrated units for cameras KA, KB (the rule above)"""
    return px * 0.5 * (2.0 / (KA[0, 0] + KA[1, 1]) + 2.0 / (KB[0, 0] + KB[1, 1]))


def scene_pose(motion, seed):
    """R, t (unit) of general_scene(motion, seed, ...): the table value plus the first draw of its default_rng(seed) stream"""
    w, t = MOTIONS[motion]
    rng = np.random.default_rng(seed)
    R = G.rodrigues(np.array(w) + 0.01 * rng.normal(size=3))
    t = np.array(t)
    return R, t / np.linalg.norm(t)


def fundamental_from_pose(R, t, KA=K_A, KB=K_B):
    """F in pixels (x_B^T F x_A = 0), unit norm, sign fixed"""
    return G.sign_fixed(np.linalg.inv(KB).T @ G.skew(t) @ R @ np.linalg.inv(KA))


def _uniform(rng, w, h, n):
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], -1)


def project(X, K):
    u = X @ K.T
    return u[:, :2] / u[:, 2:3]


def backproject(u, d, K):
    return (np.concatenate([u, np.ones((len(u), 1))], -1) @ np.linalg.inv(K).T) * d[:, None]


def general_scene(motion, seed, N=2000, outlier_frac=0.3, sigma=0.5, KA=K_A, KB=K_B):
    """-> xa, xb (N,2) pixels, is_inlier (N,), R, t (unit).  sigma = 0 gives the same scene without noise (the same draws, the same
    permutation): the clean points of the noisy one."""
    rng = np.random.default_rng(seed)
    w, t = MOTIONS[motion]
    R = G.rodrigues(np.array(w) + 0.01 * rng.normal(size=3))
    t = np.array(t) / np.linalg.norm(t)
    n_in = int(round(N * (1 - outlier_frac)))
    pa, pb = [], []
    while sum(len(a) for a in pa) < n_in:
        u = _uniform(rng, W_A, H_A, 4 * n_in)
        Xb = backproject(u, rng.uniform(4, 12, 4 * n_in), KA) @ R.T + t
        ub = project(Xb, KB)
        keep = (Xb[:, 2] > 0.5) & (ub[:, 0] >= 0) & (ub[:, 0] < W_B) & (ub[:, 1] >= 0) & (ub[:, 1] < H_B)
        pa.append(u[keep])
        pb.append(ub[keep])
    ca, cb = np.concatenate(pa)[:n_in], np.concatenate(pb)[:n_in]
    n_out = N - n_in
    oa, ob = _uniform(rng, W_A, H_A, n_out), _uniform(rng, W_B, H_B, n_out)
    xa = np.concatenate([ca + rng.normal(0, sigma, ca.shape), oa])
    xb = np.concatenate([cb + rng.normal(0, sigma, cb.shape), ob])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(N)
    return xa[perm], xb[perm], truth[perm], R, t


def exact_scene(motion, seed, N=400, sign=1.0, KA=K_A, KB=K_B):
    """Exact projections of points at depths 4-12 uniform over image A, wherever they land in B; `sign` = -1 puts camera B on the
    other side.  -> xa, xb, R, t (unit)"""
    R, t = scene_pose(motion, seed)
    t = sign * t
    rng = np.random.default_rng([seed, 1])
    u = _uniform(rng, W_A, H_A, N)
    return u, project(backproject(u, rng.uniform(4, 12, N), KA) @ R.T + t, KB), R, t


def general_planar_scene(seed, N=2000, outlier_frac=0.4, sigma=0.5):
    """H maps the corners of image A to the corners of image B, each moved by up to 60 px; the rest as planar_scene, with the outliers
    of B uniform over 800 x 600.  -> xa, xb, is_inlier, H_true"""
    rng = np.random.default_rng(seed)
    src = np.array([[0, 0], [W_A, 0], [W_A, H_A], [0, H_A]], dtype=np.float64)
    dst = np.array([[0, 0], [W_B, 0], [W_B, H_B], [0, H_B]], dtype=np.float64) + rng.uniform(-60, 60, src.shape)
    H = np.linalg.svd(G.h_rows(src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))[2][-1].reshape(3, 3)
    H = H / H[2, 2]
    n_in = int(round(N * (1 - outlier_frac)))
    ca = _uniform(rng, W_A, H_A, n_in)
    hb = np.concatenate([ca, np.ones((n_in, 1))], -1) @ H.T
    cb = hb[:, :2] / hb[:, 2:3]
    n_out = N - n_in
    oa, ob = _uniform(rng, W_A, H_A, n_out), _uniform(rng, W_B, H_B, n_out)
    xa = np.concatenate([ca + rng.normal(0, sigma, ca.shape), oa])
    xb = np.concatenate([cb + rng.normal(0, sigma, cb.shape), ob])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(N)
    return xa[perm], xb[perm], truth[perm], H
