"""numpy restatement of the calibrated two-view estimator of roma_amd.geometry (csrc/essential.hip): the sample draw with stage 4
bit for bit, a 5-point solver (null space by SVD, the ten cubic constraints, action matrix of multiplication by x, np.linalg.eig —
independent of the kernel's hidden-variable finish), the projection onto the essential manifold, the four-candidate decomposition
with its cheirality count, the whole RANSAC, and the pose errors of the reference (romatch/utils/utils.py:116-134).  The scenes are
two_view_scene of tests/geometry_ref.py; scene_pose re-derives their K, R, t."""
from __future__ import annotations

import itertools

import numpy as np

from tests import geometry_ref as G

M32 = 0xFFFFFFFF
STAGE_E, S_E, SLOTS_E = 4, 5, 10
K_SCENE = np.array([[800.0, 0, G.W_IMG / 2], [0, 800.0, G.H_IMG / 2], [0, 0, 1]])

# monomials of degree <= 3 in (x, y, z) as multisets over (x, y, z, 1) = (0, 1, 2, 3):
# x^3 x^2y x^2z xy^2 xyz xz^2 y^3 y^2z yz^2 z^3 | x^2 xy xz y^2 yz z^2 x y z 1
MONOMIALS = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (0, 2, 2), (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 2, 2),
             (0, 0, 3), (0, 1, 3), (0, 2, 3), (1, 1, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]


def scene_pose(seed):
    """K, R, t of G.two_view_scene(seed, ...): K is fixed, R and t are the first draws of its default_rng(seed) stream."""
    rng = np.random.default_rng(seed)
    R = G.rodrigues(rng.normal(size=3) * 0.08)
    t = np.array([1.0, 0.1 * rng.normal(), 0.1 * rng.normal()])
    return K_SCENE.copy(), R, t


def essential_from_pose(R, t):
    return G.sign_fixed(G.skew(t) @ R)


def calibrate(x, K):
    """x_hat = K^-1 x for (..., 2) pixel coordinates and an upper-triangular K with last row 0 0 1."""
    Ki = np.linalg.inv(K)
    h = np.concatenate([x, np.ones_like(x[..., :1])], -1) @ Ki.T
    return h[..., :2]


def minimal_samples(xa, xb, iters, seed, p0=0):
    """(P,N,2) -> (P, iters, 5) int32, rows of -1 for invalid samples: the draw of geometry.hip with S = 5 and stage 4."""
    P, N = xa.shape[0], xa.shape[1]
    ok_pt = G.usable(xa, xb)
    stream = int(G.fmix32((int(seed) & M32) ^ ((STAGE_E * 0x9E3779B9) & M32)))
    p = np.arange(p0, p0 + P, dtype=np.uint64)[:, None]
    h = np.arange(iters, dtype=np.uint64)[None, :]
    idx = np.full((P, iters, S_E), -1, dtype=np.int64)
    for k in range(S_E):
        ctr = ((p * np.uint64(iters) + h) * np.uint64(8) + np.uint64(k)) & M32
        got = np.full((P, iters), -1, dtype=np.int64)
        for att in range(16):
            hs = G.fmix32((np.uint64(stream) + ctr * np.uint64(0x9E3779B1) + np.uint64(att * 0x7FEB352D)) & M32)
            i = ((hs * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
            good = ok_pt[np.arange(P)[:, None], i]
            for j in range(k):
                good &= idx[:, :, j] != i
            take = (got < 0) & good
            got[take] = i[take]
        idx[:, :, k] = got
    bad = (idx < 0).any(-1)
    idx[bad] = -1
    return idx.astype(np.int32)


def _trilinear(P, Q, R):
    """the ten cubic constraints as a trilinear form T with T(E, E, E) = (det E, 2 E E^T E - tr(E E^T) E)"""
    det = np.dot(P[0], np.cross(Q[1], R[2]))
    PQ = P @ Q.T
    return np.concatenate([[det], (2.0 * PQ @ R - np.trace(PQ) * R).reshape(9)])


def constraint_matrix(basis):
    """basis (4,3,3) = X, Y, Z, W of E = xX + yY + zZ + W -> the 10 x 20 matrix over MONOMIALS (by polarisation: the coefficient of
    v_a v_b v_c is the sum of T over the distinct orders of (a, b, c))."""
    M = np.zeros((10, 20))
    for j, abc in enumerate(MONOMIALS):
        for perm in set(itertools.permutations(abc)):
            M[:, j] += _trilinear(basis[perm[0]], basis[perm[1]], basis[perm[2]])
    return M


def five_point(xh, xh2):
    """xh, xh2: (5,2) calibrated points of A and B.  Returns (models: unit-norm 3x3, ordered by increasing x; all 10 eigenvalues;
    condition number of the leading 10 x 10 block of the row-max-scaled constraint matrix)."""
    A = G.f_rows(xh[:, 0], xh[:, 1], xh2[:, 0], xh2[:, 1])
    vt = np.linalg.svd(A)[2]
    basis = vt[5:9].reshape(4, 3, 3)
    M = constraint_matrix(basis)
    M = M / np.abs(M).max(1, keepdims=True)
    cond = np.linalg.cond(M[:, :10])
    if not np.isfinite(cond) or cond > 1e12:
        return [], np.zeros(0, complex), cond
    B = np.linalg.solve(M[:, :10], M[:, 10:])
    # basis of the quotient ring b = [x^2 xy xz y^2 yz z^2 x y z 1]; x b = [x^3 x^2y x^2z xy^2 xyz xz^2 | x^2 xy xz | x]
    Ax = np.zeros((10, 10))
    Ax[:6] = -B[:6]
    Ax[6, 0] = Ax[7, 1] = Ax[8, 2] = Ax[9, 6] = 1.0
    w, V = np.linalg.eig(Ax)
    models = []
    for k in np.argsort(w.real):
        if abs(w[k].imag) > 1e-10 * max(1.0, abs(w[k])) or abs(V[9, k]) == 0:
            continue
        v = (V[:, k] / V[9, k]).real
        models.append(G.unit(v[6] * basis[0] + v[7] * basis[1] + v[8] * basis[2] + basis[3]))
    return models, w, cond


def well_conditioned(w, cond):
    """the predicate of tests/test_pose.py: condition <= 1e6 and every root separated — real roots from each other, complex roots
    from the real axis — by more than 1e-4 relative to max(1, |root|)."""
    if not cond <= 1e6 or len(w) != 10:
        return False
    scale = np.maximum(1.0, np.abs(w))
    real = np.abs(w.imag) <= 1e-10 * scale
    if (np.abs(w.imag[~real]) <= 1e-4 * scale[~real]).any():
        return False
    r = np.sort(w.real[real])
    return bool((np.diff(r) > 1e-4 * np.maximum(1.0, np.abs(r[1:]))).all())


def project_essential(M):
    U, _, Vt = np.linalg.svd(M)
    return G.unit(U @ np.diag([1.0, 1.0, 0.0]) @ Vt)


def decompose(E):
    """the four (R, t) candidates in the order (W,+) (W,-) (W^T,+) (W^T,-)"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    t = U[:, 2]
    return [(U @ W @ Vt, t), (U @ W @ Vt, -t), (U @ W.T @ Vt, t), (U @ W.T @ Vt, -t)]


def depths(R, t, xh, xh2):
    """least-squares depths (lambda_A, lambda_B) of lambda_B x_B = lambda_A R x_A + t, x_A, x_B homogeneous calibrated points"""
    a = np.concatenate([xh, np.ones_like(xh[..., :1])], -1) @ R.T
    b = np.concatenate([xh2, np.ones_like(xh2[..., :1])], -1)
    aa, bb, ab = (a * a).sum(-1), (b * b).sum(-1), (a * b).sum(-1)
    at, bt = a @ t, b @ t
    with np.errstate(all="ignore"):
        det = aa * bb - ab * ab
        return (ab * bt - bb * at) / det, (aa * bt - ab * at) / det


def recover_pose(E, xa, xb, KA, KB, mask=None):
    """-> (R, t, narrowed mask, count): the candidate with the most masked matches of positive depth in both cameras."""
    N = xa.shape[0]
    mask = np.ones(N, bool) if mask is None else np.asarray(mask, bool)
    if not np.isfinite(E).all() or not np.abs(E).max() > 0:
        return np.eye(3), np.zeros(3), np.zeros(N, bool), 0
    xh, xh2 = calibrate(xa, KA), calibrate(xb, KB)
    best = None
    for R, t in decompose(E):
        la, lb = depths(R, t, xh, xh2)
        ok = mask & np.isfinite(la) & np.isfinite(lb) & (la > 0) & (lb > 0)
        if best is None or ok.sum() > best[3]:
            best = (R, t, ok, int(ok.sum()))
    return best


def ransac_essential(xa, xb, KA, KB, threshold, iters, seed, lo_iters=3):
    """One pair (N,2) pixels -> (E (3,3) unit norm, sign-fixed, in calibrated coordinates; inlier mask).  fp64 throughout."""
    N = xa.shape[0]
    xh, xh2 = calibrate(xa, KA), calibrate(xb, KB)
    idx = minimal_samples(xa[None], xb[None], iters, seed)[0]
    t2 = threshold ** 2
    cands = []
    for h in range(iters):
        if idx[h, 0] >= 0:
            cands += five_point(xh[idx[h]], xh2[idx[h]])[0]
    if not cands:
        return np.zeros((3, 3)), np.zeros(N, dtype=bool)
    e = G.errors("fundamental", np.stack(cands), xh, xh2)
    inl = e < t2
    cost = np.where(inl, e, t2).sum(-1)
    best = int(np.argmin(cost))
    cur, cc, cin = cands[best], cost[best], inl[best]
    for _ in range(lo_iters):
        if cin.sum() < 8:
            break
        i = np.nonzero(cin)[0]
        rows = G.f_rows(xh[i, 0], xh[i, 1], xh2[i, 0], xh2[i, 1])
        cand = project_essential(np.linalg.eigh(rows.T @ rows)[1][:, 0].reshape(3, 3))
        e2 = G.errors("fundamental", cand, xh, xh2)
        in2 = e2 < t2
        c2 = np.where(in2, e2, t2).sum()
        if not c2 < cc:
            break
        cur, cc, cin = cand, c2, in2
    E = G.sign_fixed(project_essential(cur))
    return E, G.errors("fundamental", E, xh, xh2) < t2


def truth_aware_fit(xa, xb, truth, KA, KB):
    """least squares on the TRUE inliers in calibrated coordinates -> essential projection -> cheirality choice (no RANSAC):
    the yardstick the scene tests print next to the estimator's errors."""
    xh, xh2 = calibrate(xa[truth], KA), calibrate(xb[truth], KB)
    rows = G.f_rows(xh[:, 0], xh[:, 1], xh2[:, 0], xh2[:, 1])
    E = project_essential(np.linalg.eigh(rows.T @ rows)[1][:, 0].reshape(3, 3))
    return recover_pose(E, xa, xb, KA, KB, truth)[:2]


def rotation_error_deg(R, R_true):
    c = np.clip((np.trace(R.T @ R_true) - 1) / 2, -1.0, 1.0)
    return float(np.rad2deg(np.abs(np.arccos(c))))


def translation_error_deg(t, t_true):
    """angle between the translation directions, folded by the sign ambiguity of E as compute_pose_error does"""
    n = np.linalg.norm(t) * np.linalg.norm(t_true)
    e = float(np.rad2deg(np.arccos(np.clip(np.dot(t, t_true) / n, -1.0, 1.0))))
    return min(e, 180.0 - e)
