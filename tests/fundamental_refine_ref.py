"""numpy fp64 restatement of roma_amd.geometry.refine_fundamental (csrc/fundamental_refine.hip): Levenberg-Marquardt on the truncated
Sampson cost of a fundamental matrix, with the kernel's normalisation, parameterisation, analytic Jacobian, schedule and failure
rules (the cyclic Jacobi of the initial factorisation included, so that both start from the same U, V).  The two differ in the order
of their sums, in where the compiler fuses a multiply-add and in the last bits of sqrt and division, nothing else.

Model F^ = U diag(1, s, 0) V^T in Hartley-normalised coordinates, U, V in SO(3); seven parameters (w_u, w_v, ds): U <- U exp([w_u]x),
V <- V exp([w_v]x) (each |w| limited to 1 rad), s <- s + ds.  The model in pixels is sign_fixed(T_B^T F^ T_A).  Residual of a pixel
match r = x_B^T F x_A / sqrt((F x_A)_1^2 + (F x_A)_2^2 + (F^T x_B)_1^2 + (F^T x_B)_2^2) (the F branch of geometry_ref.errors is
r^2); cost = sum of min(r^2, thr^2) over the usable matches (finite, and allowed by the optional mask); weight 1 where r^2 < thr^2."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G
from tests.lm_ref import ACCEPT_REL, LAMBDA0, LAMBDA_MIN, cholesky_solve, same_bits, schedule, usable  # noqa: F401  (shared by the three)
from tests.pose_refine_ref import exp_so3

MIN_MATCHES = 8
RANK_TOL = 1e-14                   # sigma_2^2 <= RANK_TOL sigma_1^2: no second singular value (the eigenvalues carry ~eps sigma_1^2)
JACOBI_SWEEPS = 10
NPAR = 7


def normalisation(xa, xb, ok):
    """(T_A, T_B) over the usable matches, as geometry_ref.normalisation"""
    return G.transform(G.normalisation(xa, ok)), G.transform(G.normalisation(xb, ok))


def jacobi(A):
    """cyclic Jacobi of ransac_common.h's jacobi_lds: -> (eigenvalues, eigenvectors in columns), unsorted"""
    A = np.array(A, float)
    n = len(A)
    V = np.eye(n)
    for _ in range(JACOBI_SWEEPS):
        for p in range(n - 1):
            for q in range(p + 1, n):
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                if apq == 0.0:
                    continue
                theta = (aqq - app) / (2.0 * apq)
                t = 0.5 / theta if abs(theta) > 1e150 else (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                akp, akq, vp, vq = A[:, p].copy(), A[:, q].copy(), V[:, p].copy(), V[:, q].copy()
                for k in range(n):
                    if k == p:
                        A[p, p] = app - t * apq
                        A[p, q] = A[q, p] = 0.0
                    elif k == q:
                        A[q, q] = aqq + t * apq
                    else:
                        A[k, p] = A[p, k] = c * akp[k] - s * akq[k]
                        A[k, q] = A[q, k] = s * akp[k] + c * akq[k]
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq
    return np.diag(A).copy(), V


def factorise(F, TA, TB):
    """pixels -> (U, s, V) with T_B^-T F T_A^-1 ~ U diag(1, s, 0) V^T; None without a second singular value"""
    Fh = np.linalg.inv(TB).T @ F @ np.linalg.inv(TA)
    w, E = jacobi(Fh.T @ Fh)
    i1 = int(np.argmax(w))                                   # first index on ties, as the kernel
    i3 = int(np.argmin(w))
    if i1 == i3:
        i1, i3 = 0, 2
    V = E[:, [i1, 3 - i1 - i3, i3]]
    if np.linalg.det(V) < 0.0:
        V[:, 2] = -V[:, 2]
    u1, u2 = Fh @ V[:, 0], Fh @ V[:, 1]
    s1, s2 = np.sqrt(u1 @ u1), np.sqrt(u2 @ u2)
    if not (np.isfinite(s1) and np.isfinite(s2) and s1 > 0.0 and s2 * s2 > RANK_TOL * (s1 * s1)):
        return None
    u1, u2 = u1 / s1, u2 / s2
    return np.stack([u1, u2, np.cross(u1, u2)], 1), s2 / s1, V


def hat_matrices(U, s, V):
    """F^ and its derivatives by (w_u, w_v, ds) at zero -> (8,3,3)"""
    u, v = U.T, V.T                                          # rows: the columns u_i, v_i
    o = np.outer
    return np.stack([o(u[0], v[0]) + s * o(u[1], v[1]),
                     s * o(u[2], v[1]), -o(u[2], v[0]), o(u[1], v[0]) - s * o(u[0], v[1]),
                     s * o(u[1], v[2]), -o(u[0], v[2]), o(u[0], v[1]) - s * o(u[1], v[0]),
                     o(u[1], v[1])])


def pixel_model(U, s, V, TA, TB):
    """the model as it is returned: unit Frobenius norm, largest-magnitude entry positive"""
    return G.sign_fixed(TB.T @ hat_matrices(U, s, V)[0] @ TA)


def step(U, s, V, delta):
    return U @ exp_so3(delta[:3]), s + delta[6], V @ exp_so3(delta[3:6])


def _terms(M, xa, xb):
    ha = np.concatenate([xa, np.ones_like(xa[:, :1])], -1)
    hb = np.concatenate([xb, np.ones_like(xb[:, :1])], -1)
    Mx = np.einsum("kij,nj->kni", M, ha)                     # M_k x_A
    Mt = np.einsum("kji,nj->kni", M, hb)[..., :2]            # first two entries of M_k^T x_B
    return hb, Mx, Mt


def residuals(F, xa, xb):
    """r (N,) of the pixel-space model F; NaN where the match or r is not finite"""
    with np.errstate(all="ignore"):
        hb, Mx, Mt = _terms(np.asarray(F, float)[None], xa, xb)
        n = (hb * Mx[0]).sum(-1)
        d = Mx[0, :, 0] ** 2 + Mx[0, :, 1] ** 2 + Mt[0, :, 0] ** 2 + Mt[0, :, 1] ** 2
        return n / np.sqrt(d)


def residuals_and_jacobian(U, s, V, TA, TB, xa, xb):
    """r (N,) and dr/d(w_u, w_v, ds) (N,7) of T_B^T F^ T_A"""
    M = np.stack([TB.T @ h @ TA for h in hat_matrices(U, s, V)])
    with np.errstate(all="ignore"):
        hb, Mx, Mt = _terms(M, xa, xb)
        n = (hb * Mx[0]).sum(-1)
        d = Mx[0, :, 0] ** 2 + Mx[0, :, 1] ** 2 + Mt[0, :, 0] ** 2 + Mt[0, :, 1] ** 2
        isd = 1.0 / np.sqrt(d)
        dn = (hb[None] * Mx[1:]).sum(-1)                                                   # (7,N)
        dd = 2.0 * (Mx[0, :, 0] * Mx[1:, :, 0] + Mx[0, :, 1] * Mx[1:, :, 1] + Mt[0, :, 0] * Mt[1:, :, 0] + Mt[0, :, 1] * Mt[1:, :, 1])
        J = dn * isd - (n * (0.5 * isd / d)) * dd
    return n * isd, J.T


def cost_of(F, xa, xb, thr, ok):
    """-> (truncated cost, inlier count, inlier mask, r^2) of the pixel-space model F over the usable matches `ok`"""
    t2 = thr * thr
    with np.errstate(all="ignore"):
        r2 = residuals(F, xa, xb) ** 2
        w = ok & (r2 < t2)
    return float(np.where(w, r2, t2)[ok].sum()), int(w.sum()), w, r2


def truncated_cost(F, xa, xb, thr, mask=None):
    return cost_of(F, xa, xb, thr, usable(xa, xb, mask))[0]


def normal_equations(U, s, V, TA, TB, xa, xb, thr, ok):
    r, J = residuals_and_jacobian(U, s, V, TA, TB, xa, xb)
    with np.errstate(invalid="ignore"):
        w = ok & (r * r < thr * thr)
    return J[w].T @ J[w], J[w].T @ r[w]


def refine(F0, xa, xb, thr, iters=15, mask=None):
    """One pair, pixels (N,2).  Returns a dict: F, mask, cost, count, steps (kept), costs (the cost of the input and after every kept
    step), cost0 (of the input as given).  Without a kept step — and with fewer than 8 weighted matches, a Cholesky pivot that is not
    positive, an input that is not finite or has no second singular value — the input is returned as it came."""
    F0 = np.asarray(F0, float)
    ok = usable(xa, xb, mask)
    cost, cnt, w, _ = cost_of(F0, xa, xb, thr, ok)
    start = dict(F=F0, mask=w, cost=cost, count=cnt, steps=0, costs=[cost], cost0=cost)
    if not np.isfinite(F0).all() or cnt < MIN_MATCHES:
        return start
    TA, TB = normalisation(xa, xb, ok)
    with np.errstate(all="ignore"):
        fac = factorise(F0, TA, TB)
    if fac is None:
        return start

    def propose(state, delta):
        U, s, V = state[:3]
        Uc, sc, Vc = step(U, s, V, delta)
        if same_bits(Uc, U) and same_bits(Vc, V) and same_bits(sc, s):
            return None
        return Uc, sc, Vc, pixel_model(Uc, sc, Vc, TA, TB)

    out = schedule((*fac, F0), cost, cnt, w, iters, lambda state, _: normal_equations(*state[:3], TA, TB, xa, xb, thr, ok), propose,
                   lambda state: (*cost_of(state[3], xa, xb, thr, ok)[:3], None))
    if out is None:
        return start
    (_, _, _, F), cost, cnt, w, steps, costs = out
    return dict(F=F, mask=w, cost=cost, count=cnt, steps=steps, costs=costs, cost0=costs[0])
