"""numpy fp64 restatement of roma_amd.geometry.refine_pose (csrc/pose_refine.hip): Levenberg-Marquardt on the truncated Sampson cost of
a relative pose, with the kernel's parameterisation, analytic Jacobian, schedule and failure rules.  The two differ in the order of
their sums, in where the compiler fuses a multiply-add and in the last bits of sqrt and division, nothing else.

Pose (R, t), |t| = 1, E = [t]x R.  Five parameters (w, a, b): R <- exp([w]x) R (|w| limited to 1 rad, re-orthonormalised), t <- (t + a b1 + b b2) / |.| with e the coordinate
axis of the smallest |t_i| (lowest index on ties), b1 = (t x e) / |t x e|, b2 = t x b1.  Residual of a calibrated match
r = x_B^T E x_A / sqrt((E x_A)_1^2 + (E x_A)_2^2 + (E^T x_B)_1^2 + (E^T x_B)_2^2); cost = sum of min(r^2, thr^2) over the usable
matches (finite, and allowed by the optional mask); weight 1 where r^2 < thr^2."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G
from tests import pose_ref as PR
from tests.lm_ref import ACCEPT_REL, LAMBDA0, LAMBDA_MIN, cholesky_solve, schedule, usable  # noqa: F401  (the schedule the three refinements share)

MIN_MATCHES = 5
EXP_TERMS = 10


def tangent_basis(t):
    e = np.zeros(3)
    e[int(np.argmin(np.abs(t)))] = 1.0          # argmin: first index on ties
    b1 = np.cross(t, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(t, b1)


def exp_so3(w):
    """I + A K + B K^2 with A = sin(th) / th and B = (1 - cos(th)) / th^2 by their nested series in th^2 (11 terms: exact to rounding
    for th <= 1); a longer w is scaled to 1 rad first."""
    w = np.asarray(w, float)
    th2 = float(w @ w)
    if th2 > 1.0:
        w = w * (1.0 / np.sqrt(th2))
        th2 = float(w @ w)
    A = B = 1.0
    for k in range(EXP_TERMS - 1, -1, -1):
        A = 1.0 - th2 * (1.0 / ((2 * k + 2) * (2 * k + 3))) * A
        B = 1.0 - th2 * (1.0 / ((2 * k + 3) * (2 * k + 4))) * B
    K = G.skew(w)
    return np.eye(3) + A * K + (0.5 * B) * (K @ K)


def orthonormalise(R):
    """Gram-Schmidt on the rows: r0, r1 made orthogonal to r0, r2 = r0 x r1"""
    r0 = R[0] / np.sqrt(R[0] @ R[0])
    r1 = R[1] - (r0 @ R[1]) * r0
    r1 = r1 / np.sqrt(r1 @ r1)
    return np.stack([r0, r1, np.cross(r0, r1)])


def step(R, t, delta):
    b1, b2 = tangent_basis(t)
    tn = t + delta[3] * b1 + delta[4] * b2
    return orthonormalise(exp_so3(delta[:3]) @ R), tn / np.sqrt(tn @ tn)


def model_matrices(R, t):
    """E and its derivatives by (w0, w1, w2, a, b) at zero: [t]x [e_k]x R, [b1]x R, [b2]x R -> (6,3,3)"""
    b1, b2 = tangent_basis(t)
    T = G.skew(t)
    return np.stack([T @ R] + [T @ G.skew(e) @ R for e in np.eye(3)] + [G.skew(b1) @ R, G.skew(b2) @ R])


def residuals(R, t, xh, xh2, jacobian=False):
    """r (N,) and, on request, dr/d(w, a, b) (N,5) of calibrated matches xh <-> xh2 (N,2); NaN where the match or r is not finite."""
    M = model_matrices(R, t)
    ha = np.concatenate([xh, np.ones_like(xh[:, :1])], -1)
    hb = np.concatenate([xh2, np.ones_like(xh2[:, :1])], -1)
    with np.errstate(all="ignore"):
        Mx = np.einsum("kij,nj->kni", M, ha)                 # M_k x_A
        Mt = np.einsum("kji,nj->kni", M, hb)[..., :2]        # first two entries of M_k^T x_B
        n = (hb * Mx[0]).sum(-1)
        d = Mx[0, :, 0] ** 2 + Mx[0, :, 1] ** 2 + Mt[0, :, 0] ** 2 + Mt[0, :, 1] ** 2
        isd = 1.0 / np.sqrt(d)
        r = n * isd
        if not jacobian:
            return r
        dn = (hb[None] * Mx[1:]).sum(-1)                                                   # (5,N)
        dd = 2.0 * (Mx[0, :, 0] * Mx[1:, :, 0] + Mx[0, :, 1] * Mx[1:, :, 1] + Mt[0, :, 0] * Mt[1:, :, 0] + Mt[0, :, 1] * Mt[1:, :, 1])
        J = dn * isd - (n * (0.5 * isd / d)) * dd
    return r, J.T


def evaluate(R, t, xh, xh2, thr, ok):
    """-> (A = J^T J (5,5), g = J^T r (5,), cost, inlier count, inlier mask, r^2) over the usable matches `ok`"""
    r, J = residuals(R, t, xh, xh2, jacobian=True)
    t2 = thr * thr
    with np.errstate(invalid="ignore"):
        r2 = r * r
        w = ok & (r2 < t2)
    cost = float(np.where(w, r2, t2)[ok].sum())
    Jw, rw = J[w], r[w]
    return Jw.T @ Jw, Jw.T @ rw, cost, int(w.sum()), w, r2


def truncated_cost(R, t, xh, xh2, thr, ok=None):
    ok = usable(xh, xh2) if ok is None else ok
    r = residuals(R, t, xh, xh2)
    with np.errstate(invalid="ignore"):
        r2 = r * r
        return float(np.where(r2 < thr * thr, r2, thr * thr)[ok].sum())


def refine(R0, t0, xa, xb, KA, KB, thr, iters=15, mask=None):
    """One pair, pixels (N,2).  Returns a dict: R, t, mask, cost, count, steps (accepted), costs (the cost after the start and after
    every accepted step), cost0 (of the input pose).  A failure (fewer than 5 weighted matches, a Cholesky pivot that is not
    positive, a pose that is not finite or has t = 0) returns the input pose."""
    with np.errstate(all="ignore"):
        xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    ok = usable(xh, xh2, mask)
    if not (np.isfinite(KA).all() and np.isfinite(KB).all() and np.isfinite(np.linalg.inv(KA)).all() and np.isfinite(np.linalg.inv(KB)).all()):
        ok = np.zeros(len(xa), bool)
    R0, t0 = np.asarray(R0, float), np.asarray(t0, float)
    good = bool(np.isfinite(R0).all() and np.isfinite(t0).all() and (t0 @ t0) > 0)
    with np.errstate(all="ignore"):
        A, g, cost, cnt, w, _ = evaluate(R0, t0, xh, xh2, thr, ok)
    start = dict(R=R0, t=t0, mask=w, cost=cost, count=cnt, steps=0, costs=[cost], cost0=cost)
    if not good or cnt < MIN_MATCHES:
        return start

    def propose(pose, delta):
        Rc, tc = step(*pose, delta)
        return None if np.array_equal(Rc, pose[0]) and np.array_equal(tc, pose[1]) else (Rc, tc)

    def evaluate_pose(pose):                               # one pass: the cost of the candidate and, if it is kept, its equations
        A2, g2, c2, n2, w2, _ = evaluate(*pose, xh, xh2, thr, ok)
        return c2, n2, w2, (A2, g2)

    out = schedule((R0, t0), cost, cnt, w, iters, lambda pose, eqs: eqs, propose, evaluate_pose, (A, g))
    if out is None:
        return start
    (R, t), cost, cnt, w, steps, costs = out
    return dict(R=R, t=t, mask=w, cost=cost, count=cnt, steps=steps, costs=costs, cost0=costs[0])


def calibrated_threshold(max_epipolar_error, camera0, camera1):
    """the threshold of estimate_relative_pose: pixels -> calibrated units by the mean of the two cameras' 1 / focal length"""
    f0 = 0.5 * (camera0["params"][0] + camera0["params"][1])
    f1 = 0.5 * (camera1["params"][0] + camera1["params"][1])
    return max_epipolar_error * 0.5 * (1.0 / f0 + 1.0 / f1)
