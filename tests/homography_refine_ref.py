"""numpy fp64 restatement of roma_amd.geometry.refine_homography (csrc/homography_refine.hip): Levenberg-Marquardt on the truncated
forward-transfer cost of a homography, with the kernel's normalisation, gauge, analytic Jacobian, schedule and failure rules.  The
two differ in the order of their sums, in where the compiler fuses a multiply-add and in the last bits of division, nothing else.

Model H^ = T_B H T_A^-1 in Hartley-normalised coordinates, scaled to unit Frobenius norm; eight parameters: the entries of H^ but the
one of largest magnitude (first on ties), which is held and chosen again at every Jacobian pass; a step is H^ <- unit(H^ + delta).
The model in pixels is geometry_ref.finish(T_B^-1 H^ T_A): H[2,2] = 1.  Residual of a pixel match r = (H x_A)_{1,2} / (H x_A)_3 - x_B
(the H branch of geometry_ref.errors is |r|^2 = e); cost = sum of min(e, thr^2) over the usable matches (finite, and allowed by the
optional mask); weight 1 where e < thr^2.  The Jacobian pass runs in normalised coordinates, with the threshold scaled by s_B."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G
from tests.lm_ref import ACCEPT_REL, LAMBDA0, LAMBDA_MIN, cholesky_solve, same_bits, schedule, usable  # noqa: F401  (shared by the three)

MIN_MATCHES = 4
NPAR = 8


def normalised_points(xa, xb, ok):
    """-> (T_A, T_B, x^_A, x^_B, s_B): the transforms of `normalisation` and the points under them, x^ = (x - c) s"""
    cA, cB = G.normalisation(xa, ok), G.normalisation(xb, ok)
    with np.errstate(invalid="ignore"):
        return G.transform(cA), G.transform(cB), (xa - cA[:2]) * cA[2], (xb - cB[:2]) * cB[2], cB[2]


def to_normalised(H, TA, TB):
    """pixels -> H^ of unit Frobenius norm (all zero for a zero H)"""
    return G.unit(TB @ H @ np.linalg.inv(TA))


def pixel_model(Hh, TA, TB):
    """the model as it is returned: H[2,2] = 1 (unit Frobenius norm where |H[2,2]| < 1e-12 |H|)"""
    return G.finish("homography", np.linalg.inv(TB) @ Hh @ TA)


def held_entry(Hh):
    """index (row major) of the entry the gauge holds: the largest magnitude, first on ties"""
    return int(np.abs(Hh).argmax())


def step(Hh, k, delta):
    """H^ + delta on the eight entries other than k, scaled back to unit Frobenius norm"""
    d = np.zeros(9)
    d[np.arange(9) != k] = delta
    return G.unit(Hh + d.reshape(3, 3))


def _hom(x):
    return np.concatenate([x, np.ones_like(x[:, :1])], -1)


def residuals(H, xa, xb):
    """r (N,2) of the model H, in the coordinates of the points; NaN or inf where the match or the projection is not finite"""
    with np.errstate(all="ignore"):
        hx = _hom(xa) @ np.asarray(H, float).T
        return hx[:, :2] / hx[:, 2:3] - xb


def residuals_and_jacobian(Hh, xa, xb):
    """r (N,2) and dr/dh^ (N,2,9) by all nine entries, in the coordinates of the points (the caller drops the held column):
    dx'/dh^ = (x, y, 1, 0, 0, 0, -x' x, -x' y, -x') / w, dy'/dh^ = (0, 0, 0, x, y, 1, -y' x, -y' y, -y') / w"""
    with np.errstate(all="ignore"):
        ha = _hom(xa)
        hx = ha @ np.asarray(Hh, float).T
        a = ha / hx[:, 2:3]
        p = hx[:, :2] / hx[:, 2:3]
        z = np.zeros_like(a)
        J = np.stack([np.concatenate([a, z, -p[:, :1] * a], -1), np.concatenate([z, a, -p[:, 1:] * a], -1)], 1)
    return p - xb, J


def cost_of(H, xa, xb, thr, ok):
    """-> (truncated cost, inlier count, inlier mask, e) of the pixel-space model H over the usable matches `ok`"""
    t2 = thr * thr
    with np.errstate(all="ignore"):
        e = (residuals(H, xa, xb) ** 2).sum(-1)
        w = ok & (e < t2)
    return float(np.where(w, e, t2)[ok].sum()), int(w.sum()), w, e


def truncated_cost(H, xa, xb, thr, mask=None):
    return cost_of(H, xa, xb, thr, usable(xa, xb, mask))[0]


def normal_equations(Hh, k, xah, xbh, thr_h, ok):
    """J^T J (8,8) and J^T r (8,) over the weighted matches, in normalised coordinates, the held column k dropped"""
    r, J = residuals_and_jacobian(Hh, xah, xbh)
    with np.errstate(invalid="ignore"):
        w = ok & ((r ** 2).sum(-1) < thr_h * thr_h)
    Jw, rw = J[w][:, :, np.arange(9) != k].reshape(-1, NPAR), r[w].reshape(-1)
    return Jw.T @ Jw, Jw.T @ rw


def refine(H0, xa, xb, thr, iters=15, mask=None):
    """One pair, pixels (N,2).  Returns a dict: H, mask, cost, count, steps (kept), costs (the cost of the input and after every kept
    step), cost0 (of the input as given).  Without a kept step — and with fewer than 4 weighted matches, a Cholesky pivot that is not
    positive, an input that is not finite or is all zero — the input is returned as it came."""
    H0 = np.asarray(H0, float)
    ok = usable(xa, xb, mask)
    cost, cnt, w, _ = cost_of(H0, xa, xb, thr, ok)
    start = dict(H=H0, mask=w, cost=cost, count=cnt, steps=0, costs=[cost], cost0=cost)
    if not np.isfinite(H0).all() or cnt < MIN_MATCHES:
        return start
    TA, TB, xah, xbh, sB = normalised_points(xa, xb, ok)
    with np.errstate(all="ignore"):
        Hh = to_normalised(H0, TA, TB)
    if not np.isfinite(Hh).all() or not Hh.any():
        return start
    thr_h = thr * sB

    def propose(state, delta):
        Hh, _, k = state
        d = np.zeros(9)
        d[np.arange(9) != k] = delta
        if same_bits(Hh + d.reshape(3, 3), Hh):
            return None
        Hc = step(Hh, k, delta)
        with np.errstate(all="ignore"):
            return Hc, pixel_model(Hc, TA, TB), held_entry(Hc)

    # a state: (H^, the model in pixels, the entry of H^ that its equations hold)
    out = schedule((Hh, H0, held_entry(Hh)), cost, cnt, w, iters, lambda state, _: normal_equations(state[0], state[2], xah, xbh, thr_h, ok),
                   propose, lambda state: (*cost_of(state[1], xa, xb, thr, ok)[:3], None))
    if out is None:
        return start
    (_, H, _), cost, cnt, w, steps, costs = out
    return dict(H=H, mask=w, cost=cost, count=cnt, steps=steps, costs=costs, cost0=costs[0])


def corner_error_hpatches(H, H_gt, w, h, scale=1.0):
    """the reference's HPatches metric (hpatches_sequences_homog_benchmark.py:92-103): the mean distance of the four warped corners of
    image A, over `scale` (the benchmark passes min(w2, h2) / 480)"""
    corners = np.array([[0, 0, 1], [0, h - 1, 1], [w - 1, 0, 1], [w - 1, h - 1, 1]], dtype=np.float64)
    with np.errstate(all="ignore"):
        real = corners @ np.asarray(H_gt, float).T
        real = real[:, :2] / real[:, 2:]
        warped = corners @ np.asarray(H, float).T
        warped = warped[:, :2] / warped[:, 2:]
        return float(np.mean(np.linalg.norm(real - warped, axis=1)) / scale)
