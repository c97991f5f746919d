"""What the numpy restatements of the three refinements share (tests/pose_refine_ref.py, fundamental_refine_ref.py,
homography_refine_ref.py): the Levenberg-Marquardt schedule of the kernels' common loop (twoview_math.h: solve_step and the
accept / damp rule), its constants, the damped Cholesky solve and the usable-match rule.  Everything that belongs to one model — the
parameterisation, residuals, Jacobians, normalisation — stays in that model's file and reaches `schedule` as three callbacks."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G

LAMBDA0, LAMBDA_MIN = 1e-3, 1e-10
ACCEPT_REL = 1e-12                 # a step is kept when cost' < cost * (1 - ACCEPT_REL): strictly lower, by more than rounding


def usable(xa, xb, mask=None):
    ok = G.usable(xa, xb)
    return ok if mask is None else ok & np.asarray(mask, bool)


def same_bits(a, b):
    return np.asarray(a, float).tobytes() == np.asarray(b, float).tobytes()


def cholesky_solve(A, lam, g):
    """delta of (A + lam diag A) delta = -g by Cholesky; None on a pivot that is not positive (or not finite)"""
    n = len(g)
    M = A + lam * np.diag(np.diag(A))
    L = np.zeros((n, n))
    for j in range(n):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0.0 or not np.isfinite(p):
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def schedule(state, cost, count, mask, iters, equations, propose, evaluate, extra=None):
    """At most `iters` steps from `state`, whose truncated cost, inlier count and inlier mask are given.
      equations(state, extra) -> (A, g): the normal equations at the state, asked for at the start and after every kept step; `extra`
                                 is what evaluate returned with that state (the pose hands its A, g over this way: one pass gives
                                 that kernel both the cost and the equations; F and H compute them here, for a kept step only)
      propose(state, delta)   -> the candidate state, or None where the step moved no bit (no later one will: the loop ends)
      evaluate(candidate)     -> (cost, count, mask, extra)
    A candidate is kept when its cost is strictly lower (ACCEPT_REL), then lambda /= 10 (not below LAMBDA_MIN); else lambda *= 10.
    Returns (state, cost, count, mask, steps kept, [the cost at the start and after every kept step]), or None where the caller
    returns its input as it came: no step was kept, or a Cholesky pivot was not positive."""
    lam, steps, costs, eqs = LAMBDA0, 0, [cost], None
    for _ in range(iters):
        if eqs is None:
            eqs = equations(state, extra)
        delta = cholesky_solve(eqs[0], lam, eqs[1])
        if delta is None:
            return None
        cand = propose(state, delta)
        if cand is None:
            break
        c2, n2, w2, extra2 = evaluate(cand)
        if c2 < cost * (1.0 - ACCEPT_REL):
            state, cost, count, mask, extra, eqs = cand, c2, n2, w2, extra2, None
            lam = max(lam / 10.0, LAMBDA_MIN)
            steps += 1
            costs.append(cost)
        else:
            lam *= 10.0
    if steps == 0:
        return None
    return state, cost, count, mask, steps, costs
