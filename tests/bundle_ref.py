"""numpy restatement of roma_amd.geometry.bundle_adjust (csrc/bundle.hip), fp64.  It builds and solves the FULL damped normal equations
over the free points and the free views — no Schur complement, so it shares no algebra with the kernels — and takes the Levenberg-
Marquardt schedule, its constants and the Cholesky solve from tests/lm_ref.py.  `schur_step` is the other thing in here: steps 1 to 4 of
the kernels (per-point elimination, the reduced camera system, back substitution) stated in numpy, which a test holds against the full
solve.

Definition (x_v ~ K_v (R_v X + t_v), everything relative to c0 = the mean of the centres of the usable views in view order):
  observed (v, n)  x[v, n] finite, visible[v, n] set, view v usable (K upper triangular, fx fy != 0, K R t finite), X[n] finite
  weighted         observed, depth > 0, squared pixel error e < thr^2;  cost = sum over observed (weighted ? e : thr^2)
  parameters       a free view: R' = orthonormalise(exp([w]x) R), t' = exp([w]x) t + tau; a point: X' = X + d
  held             the views of `fixed`, unusable views, a free view without a weighted observation; a point with fewer than two
                   weighted observations.  (The kernels also hold a point whose damped 3 x 3 block has a pivot that is not positive;
                   here such a pivot is one of the full Cholesky and returns the input.  With two weighted observations at positive
                   depth and fx fy != 0 the block is positive definite, so finite inputs never get there.)
  unknowns         the free points in ascending order, 3 each, then the free views, 6 each: eliminating the points first makes the
                   remaining pivots those of the reduced camera system
The caller's R, t, X come back bit for bit when no step is kept or a pivot fails; a view or point held at every kept step does too."""
from __future__ import annotations

import numpy as np

from tests import lm_ref as LM
from tests.pose_refine_ref import exp_so3, orthonormalise

PERTURB_ROT_DEG, PERTURB_T, PERTURB_DEPTH = 0.1, 0.01, 0.005


def perturbed_start(s, seed, fixed=(0, 1), scale=1.0):
    """the start of the tests: every view outside `fixed` turned by PERTURB_ROT_DEG about each axis (random signs) and moved by PERTURB_T in a random direction, every
    point moved along its ray from the centre of view 0 by PERTURB_DEPTH (normal) of its depth -> R, t, X"""
    rng = np.random.default_rng([seed, 31])
    V = len(s["R"])
    R, t = s["R"].copy(), s["t"].copy()
    for v in range(V):
        w, d = rng.normal(size=3), rng.normal(size=3)
        if v not in fixed:
            R[v] = exp_so3(scale * np.radians(PERTURB_ROT_DEG) * np.sign(w)) @ R[v]
            t[v] = t[v] + scale * PERTURB_T * d / np.linalg.norm(d)
    C0 = -s["R"][0].T @ s["t"][0]
    X = C0 + (1.0 + scale * PERTURB_DEPTH * rng.normal(size=(len(s["X"]), 1))) * (s["X"] - C0)
    return R, t, X


def usable_views(K, R, t):
    ok = np.isfinite(K).all((1, 2)) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    ok &= (K[:, 1, 0] == 0) & (K[:, 2, 0] == 0) & (K[:, 2, 1] == 0)
    with np.errstate(all="ignore"):
        d = K[:, 0, 0] * K[:, 1, 1]
        ok &= (d != 0) & np.isfinite(1.0 / d)
    return ok


def terms(K, R, t, X, x):
    """e (V,N), depth (V,N), r (V,N,2), Jc (V,N,2,6) by (w, tau), Jp (V,N,2,3) by X"""
    with np.errstate(all="ignore"):
        q = np.einsum("vij,nj->vni", R, X) + t[:, None, :]
        z = q[..., 2]
        iz = 1.0 / z
        a, b = q[..., 0] * iz, q[..., 1] * iz
        fx, sk, cx, fy, cy = (K[:, i, j, None] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)))
        r = np.stack([fx * a + sk * b + cx - x[..., 0], fy * b + cy - x[..., 1]], -1)
        e = (r * r).sum(-1)
        zero = np.zeros_like(z)
        Jq = np.stack([np.stack([fx * iz, sk * iz, -(fx * a + sk * b) * iz], -1), np.stack([zero, fy * iz, -(fy * b) * iz], -1)], -2)
        D = np.stack([np.stack([zero, q[..., 2], -q[..., 1]], -1), np.stack([-q[..., 2], zero, q[..., 0]], -1),
                      np.stack([q[..., 1], -q[..., 0], zero], -1)], -2)                      # d q / d w = -[q]x
        Jc = np.concatenate([np.einsum("vndk,vnkj->vndj", Jq, D), Jq], -1)
        Jp = np.einsum("vndk,vkj->vndj", Jq, R)
    return e, z, r, Jc, Jp


class Problem:
    """the constants of one call: observations in fp64, the observed pattern, the free views, the order of the sums"""

    def __init__(self, x, K, R, t, X, visible, fixed, thr, order):
        V, N = x.shape[:2]
        self.V, self.N, self.t2 = V, N, float(thr) * float(thr)
        self.x = np.asarray(x, np.float32).astype(np.float64)
        self.K = np.broadcast_to(np.asarray(K, float), (V, 3, 3)) if np.ndim(K) == 2 else np.asarray(K, float)
        self.ok = usable_views(self.K, R, t)
        self.free = self.ok.copy()
        self.free[list(fixed)] = False
        seen = np.isfinite(self.x).all(-1) if visible is None else np.isfinite(self.x).all(-1) & np.asarray(visible, bool)
        self.observed = seen & self.ok[:, None] & np.isfinite(X).all(-1)[None, :]
        self.sel = (np.arange(N), np.arange(N)[::-1], np.random.default_rng(1).permutation(N))[order]
        C = -np.einsum("vji,vj->vi", np.where(self.ok[:, None, None], R, 0.0), np.where(self.ok[:, None], t, 0.0))
        self.c0 = np.zeros(3)
        for v in range(V):
            if self.ok[v]:
                self.c0 = self.c0 + C[v]
        if self.ok.any():
            self.c0 = self.c0 / int(self.ok.sum())

    def evaluate(self, st):
        """-> (cost, count, weighted (V,N), the terms)"""
        R, t, X = st[:3]
        T = terms(self.K, R, t, X, self.x)
        with np.errstate(invalid="ignore"):
            w = self.observed & (T[1] > 0.0) & (T[0] < self.t2)
        per = np.where(self.observed, np.where(w, T[0], self.t2), 0.0)
        cost = float(per.sum(0)[self.sel].sum())
        return cost, int(w.sum()), w, (w, T)

    def structure(self, w):
        """the views and points that take part in a step under the weighted pattern w"""
        return self.free & w.any(1), w.sum(0) >= 2

    def equations(self, st, extra):
        w, (_, _, r, Jc, Jp) = extra
        act, pfree = self.structure(w)
        npf = int(pfree.sum())
        pcol = np.cumsum(pfree) - 1
        vcol = np.cumsum(act) - 1
        ns, vs = np.nonzero(w.T[self.sel])                            # the observations, point by point in the order of the sums
        ns = self.sel[ns]
        npar = 3 * npf + 6 * int(act.sum())
        J = np.concatenate([Jp[vs, ns], Jc[vs, ns]], -1)             # (m,2,9): the point's three columns, then the view's six
        col = np.concatenate([np.where(pfree[ns, None], 3 * pcol[ns, None] + np.arange(3), npar),
                              np.where(act[vs, None], 3 * npf + 6 * vcol[vs, None] + np.arange(6), npar)], -1)
        H = np.einsum("kdi,kdj->kij", J, J)
        A, g = np.zeros((npar + 1, npar + 1)), np.zeros(npar + 1)    # the last row and column take what belongs to held unknowns
        np.add.at(A, (col[:, :, None], col[:, None, :]), H)          # unbuffered: one observation after the other, no BLAS
        np.add.at(g, col, np.einsum("kdi,kd->ki", J, r[vs, ns]))
        return A[:npar, :npar], g[:npar]

    def propose(self, st, delta):
        R, t, X, mv, mp = st
        w = self.evaluate(st)[2]
        act, pfree = self.structure(w)
        npf = int(pfree.sum())
        X2 = X.copy()
        X2[pfree] = X[pfree] + delta[:3 * npf].reshape(-1, 3)
        R2, t2 = R.copy(), t.copy()
        for i, v in enumerate(np.nonzero(act)[0]):
            d = delta[3 * npf + 6 * i: 3 * npf + 6 * i + 6]
            E = exp_so3(d[:3])
            R2[v], t2[v] = orthonormalise(E @ R[v]), E @ t[v] + d[3:]
        return R2, t2, X2, mv | act, mp | pfree


def refine(x, K, R0, t0, X0, thr=2.0, iters=10, fixed=(0,), visible=None, order=0):
    """-> dict: R, t, X, mask (V,N) bool, cost, cost0, count, steps.  order = 1 sums the points in reverse and order = 2 in a shuffled
    order (what the order of the sums is worth)."""
    R0, t0, X0 = np.asarray(R0, float), np.asarray(t0, float), np.asarray(X0, float)
    P = Problem(x, K, R0, t0, X0, visible, fixed, thr, order)
    with np.errstate(all="ignore"):
        st0 = (R0, t0 + np.einsum("vij,j->vi", R0, P.c0), X0 - P.c0, np.zeros(P.V, bool), np.zeros(P.N, bool))
        cost, cnt, w, extra = P.evaluate(st0)
    start = dict(R=R0, t=t0, X=X0, mask=w, cost=cost, cost0=cost, count=cnt, steps=0)
    if iters == 0 or not P.free.any() or not np.isfinite(cost):
        return start

    def evaluate(st):
        c, n, w2, ex = P.evaluate(st)
        return c, n, w2, ex

    out = LM.schedule(st0, cost, cnt, w, iters, P.equations, P.propose, evaluate, extra)
    if out is None:
        return start
    (R, t, X, mv, mp), cost1, cnt, w, steps, _ = out
    t = np.where(mv[:, None], t - np.einsum("vij,j->vi", R, P.c0), t0)
    R = np.where(mv[:, None, None], R, R0)
    X = np.where(mp[:, None], X + P.c0, X0)
    return dict(R=R, t=t, X=X, mask=w, cost=cost1, cost0=cost, count=cnt, steps=steps)


def schur_step(x, K, R, t, X, thr, fixed, lam, visible=None):
    """One step the way the kernels take it, from the state as given (no centring): per point the damped V*^-1, the reduced system
    S dc = b over the free views, dp = V*^-1 (-g_p - sum_v W_vn^T dc_v).  -> (dc (views that take part, 6), dp (free points, 3), and
    the same two from lm_ref.cholesky_solve on the full equations)"""
    P = Problem(x, K, R, t, X, visible, fixed, thr, 0)
    st = (np.asarray(R, float), np.asarray(t, float), np.asarray(X, float), None, None)
    _, _, w, extra = P.evaluate(st)
    _, _, r, Jc, Jp = extra[1]
    act, pfree = P.structure(w)
    views, nv = np.nonzero(act)[0], int(act.sum())
    S, b = np.zeros((6 * nv, 6 * nv)), np.zeros(6 * nv)
    for i, v in enumerate(views):
        for n in np.nonzero(w[v])[0]:
            S[6 * i:6 * i + 6, 6 * i:6 * i + 6] += Jc[v, n].T @ Jc[v, n]
            b[6 * i:6 * i + 6] -= Jc[v, n].T @ r[v, n]
    S = S + lam * np.diag(np.diag(S))
    Vinv, gp = {}, {}
    for n in np.nonzero(pfree)[0]:
        vs = np.nonzero(w[:, n])[0]
        Vn = sum(Jp[v, n].T @ Jp[v, n] for v in vs)
        Vinv[n] = np.linalg.inv(Vn + lam * np.diag(np.diag(Vn)))
        gp[n] = sum(Jp[v, n].T @ r[v, n] for v in vs)
        W = {i: Jc[v, n].T @ Jp[v, n] for i, v in enumerate(views) if w[v, n]}
        for i, Wi in W.items():
            b[6 * i:6 * i + 6] += Wi @ Vinv[n] @ gp[n]
            for j, Wj in W.items():
                S[6 * i:6 * i + 6, 6 * j:6 * j + 6] -= Wi @ Vinv[n] @ Wj.T
    dc = np.linalg.solve(S, b)
    dp = []
    for n in np.nonzero(pfree)[0]:
        rhs = -gp[n]
        for i, v in enumerate(views):
            if w[v, n]:
                rhs = rhs - (Jc[v, n].T @ Jp[v, n]).T @ dc[6 * i:6 * i + 6]
        dp.append(Vinv[n] @ rhs)
    dp = np.array(dp).reshape(-1, 3)
    A, g = P.equations(st, extra)
    full = LM.cholesky_solve(A, lam, g)
    npf = int(pfree.sum())
    return dc.reshape(-1, 6), dp, full[3 * npf:].reshape(-1, 6), full[:3 * npf].reshape(-1, 3)


def rotation_error_deg(R, R_true):
    return float(np.degrees(np.arccos(np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1))))


def worst_errors(R, t, R_true, t_true):
    """the worst rotation error in degrees and the worst camera-centre error over the views, in the frame both share"""
    er = max(rotation_error_deg(a, b) for a, b in zip(R, R_true))
    C, Ct = -np.einsum("vji,vj->vi", R, t), -np.einsum("vji,vj->vi", R_true, t_true)
    return er, float(np.linalg.norm(C - Ct, axis=1).max())
