"""numpy fp64 restatement of roma_amd.geometry.find_absolute_pose / refine_absolute_pose (csrc/absolute_pose.hip), no torch: the sample
draw bit for bit (stage 5), the normalisation of the world points, the P3P solver with its rejection rules and its polish, the
reprojection error, the RANSAC with its local optimisation and the Levenberg-Marquardt refinement.  Plus the scenes the tests use.

Convention: x ~ K (R X + t), X in any world frame, x in pixels, K upper triangular with last row 0 0 1.

P3P (the kernel's steps, statement for statement where a branch is taken):
  bearings f_i = (K^-1 x_i, 1) / |.|, c_ij = f_i . f_j, a_ij = |X_i - X_j|^2; the depths d satisfy d^T M_ij d = a_ij.
  D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23 are two homogeneous conics in d.  det(alpha D1 + beta D2) is a cubic; the side with
  the larger leading coefficient is made monic (gamma = beta / alpha, or mu = alpha / beta), one real root is taken in closed form
  (of three, the one with the largest |derivative|) and polished by two Newton steps.  The degenerate conic D0 is split into its
  two lines: B = -adj D0 = p p^T, p from the column of the largest diagonal entry, D0 + [p]x = 2 m l^T.  On each line the other conic
  is a quadratic in one depth ratio; each real root with three positive depths is scaled by d^T (M12 + M13 + M23) d = a12 + a13 + a23.
  (R, t) from the three camera points d_i f_i, R made orthonormal, then POLISH undamped Gauss-Newton steps on the six reprojection
  equations of the sample in calibrated coordinates.  Slots: line l before line m, on a line the root -sqrt before +sqrt."""
from __future__ import annotations

import numpy as np

from tests import general_scenes as GS
from tests import geometry_ref as G
from tests.lm_ref import ACCEPT_REL, LAMBDA0, LAMBDA_MIN, cholesky_solve, schedule  # noqa: F401
from tests.pose_refine_ref import exp_so3, orthonormalise

M32 = 0xFFFFFFFF
STAGE = 5
SLOTS = 4
POLISH = 2
COLLINEAR_TOL = 1e-6
MIN_MATCHES = 4
T_SCALE = 1.5
OFFSET = np.array([1e4, -2e4, 5e3])


# ------------------------------------------------------------------------------------------------------------------- scenes
def scene(motion, seed, N=2000, outlier_frac=0.3, sigma=0.5):
    """-> X (N,3) world points (camera A's frame), x (N,2) pixels of image B, is_inlier (N,), R, t (|t| = 1.5).  Inliers:
    backproject(u, d, K_A), u uniform over image A, depths 4-12, kept if in front of B and inside image B; outliers: world points of
    the same distribution paired with pixels uniform over image B; sigma on the pixels; permuted."""
    rng = np.random.default_rng([seed, 5])
    R, t = GS.scene_pose(motion, seed)
    t = T_SCALE * t
    n_in = int(round(N * (1 - outlier_frac)))
    Xs, xs = [], []
    while sum(len(a) for a in Xs) < n_in:
        u = GS._uniform(rng, GS.W_A, GS.H_A, 4 * n_in)
        Xw = GS.backproject(u, rng.uniform(4, 12, 4 * n_in), GS.K_A)
        Xb = Xw @ R.T + t
        ub = GS.project(Xb, GS.K_B)
        keep = (Xb[:, 2] > 0.5) & (ub[:, 0] >= 0) & (ub[:, 0] < GS.W_B) & (ub[:, 1] >= 0) & (ub[:, 1] < GS.H_B)
        Xs.append(Xw[keep])
        xs.append(ub[keep])
    Xi, xi = np.concatenate(Xs)[:n_in], np.concatenate(xs)[:n_in]
    n_out = N - n_in
    Xo = GS.backproject(GS._uniform(rng, GS.W_A, GS.H_A, n_out), rng.uniform(4, 12, n_out), GS.K_A)
    xo = GS._uniform(rng, GS.W_B, GS.H_B, n_out)
    X = np.concatenate([Xi, Xo])
    x = np.concatenate([xi + rng.normal(0, sigma, xi.shape), xo])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(N)
    return X[perm], x[perm], truth[perm], R, t


def rotation_error_deg(R, R_true):
    return float(np.degrees(np.arccos(np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1))))


def centre_error(R, t, R_true, t_true):
    return float(np.linalg.norm(-R.T @ t + R_true.T @ t_true))


# ----------------------------------------------------------------------------------------------------------------- the draw
def usable(X, x):
    return np.isfinite(X).all(-1) & np.isfinite(x).all(-1)


def minimal_samples(X, x, iters, seed, p0=0):
    """(P,N,3), (P,N,2) -> (P, iters, 3) int32, rows of -1 for invalid samples: the draw of geometry.hip's header with stage 5"""
    P, N = X.shape[0], X.shape[1]
    ok_pt = usable(X, x)
    stream = int(G.fmix32((int(seed) & M32) ^ ((STAGE * 0x9E3779B9) & M32)))
    p = np.arange(p0, p0 + P, dtype=np.uint64)[:, None]
    h = np.arange(iters, dtype=np.uint64)[None, :]
    idx = np.full((P, iters, 3), -1, dtype=np.int64)
    for k in range(3):
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
    idx[(idx < 0).any(-1)] = -1
    return idx.astype(np.int32)


def normalisation(X, ok):
    """centroid c and scale s of the usable world points: X' = s (X - c) has mean distance sqrt 3 from the origin"""
    if not ok.any():
        return np.zeros(3), 1.0
    c = X[ok].mean(0)
    md = np.sqrt(((X[ok] - c) ** 2).sum(-1)).mean()
    s = np.sqrt(3.0) / md if md > 0 else 1.0
    return c, (float(s) if np.isfinite(s) else 1.0)


def calibrate(x, K):
    h = np.concatenate([x, np.ones_like(x[..., :1])], -1) @ np.linalg.inv(K).T
    return h[..., :2]


# ---------------------------------------------------------------------------------------------------------------------- P3P
def real_root(A, B, C):
    """one real root of x^3 + A x^2 + B x + C: closed form, of three the one with the largest |derivative|, two Newton steps"""
    p = B - A * A / 3.0
    q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + C
    disc = q * q / 4.0 + p * p * p / 27.0
    if disc > 0.0:
        sq = np.sqrt(disc)
        u = np.cbrt(-q / 2.0 - (sq if q >= 0 else -sq))
        y = u - p / (3.0 * u) if u != 0.0 else 0.0
        x = y - A / 3.0
    else:
        r = 2.0 * np.sqrt(max(-p / 3.0, 0.0))
        cphi = np.clip(3.0 * q / (p * r), -1.0, 1.0) if p * r != 0.0 else 0.0
        phi = np.arccos(cphi)
        x, best = 0.0, -1.0
        for k in range(3):
            xk = r * np.cos((phi - 2.0 * np.pi * k) / 3.0) - A / 3.0
            d = abs((3.0 * xk + 2.0 * A) * xk + B)
            if d > best:
                x, best = xk, d
    for _ in range(2):
        f = ((x + A) * x + B) * x + C
        df = (3.0 * x + 2.0 * A) * x + B
        if df != 0.0:
            x = x - f / df
    return x


def pose_from_points(Xs, Y):
    """(R, t) with Y_i = R X_i + t from three points: the frames (e1, e2, e1 x e2) of both triangles"""
    A = np.stack([Xs[1] - Xs[0], Xs[2] - Xs[0], np.cross(Xs[1] - Xs[0], Xs[2] - Xs[0])], -1)
    Bm = np.stack([Y[1] - Y[0], Y[2] - Y[0], np.cross(Y[1] - Y[0], Y[2] - Y[0])], -1)
    R = orthonormalise(Bm @ np.linalg.inv(A))
    return R, Y[0] - R @ Xs[0]


def point_terms(R, t, X, x, K):
    """error e (N,), depth z (N,), residual r (N,2) and Jacobian J (N,2,6) by (w, dt): R <- exp([w]x) R, t <- t + dt"""
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    with np.errstate(all="ignore"):
        Q = X @ R.T
        Y = Q + t
        z = Y[:, 2]
        iz = 1.0 / z
        a, b = Y[:, 0] * iz, Y[:, 1] * iz
        r = np.stack([fx * a + sk * b + cx - x[:, 0], fy * b + cy - x[:, 1]], -1)
        e = (r * r).sum(-1)
        zero = np.zeros_like(z)
        dY = np.stack([np.stack([zero, Q[:, 2], -Q[:, 1]], -1), np.stack([-Q[:, 2], zero, Q[:, 0]], -1),
                       np.stack([Q[:, 1], -Q[:, 0], zero], -1)], 1)                            # (N, row of Y, w)
        dY = np.concatenate([dY, np.broadcast_to(np.eye(3), (len(X), 3, 3))], -1)               # (N,3,6)
        da = (dY[:, 0] - a[:, None] * dY[:, 2]) * iz[:, None]
        db = (dY[:, 1] - b[:, None] * dY[:, 2]) * iz[:, None]
        J = np.stack([fx * da + sk * db, fy * db], 1)
    return e, z, r, J


def apply_step(R, t, delta):
    return orthonormalise(exp_so3(delta[:3]) @ R), t + delta[3:]


def polish(R, t, Xs, bs):
    I = np.eye(3)
    for _ in range(POLISH):
        _, _, r, J = point_terms(R, t, Xs, bs, I)
        Jm, rm = J.reshape(6, 6), r.reshape(6)
        d = cholesky_solve(Jm.T @ Jm, 0.0, Jm.T @ rm)
        if d is None or not np.isfinite(d).all():
            break
        R, t = apply_step(R, t, d)
    return R, t


def p3p(Xs, bs):
    """Xs (3,3) world points, bs (3,2) calibrated image points -> list of up to 4 (R, t), [] for a rejected sample"""
    e1, e2 = Xs[1] - Xs[0], Xs[2] - Xs[0]
    n1, n2 = np.sqrt(e1 @ e1), np.sqrt(e2 @ e2)
    cr = np.cross(e1, e2)
    if not np.sqrt(cr @ cr) > COLLINEAR_TOL * n1 * n2:
        return []
    f = np.concatenate([bs, np.ones((3, 1))], -1)
    f = f / np.sqrt((f * f).sum(-1))[:, None]
    c12, c13, c23 = f[0] @ f[1], f[0] @ f[2], f[1] @ f[2]
    a12, a13, a23 = e1 @ e1, e2 @ e2, (Xs[2] - Xs[1]) @ (Xs[2] - Xs[1])
    D1 = np.array([[a23, -a23 * c12, 0.0], [-a23 * c12, a23 - a12, a12 * c23], [0.0, a12 * c23, -a12]])
    D2 = np.array([[a23, 0.0, -a23 * c13], [0.0, -a13, a13 * c23], [-a23 * c13, a13 * c23, a23 - a13]])
    det = np.linalg.det
    k0, k3 = det(D1), det(D2)
    k1 = sum(det(np.where(np.arange(3)[:, None] == i, D2, D1)) for i in range(3))
    k2 = sum(det(np.where(np.arange(3)[:, None] == i, D1, D2)) for i in range(3))
    kmax = max(abs(k0), abs(k1), abs(k2), abs(k3))
    side = abs(k3) >= abs(k0)
    lead = k3 if side else k0
    if not abs(lead) > 1e-12 * kmax:
        return []
    if side:
        g = real_root(k2 / k3, k1 / k3, k0 / k3)
        D0, Q = D1 + g * D2, D2
    else:
        g = real_root(k1 / k0, k2 / k0, k3 / k0)
        D0, Q = g * D1 + D2, D1
    cof = np.array([[D0[1, 1] * D0[2, 2] - D0[1, 2] * D0[2, 1], D0[1, 2] * D0[2, 0] - D0[1, 0] * D0[2, 2], D0[1, 0] * D0[2, 1] - D0[1, 1] * D0[2, 0]],
                    [0.0, D0[0, 0] * D0[2, 2] - D0[0, 2] * D0[2, 0], D0[0, 1] * D0[2, 0] - D0[0, 0] * D0[2, 1]],
                    [0.0, 0.0, D0[0, 0] * D0[1, 1] - D0[0, 1] * D0[1, 0]]])
    Bm = -(cof + cof.T - np.diag(np.diag(cof)))
    i = int(np.argmax(np.diag(Bm)))
    if not Bm[i, i] > 0.0:
        return []
    p = Bm[:, i] / np.sqrt(Bm[i, i])
    Nm = D0 + G.skew(p)
    ij = int(np.argmax(np.abs(Nm)))
    lines = (Nm[ij // 3, :], Nm[:, ij % 3])
    asum = a12 + a13 + a23
    Ms = np.array([[2.0, -c12, -c13], [-c12, 2.0, -c23], [-c13, -c23, 2.0]])
    out = []
    for L in lines:
        k = int(np.argmax(np.abs(L)))
        if not abs(L[k]) > 0.0:
            continue
        i, j = [v for v in range(3) if v != k]
        u, w = np.zeros(3), np.zeros(3)
        u[i], u[k] = 1.0, -L[i] / L[k]
        w[j], w[k] = 1.0, -L[j] / L[k]
        qa, qb, qc = u @ Q @ u, 2.0 * (u @ Q @ w), w @ Q @ w
        disc = qb * qb - 4.0 * qa * qc
        if not disc >= 0.0:
            continue
        sq = np.sqrt(disc)
        for sgn in (-1.0, 1.0):
            with np.errstate(all="ignore"):
                al = (-qb + sgn * sq) / (2.0 * qa)
                d = al * u + w
                sc = np.sqrt(asum / (d @ Ms @ d))
                d = d * sc
            if not (np.isfinite(d).all() and (d > 0.0).all()):
                continue
            R, t = pose_from_points(Xs, d[:, None] * f)
            R, t = polish(R, t, Xs, bs)
            z = (Xs @ R.T + t)[:, 2]
            if np.isfinite(R).all() and np.isfinite(t).all() and (z > 0.0).all():
                out.append((R, t))
    return out[:SLOTS]


# ------------------------------------------------------------------------------------------------------------------ scoring
def errors(R, t, X, x, K):
    """squared reprojection error in pixels (inf behind the camera, NaN for a row that is not finite)"""
    with np.errstate(all="ignore"):
        Y = X @ R.T + t
        u = Y @ K.T
        e = ((u[:, :2] / u[:, 2:3] - x) ** 2).sum(-1)
        return np.where(Y[:, 2] > 0.0, e, np.where(np.isnan(e), np.nan, np.inf))


def cost_of(e, t2, scoring="msac"):
    from tests import magsac_ref as MR
    return float(MR.cost(e, t2, scoring))


def evaluate(R, t, X, x, K, thr, ok, weights=None):
    """-> (A (6,6), g (6,), truncated cost, count, mask) over the usable matches in front of the camera"""
    e, z, r, J = point_terms(R, t, X, x, K)
    t2 = thr * thr
    with np.errstate(invalid="ignore"):
        front = ok & (z > 0.0)
        w = front & (e < t2)
    cost = float(np.where(w, e, t2)[front].sum())
    wt = np.ones(int(w.sum())) if weights is None else weights(e[w], t2)
    Jw, rw = J[w].reshape(-1, 6), r[w].reshape(-1)
    ww = np.repeat(wt, 2)
    Jww = Jw * ww[:, None]                                   # plain sums, no BLAS: the order of the sums is numpy's pairwise one
    return (Jww[:, :, None] * Jw[:, None, :]).sum(0), (Jww * rw[:, None]).sum(0), cost, int(w.sum()), w


def refine(R0, t0, X, x, K, thr, iters=15, mask=None, order=0):
    """Levenberg-Marquardt on sum min(e, thr^2) in the normalised world frame X' = s (X - c), as the kernel.  order = 1 sums the matches
    in reverse and order = 2 in a shuffled order (the tests' measure of what the order of the sums is worth).  Returns a dict: R, t, mask, cost, count, steps, cost0."""
    R0, t0 = np.asarray(R0, float), np.asarray(t0, float)
    ok = usable(X, x) if mask is None else usable(X, x) & np.asarray(mask, bool)
    if not np.isfinite(np.linalg.inv(K)).all():
        ok = np.zeros(len(X), bool)
    sel = (np.arange(len(X)), np.arange(len(X))[::-1], np.random.default_rng(1).permutation(len(X)))[order]
    c, s = normalisation(X, ok)
    Xn, xs, oks = ((X - c) * s)[sel], x[sel], ok[sel]
    with np.errstate(all="ignore"):
        tn = s * (R0 @ c + t0)
        A, g, cost, cnt, w = evaluate(R0, tn, Xn, xs, K, thr, oks)
    back = np.argsort(sel)
    start = dict(R=R0, t=t0, mask=w[back], cost=cost, count=cnt, steps=0, cost0=cost)
    if not (np.isfinite(R0).all() and np.isfinite(t0).all()) or cnt < MIN_MATCHES:
        return start

    def propose(pose, delta):
        Rc, tc = apply_step(*pose, delta)
        return None if np.array_equal(Rc, pose[0]) and np.array_equal(tc, pose[1]) else (Rc, tc)

    def evaluate_pose(pose):
        A2, g2, c2, n2, w2 = evaluate(*pose, Xn, xs, K, thr, oks)
        return c2, n2, w2, (A2, g2)

    out = schedule((R0, tn), cost, cnt, w, iters, lambda pose, eqs: eqs, propose, evaluate_pose, (A, g))
    if out is None:
        return start
    (R, tn), cost, cnt, w, steps, _ = out
    return dict(R=R, t=tn / s - R @ c, mask=w[back], cost=cost, count=cnt, steps=steps, cost0=start["cost"])


def hypotheses(X, x, K, iters, seed, p0=0):
    """one pair -> (samples (iters,3), [list of (R, t) in the WORLD frame per sample])"""
    idx = minimal_samples(X[None], x[None], iters, seed, p0)[0]
    ok = usable(X, x)
    c, s = normalisation(X, ok)
    Xn, b = (X - c) * s, calibrate(x, K)
    out = []
    for h in range(iters):
        sols = p3p(Xn[idx[h]], b[idx[h]]) if idx[h, 0] >= 0 else []
        out.append([(R, t / s - R @ c) for R, t in sols])
    return idx, out


def ransac(X, x, K, thr, iters, seed, lo_iters=3, scoring="msac"):
    """-> (R, t, mask), zeros and an empty mask when no sample gives a model"""
    t2 = thr * thr
    ok = usable(X, x)
    c, s = normalisation(X, ok)
    Xn = (X - c) * s
    _, hyp = hypotheses(X, x, K, iters, seed)
    best, bc = None, np.inf
    for sols in hyp:
        for R, t in sols:
            cst = cost_of(errors(R, t, X, x, K), t2, scoring)
            if cst < bc:
                best, bc = (R, s * (R @ c + t)), cst
    if best is None:
        return np.zeros((3, 3)), np.zeros(3), np.zeros(len(X), bool)
    weights = None
    if scoring == "magsac":
        from tests import magsac_ref as MR
        weights = MR.weight
    R, tn = best
    for _ in range(lo_iters):
        A, g, _, cnt, _ = evaluate(R, tn, Xn, x, K, thr, ok, weights)
        if cnt < MIN_MATCHES:
            break
        d = cholesky_solve(A, LAMBDA0, g)
        if d is None:
            break
        Rc, tc = apply_step(R, tn, d)
        c2 = cost_of(errors(Rc, tc, Xn, x, K), t2, scoring)
        if not c2 < bc:
            break
        R, tn, bc = Rc, tc, c2
    with np.errstate(invalid="ignore"):
        mask = errors(R, tn, Xn, x, K) < t2
    return R, tn / s - R @ c, mask


def truth_aware_fit(X, x, truth, K, R_true, t_true, thr=1e3):
    """LM on the true inliers from the true pose: what the data supports"""
    r = refine(R_true, t_true, X, x, K, thr, iters=30, mask=truth)
    return r["R"], r["t"]


# ----------------------------------------------------------------------------------------------------- three views, depth maps
BASELINE = 0.8                 # |t| of view B in the three-view scene: triangulated points come out in units of it


def three_view_scene(motion_ab, motion_ac, seed, N=2000, outlier_frac=0.3, sigma=0.5):
    """Views A (K_A), B and C (both K_B, 800 x 600): points uniform over image A at depths 4-12 that B and C both see.
    -> xa, xb, xc (N,2) noisy pixels — xc with `outlier_frac` of its rows replaced by pixels uniform over image C —, truth_c (N,),
    (R_ab, t_ab) with |t_ab| = BASELINE, (R_ac, t_ac) with |t_ac| = 1.5"""
    rng = np.random.default_rng([seed, 9])
    R_ab, t_ab = GS.scene_pose(motion_ab, seed)
    R_ac, t_ac = GS.scene_pose(motion_ac, seed + 100)
    t_ab, t_ac = BASELINE * t_ab, T_SCALE * t_ac

    def inside(u, z):
        return (z > 0.5) & (u[:, 0] >= 0) & (u[:, 0] < GS.W_B) & (u[:, 1] >= 0) & (u[:, 1] < GS.H_B)

    ua, ub, uc = [], [], []
    while sum(len(a) for a in ua) < N:
        u = GS._uniform(rng, GS.W_A, GS.H_A, 4 * N)
        X = GS.backproject(u, rng.uniform(4, 12, 4 * N), GS.K_A)
        Xb, Xc = X @ R_ab.T + t_ab, X @ R_ac.T + t_ac
        pb, pc = GS.project(Xb, GS.K_B), GS.project(Xc, GS.K_B)
        keep = inside(pb, Xb[:, 2]) & inside(pc, Xc[:, 2])
        ua.append(u[keep]); ub.append(pb[keep]); uc.append(pc[keep])
    xa, xb, xc = (np.concatenate(v)[:N] for v in (ua, ub, uc))
    xa, xb, xc = (v + rng.normal(0, sigma, v.shape) for v in (xa, xb, xc))
    truth = np.ones(N, bool)
    out = rng.permutation(N)[:int(round(N * outlier_frac))]
    truth[out] = False
    xc[out] = GS._uniform(rng, GS.W_B, GS.H_B, len(out))
    return xa, xb, xc, truth, (R_ab, t_ab), (R_ac, t_ac)


def chain_errors(R, t, R_ac, t_ac):
    """errors of a pose of C recovered in units of the A-B baseline: |centre - true centre / BASELINE|, rotation in degrees"""
    return float(np.linalg.norm(-R.T @ t + R_ac.T @ t_ac / BASELINE)), rotation_error_deg(R, R_ac)


def depth_map_scene(motion, seed, N=2000, outlier_frac=0.3, sigma=0.5, hole=(200, 300, 260, 420)):
    """A depth map of image A (H_A x W_A, depths 4.5-11.5, zero in the rectangle hole = (row0, col0, row1, col1)), N key-points uniform
    over image A, and their pixels in B under scene_pose(motion, seed) with |t| = 1.5: noisy, `outlier_frac` of them uniform over image
    B.  The true world point of a key-point uses the depth of the pixel it falls in, as lift_keypoints samples it; a key-point in the
    hole, behind B or outside image B is no inlier.  -> depth, kpts (N,2), xb (N,2), truth (N,), in_hole (N,), X_true (N,3), R, t"""
    rng = np.random.default_rng([seed, 13])
    R, t = GS.scene_pose(motion, seed)
    t = T_SCALE * t
    rows, cols = np.meshgrid(np.arange(GS.H_A) + 0.5, np.arange(GS.W_A) + 0.5, indexing="ij")
    depth = 8.0 + 2.0 * np.sin(cols / 200.0) + 1.5 * np.cos(rows / 150.0)
    depth[hole[0]:hole[2], hole[1]:hole[3]] = 0.0
    kpts = GS._uniform(rng, GS.W_A, GS.H_A, N)
    d = depth[np.floor(kpts[:, 1]).astype(int), np.floor(kpts[:, 0]).astype(int)]
    in_hole = d == 0.0
    X = GS.backproject(kpts, np.where(in_hole, 1.0, d), GS.K_A)
    Xb = X @ R.T + t
    xb = GS.project(Xb, GS.K_B)
    seen = ~in_hole & (Xb[:, 2] > 0.5) & (xb[:, 0] >= 0) & (xb[:, 0] < GS.W_B) & (xb[:, 1] >= 0) & (xb[:, 1] < GS.H_B)
    xb = xb + rng.normal(0, sigma, xb.shape)
    truth = seen & (rng.uniform(size=N) >= outlier_frac)
    rand = GS._uniform(rng, GS.W_B, GS.H_B, N)
    xb = np.where(truth[:, None], xb, rand)
    return depth, kpts, xb, truth, in_hole, X, R, t
