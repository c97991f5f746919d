"""numpy restatement of roma_amd.geometry.triangulate_nview (csrc/triangulate_nview.hip): a point seen in V posed views, convention
x_v ~ K_v (R_v X + t_v), triangulated from all of them with the views that disagree left out.

The per-call constants (K_v^-1, the centres C_v = -R_v^T t_v, their mean c0 over the usable views in view order, C'_v = C_v - c0,
t'_v = t_v + R_v c0) are computed in fp64 and then rounded to `dtype`; everything per point runs in `dtype`, statement for statement what
the kernel runs in fp32 (which may fuse a multiply with an add), vectorised over the points with Python loops over the views.  c0 is
added back in fp64.  dtype = float64, the default, is the reference the tests compare the device with; the float32 run of this very
code measures what fp32 costs, and the tests derive their tolerance from it.

view set: max_view_error = inf: the observed views.  Otherwise every pair (a, b), a < b, of observed views gives the midpoint of its
two rays; a view is an inlier with positive depth and a pixel error <= max_view_error; the hypothesis counts if a and b are inliers;
score = sum over observed views of (inlier ? e^2 : thr^2); lowest score, first pair on a tie; the set is the winner's inliers.
linear start: (sum I - d d^T) X = sum (I - d d^T) C' over the set, unit d = R^T K^-1 x~.  refinement: `iters` Levenberg-Marquardt steps on
the summed squared pixel error, lambda_0 = 1e-3 on the scaled diagonal, a step kept only if the cost drops."""
from __future__ import annotations

import numpy as np


def view_constants(K, R, t):
    """fp64: dict of k (V,5) = fx s cx fy cy, ki (V,5) = the five entries of K^-1, r (V,9), c (V,3) = C - c0, t (V,3) = t + R c0,
    ok (V,) = K invertible and pose finite, c0 (3,)"""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64)
    V = len(R)
    K = np.broadcast_to(K, (V, 3, 3))
    fx, s, cx, fy, cy = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    with np.errstate(all="ignore"):
        d = fx * fy
        ok = np.isfinite(K[:, :2]).all((1, 2)) & (d != 0) & np.isfinite(1.0 / d) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
        ki = np.stack([1.0 / fx, -s / d, (s * cy - cx * fy) / d, 1.0 / fy, -cy / fy], -1)
        C = -np.einsum("vij,vi->vj", R, t)
        c0, n = np.zeros(3), 0
        for v in range(V):                                            # a fixed order
            if ok[v]:
                c0, n = c0 + C[v], n + 1
        if n:
            c0 = c0 / n
        tp = t + np.einsum("vij,j->vi", R, c0)
    return {"k": np.stack([fx, s, cx, fy, cy], -1), "ki": ki, "r": R.reshape(V, 9), "c": C - c0, "t": tp, "ok": ok, "c0": c0}


def _bearing(ki, r, x, y):
    a0, a1 = ki[0] * x + ki[1] * y + ki[2], ki[3] * y + ki[4]
    d0, d1, d2 = r[0] * a0 + r[3] * a1 + r[6], r[1] * a0 + r[4] * a1 + r[7], r[2] * a0 + r[5] * a1 + r[8]
    inv = ki.dtype.type(1) / np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
    return d0 * inv, d1 * inv, d2 * inv


def _project(k, r, t, X, x, y):
    """q0, q1, z, 1/z and the pixel residual (ru, rv) of X (three arrays, relative to c0)"""
    q0 = r[0] * X[0] + r[1] * X[1] + r[2] * X[2] + t[0]
    q1 = r[3] * X[0] + r[4] * X[1] + r[5] * X[2] + t[1]
    z = r[6] * X[0] + r[7] * X[1] + r[8] * X[2] + t[2]
    iz = k.dtype.type(1) / z
    return q0, q1, z, iz, (k[0] * q0 + k[1] * q1) * iz + k[2] - x, k[3] * q1 * iz + k[4] - y


def _solve_sym3(a, b):
    a00, a01, a02, a11, a12, a22 = a
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    return ((c00 * b[0] + c01 * b[1] + c02 * b[2]) / det, (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det,
            (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det)


def _evaluate(c, px, py, member, X):
    """cost, minz, the six entries of J^T J and the three of J^T r over the views with member[v] set, summed in view order"""
    N = px.shape[1]
    zero = np.zeros(N, px.dtype)
    cost, minz = zero.copy(), np.full(N, np.inf, px.dtype)
    h, g = [zero.copy() for _ in range(6)], [zero.copy() for _ in range(3)]
    for v in range(len(px)):
        m = member[v]
        k, r = c["k"][v], c["r"][v]
        q0, q1, z, iz, ru, rv = _project(k, r, c["t"][v], X, px[v], py[v])
        cost = np.where(m, cost + (ru * ru + rv * rv), cost)
        minz = np.where(m & (z < minz), z, minz)
        u0, u1, u2 = k[0] * iz, k[1] * iz, -(k[0] * q0 + k[1] * q1) * iz * iz
        v1, v2 = k[3] * iz, -(k[3] * q1) * iz * iz
        ju = [u0 * r[j] + u1 * r[3 + j] + u2 * r[6 + j] for j in range(3)]
        jv = [v1 * r[3 + j] + v2 * r[6 + j] for j in range(3)]
        for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            h[i] = np.where(m, h[i] + (ju[a] * ju[b] + jv[a] * jv[b]), h[i])
        for j in range(3):
            g[j] = np.where(m, g[j] + (ju[j] * ru + jv[j] * rv), g[j])
    return cost, minz, h, g


def triangulate_nview(x, K, R, t, visible=None, to_px=None, max_view_error=np.inf, iters=3, min_views=2, max_reproj=np.inf,
                      max_cos_parallax=1.0, ref_view=0, dtype=np.float64):
    """x (V,N,2) -> dict of points (N,3), depth, reproj, cos_parallax (N,) in `dtype`, views (N,) uint32, num_views (N,), valid, finite
    (N,) bool; and for the tests: observed (V,N) bool, cost0 / cost (N,) the summed squared pixel error of the linear start / of the
    result, hyp_error (V,N) the pixel error of every view under the winning hypothesis (robust mode; inf behind the camera), member
    (V,N) the view set, minz the smallest depth over it, c0."""
    x = np.asarray(x)
    V, N = x.shape[:2]
    c64 = view_constants(K, R, t)
    c = {n: (v.astype(dtype) if n in ("k", "ki", "r", "c", "t") else v) for n, v in c64.items()}
    one, zero, half = dtype(1), dtype(0), dtype(0.5)
    xs = x.astype(dtype)
    with np.errstate(all="ignore"):
        if to_px is None:
            px, py = xs[..., 0], xs[..., 1]
        else:
            s = np.asarray(to_px, np.float64).astype(dtype).reshape(V, 4)
            px, py = xs[..., 0] * s[:, 0:1] + s[:, 1:2], xs[..., 1] * s[:, 2:3] + s[:, 3:4]
        obs = np.isfinite(px) & np.isfinite(py) & c["ok"][:, None]
        if visible is not None:
            obs &= np.asarray(visible).astype(bool)
        px, py = np.where(obs, px, np.nan).astype(dtype), np.where(obs, py, np.nan).astype(dtype)
        d = [_bearing(c["ki"][v], c["r"][v], px[v], py[v]) for v in range(V)]
        robust = np.isfinite(max_view_error)
        member = obs.copy()
        hyp_error = np.full((V, N), np.nan)
        if robust:
            thr2 = dtype(dtype(max_view_error) * dtype(max_view_error))
            best = np.full(N, np.inf, dtype)
            member = np.zeros((V, N), bool)
            for a in range(V - 1):
                for b in range(a + 1, V):
                    ca, cb, da, db = c["c"][a], c["c"][b], d[a], d[b]
                    w0, w1, w2 = ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]
                    ab = da[0] * db[0] + da[1] * db[1] + da[2] * db[2]
                    aw, bw = da[0] * w0 + da[1] * w1 + da[2] * w2, db[0] * w0 + db[1] * w1 + db[2] * w2
                    den = one - ab * ab
                    sa, sb = (ab * bw - aw) / den, (bw - ab * aw) / den
                    M = [half * ((ca[j] + sa * da[j]) + (cb[j] + sb * db[j])) for j in range(3)]
                    score, inl, err = np.zeros(N, dtype), np.zeros((V, N), bool), np.full((V, N), np.nan)
                    for v in range(V):
                        _, _, z, _, ru, rv = _project(c["k"][v], c["r"][v], c["t"][v], M, px[v], py[v])
                        e2 = ru * ru + rv * rv
                        inl[v] = obs[v] & (z > 0) & (e2 <= thr2)
                        score = np.where(obs[v], score + np.where(inl[v], e2, thr2), score)
                        err[v] = np.where(z > 0, np.sqrt(e2.astype(np.float64)), np.inf)
                    better = obs[a] & obs[b] & inl[a] & inl[b] & (score < best)
                    best = np.where(better, score, best)
                    member = np.where(better, inl, member)
                    hyp_error = np.where(better, err, hyp_error)
        nset = member.sum(0)
        # the point closest to the rays of the set
        A, rhs = [np.zeros(N, dtype) for _ in range(6)], [np.zeros(N, dtype) for _ in range(3)]
        for v in range(V):
            m, dv, cv = member[v], d[v], c["c"][v]
            dc = dv[0] * cv[0] + dv[1] * cv[1] + dv[2] * cv[2]
            add = (one - dv[0] * dv[0], -(dv[0] * dv[1]), -(dv[0] * dv[2]), one - dv[1] * dv[1], -(dv[1] * dv[2]), one - dv[2] * dv[2])
            for i in range(6):
                A[i] = np.where(m, A[i] + add[i], A[i])
            for j in range(3):
                rhs[j] = np.where(m, rhs[j] + (cv[j] - dv[j] * dc), rhs[j])
        X = list(_solve_sym3(A, rhs))
        cost, minz, h, g = _evaluate(c, px, py, member, X)
        cost0 = cost.copy()
        lam = np.full(N, dtype(1e-3), dtype)
        for _ in range(int(iters)):
            hd = [h[0] + lam * h[0], h[1], h[2], h[3] + lam * h[3], h[4], h[5] + lam * h[5]]
            step = _solve_sym3(hd, g)
            Xn = [X[j] - step[j] for j in range(3)]
            cn, mzn, hn, gn = _evaluate(c, px, py, member, Xn)
            keep = cn < cost
            X = [np.where(keep, Xn[j], X[j]) for j in range(3)]
            cost, minz = np.where(keep, cn, cost), np.where(keep, mzn, minz)
            h = [np.where(keep, hn[i], h[i]) for i in range(6)]
            g = [np.where(keep, gn[j], g[j]) for j in range(3)]
            lam = np.where(keep, lam * dtype(0.1), lam * dtype(10))
        reproj = np.sqrt(cost / nset.astype(dtype))
        rr, rt = c["r"][ref_view], c["t"][ref_view]
        z_ref = rr[6] * X[0] + rr[7] * X[1] + rr[8] * X[2] + rt[2]
        cosp = np.full(N, dtype(2), dtype)
        for a in range(V - 1):
            a0, a1, a2 = c["c"][a][0] - X[0], c["c"][a][1] - X[1], c["c"][a][2] - X[2]
            ia = one / np.sqrt(a0 * a0 + a1 * a1 + a2 * a2)
            for b in range(a + 1, V):
                b0, b1, b2 = c["c"][b][0] - X[0], c["c"][b][1] - X[1], c["c"][b][2] - X[2]
                ib = one / np.sqrt(b0 * b0 + b1 * b1 + b2 * b2)
                dd = (a0 * b0 + a1 * b1 + a2 * b2) * (ia * ib)
                cosp = np.where(member[a] & member[b] & (dd < cosp), dd, cosp)
        P = np.stack([(X[j].astype(np.float64) + c["c0"][j]).astype(dtype) for j in range(3)], -1)
        fin = (nset >= 2) & np.isfinite(X[0]) & np.isfinite(X[1]) & np.isfinite(X[2]) & np.isfinite(P).all(-1) & np.isfinite(z_ref) \
            & np.isfinite(reproj) & np.isfinite(minz) & (cosp <= dtype(1.5))
        valid = fin & (nset >= min_views) & (minz > 0) & (reproj <= dtype(max_reproj)) & (cosp <= dtype(max_cos_parallax))
    member = member & fin
    views = np.zeros(N, np.uint32)
    for v in range(V):
        views |= member[v].astype(np.uint32) << np.uint32(v)
    return {"points": np.where(fin[:, None], P, zero), "depth": np.where(fin, z_ref, zero), "reproj": np.where(fin, reproj, zero),
            "cos_parallax": np.where(fin, cosp, zero), "views": views, "num_views": member.sum(0), "valid": valid, "finite": fin,
            "observed": obs, "cost0": cost0, "cost": cost, "hyp_error": hyp_error, "c0": c["c0"], "member": member, "minz": minz}


def reprojection_errors(X, x, K, R, t):
    """fp64: (V,N) pixel distance between the projection of the world points X (N,3) and the observations x (V,N,2)"""
    K = np.broadcast_to(np.asarray(K, np.float64), (len(R), 3, 3))
    q = np.einsum("vij,nj->vni", np.asarray(R, np.float64), np.asarray(X, np.float64)) + np.asarray(t, np.float64)[:, None, :]
    p = np.einsum("vij,vnj->vni", K, q)
    with np.errstate(all="ignore"):
        return np.linalg.norm(p[..., :2] / p[..., 2:] - np.asarray(x, np.float64), axis=-1)
