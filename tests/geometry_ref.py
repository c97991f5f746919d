"""numpy restatement of roma_amd.geometry (csrc/geometry.hip): the sample draw bit for bit, Hartley normalisation, the 7-point
and 4-point solvers (null spaces by SVD, independent of the kernel's elimination), the pixel errors in fp64, and the whole RANSAC
(selection, least-squares local optimisation, de-normalisation).  Plus the synthetic scenes the tests score it on."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
STAGE = {"fundamental": 2, "homography": 3}
SMIN = {"fundamental": 7, "homography": 4}


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def usable(xa, xb):
    return np.isfinite(xa).all(-1) & np.isfinite(xb).all(-1)


def minimal_samples(xa, xb, model, iters, seed):
    """(P,N,2) pixel coordinates -> (P, iters, s) int32 indices, rows of -1 for invalid samples (geometry.hip header)."""
    P, N = xa.shape[0], xa.shape[1]
    s = SMIN[model]
    ok_pt = usable(xa, xb)
    stream = int(fmix32((int(seed) & M32) ^ ((STAGE[model] * 0x9E3779B9) & M32)))
    p = np.arange(P, dtype=np.uint64)[:, None]
    h = np.arange(iters, dtype=np.uint64)[None, :]
    idx = np.full((P, iters, s), -1, dtype=np.int64)
    for k in range(s):
        ctr = ((p * np.uint64(iters) + h) * np.uint64(8) + np.uint64(k)) & M32
        got = np.full((P, iters), -1, dtype=np.int64)
        for att in range(16):
            hs = fmix32((np.uint64(stream) + ctr * np.uint64(0x9E3779B1) + np.uint64(att * 0x7FEB352D)) & M32)
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


def normalisation(x, ok):
    """Hartley: (cx, cy, s) with x_hat = (x - c) * s, mean distance sqrt(2)."""
    if not ok.any():
        return 0.0, 0.0, 1.0
    c = x[ok].mean(0)
    md = np.sqrt(((x[ok] - c) ** 2).sum(-1)).mean()
    s = np.sqrt(2.0) / md if md > 0 else 1.0
    if not np.isfinite(s):
        s = 1.0
    return float(c[0]), float(c[1]), float(s)


def transform(c):
    cx, cy, s = c
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])


def unit(m):
    m = np.asarray(m, dtype=np.float64)
    n = np.sqrt((m.reshape(m.shape[:-2] + (9,)) ** 2).sum(-1))[..., None, None]
    return m / np.where(n > 0, n, 1.0)


def sign_fixed(m):
    """unit Frobenius norm, largest-magnitude entry positive (first on ties) — makes models comparable."""
    m = unit(m)
    flat = m.reshape(m.shape[:-2] + (9,))
    j = np.abs(flat).argmax(-1)
    sg = np.sign(np.take_along_axis(flat, j[..., None], -1))[..., None]
    sg = np.where(sg == 0, 1.0, sg)
    return m * sg


def f_rows(x, y, u, v):
    one = np.ones_like(x)
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], -1)


def h_rows(x, y, u, v):
    z, one = np.zeros_like(x), np.ones_like(x)
    r1 = np.stack([x, y, one, z, z, z, -u * x, -u * y, -u], -1)
    r2 = np.stack([z, z, z, x, y, one, -v * x, -v * y, -v], -1)
    return np.concatenate([r1, r2], -2)


def cubic_coeffs(f1, f2):
    """det(f2 + a (f1 - f2)) = c3 a^3 + c2 a^2 + c1 a + c0 from its values at a = 0, 1, -1, 2 (as the kernel)."""
    d = [np.linalg.det(f2 + a * (f1 - f2)) for a in (0.0, 1.0, -1.0, 2.0)]
    c0 = d[0]
    c2 = 0.5 * (d[1] + d[2]) - d[0]
    m = 0.5 * (d[1] - d[2])
    n = 0.5 * (d[3] - d[0] - 4 * c2)
    c3 = (n - m) / 3
    return c3, c2, m - c3, c0


def cubic_real_roots(c3, c2, c1, c0):
    """real roots of one cubic (lists), the kernel's branches: degree drop at |c3| <= 1e-12 max|c|, else companion roots."""
    cmax = max(abs(c3), abs(c2), abs(c1), abs(c0))
    if not cmax > 0:
        return []
    if abs(c3) <= 1e-12 * cmax:
        if abs(c2) <= 1e-12 * cmax:
            return [] if abs(c1) <= 1e-12 * cmax else [-c0 / c1]
        d = c1 * c1 - 4 * c2 * c0
        if d < 0:
            return []
        sq = np.sqrt(d)
        q = -0.5 * (c1 + (sq if c1 >= 0 else -sq))
        return [0.0] if q == 0 else [q / c2, c0 / q]
    a, b, c = c2 / c3, c1 / c3, c0 / c3
    p = b - a * a / 3
    q = 2 * a ** 3 / 27 - a * b / 3 + c
    disc = 0.25 * q * q + p ** 3 / 27
    if p < 0 and disc <= 0:
        r = 2 * np.sqrt(-p / 3)
        arg = np.clip(3 * q / (2 * p) * np.sqrt(-3 / p), -1, 1)
        phi = np.arccos(arg) / 3
        roots = [r * np.cos(phi - 2 * np.pi * k / 3) - a / 3 for k in range(3)]
    else:
        sq = np.sqrt(max(disc, 0.0))
        roots = [np.cbrt(-0.5 * q + sq) + np.cbrt(-0.5 * q - sq) - a / 3]
    out = []
    for x in roots:
        for _ in range(2):
            f = ((c3 * x + c2) * x + c1) * x + c0
            df = (3 * c3 * x + 2 * c2) * x + c1
            if df != 0:
                x = x - f / df
        out.append(float(x))
    return out


def cubic_discriminant_rel(c3, c2, c1, c0):
    """discriminant of the cubic over the sum of the magnitudes of its terms (near 0: a double root, the count is ambiguous)."""
    t = [18 * c3 * c2 * c1 * c0, -4 * c2 ** 3 * c0, c2 ** 2 * c1 ** 2, -4 * c3 * c1 ** 3, -27 * c3 ** 2 * c0 ** 2]
    return abs(sum(t)) / max(sum(abs(x) for x in t), 1e-300)


def seven_point(xh, xh2):
    """xh, xh2: (7,2) normalised points of A and B -> (list of unit-norm 3x3 models, cubic coefficients, condition number)."""
    A = f_rows(xh[:, 0], xh[:, 1], xh2[:, 0], xh2[:, 1])
    _, sv, vt = np.linalg.svd(A)
    f1, f2 = vt[-2].reshape(3, 3), vt[-1].reshape(3, 3)
    co = cubic_coeffs(f1, f2)
    models = [unit(a * f1 + (1 - a) * f2) for a in cubic_real_roots(*co)]
    return models, co, sv[0] / sv[-1]


def four_point(xh, xh2):
    A = h_rows(xh[:, 0], xh[:, 1], xh2[:, 0], xh2[:, 1])
    _, sv, vt = np.linalg.svd(A)
    return unit(vt[-1].reshape(3, 3)), sv[0] / sv[-1]


def collinear(p):
    """any 3 of the 4 points (4,2) collinear (the kernel's test)"""
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        u, v = p[j] - p[i], p[k] - p[i]
        if abs(u[0] * v[1] - u[1] * v[0]) <= 1e-6 * np.hypot(*u) * np.hypot(*v):
            return True
    return False


def errors(model, M, xa, xb):
    """squared pixel errors (fp64) of pixel-space model M: Sampson for F, forward transfer for H; NaN for unusable points."""
    ha = np.concatenate([xa, np.ones_like(xa[..., :1])], -1)
    hb = np.concatenate([xb, np.ones_like(xb[..., :1])], -1)
    with np.errstate(all="ignore"):
        if model == "fundamental":
            fx = ha @ np.swapaxes(M, -1, -2)
            ftx = hb @ M
            num = (hb * fx).sum(-1)
            return num ** 2 / (fx[..., 0] ** 2 + fx[..., 1] ** 2 + ftx[..., 0] ** 2 + ftx[..., 1] ** 2)
        hx = ha @ np.swapaxes(M, -1, -2)
        pr = hx[..., :2] / hx[..., 2:3]
        return ((xb - pr) ** 2).sum(-1)


def denormalise(model, Mh, TA, TB):
    return TB.T @ Mh @ TA if model == "fundamental" else np.linalg.inv(TB) @ Mh @ TA


def finish(model, M):
    if model == "fundamental":
        return sign_fixed(M)
    fro = np.sqrt((M ** 2).sum())
    return unit(M) if abs(M[2, 2]) < 1e-12 * fro else M / M[2, 2]


def ransac(model, xa, xb, threshold, iters, seed, lo_iters=3):
    """One pair (N,2) -> (model (3,3) in pixels, inlier mask).  fp64 throughout (the kernel scores in fp32)."""
    N = xa.shape[0]
    ok = usable(xa, xb)
    cA, cB = normalisation(xa, ok), normalisation(xb, ok)
    TA, TB = transform(cA), transform(cB)
    xh = (xa - cA[:2]) * cA[2]
    xh2 = (xb - cB[:2]) * cB[2]
    idx = minimal_samples(xa[None], xb[None], model, iters, seed)[0]
    t2 = threshold ** 2
    cands = []                         # (slot index, normalised model)
    for h in range(iters):
        if idx[h, 0] < 0:
            continue
        s = idx[h]
        if model == "fundamental":
            ms, _, _ = seven_point(xh[s], xh2[s])
            cands += [(3 * h + r, m) for r, m in enumerate(ms)]
        else:
            if collinear(xh[s]) or collinear(xh2[s]):
                continue
            m, _ = four_point(xh[s], xh2[s])
            cands.append((h, m))
    if not cands:
        return np.zeros((3, 3)), np.zeros(N, dtype=bool)
    Ms = np.stack([denormalise(model, m, TA, TB) for _, m in cands])
    e = errors(model, Ms, xa, xb)                            # (K, N)
    inl = e < t2
    cost = np.where(inl, e, t2).sum(-1)
    best = int(np.argmin(cost))        # first minimum = lowest slot index on ties (cands are in slot order)
    cur, cc, cin = cands[best][1], cost[best], inl[best]
    for _ in range(lo_iters):
        if cin.sum() < (8 if model == "fundamental" else 4):
            break
        i = np.nonzero(cin)[0]
        rows = (f_rows if model == "fundamental" else h_rows)(xh[i, 0], xh[i, 1], xh2[i, 0], xh2[i, 1])
        rows = rows.reshape(-1, 9)
        w, V = np.linalg.eigh(rows.T @ rows)
        cand = V[:, 0].reshape(3, 3)
        if model == "fundamental":
            U, S, Vt = np.linalg.svd(cand)
            cand = U @ np.diag([S[0], S[1], 0.0]) @ Vt
        cand = unit(cand)
        e2 = errors(model, denormalise(model, cand, TA, TB), xa, xb)
        in2 = e2 < t2
        c2 = np.where(in2, e2, t2).sum()
        if not c2 < cc:
            break
        cur, cc, cin = cand, c2, in2
    M = finish(model, denormalise(model, cur, TA, TB))
    return M, errors(model, M, xa, xb) < t2


# ------------------------------------------------------------------------------------------------------------------ scenes
W_IMG, H_IMG = 1024, 768


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    k = skew(w / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def two_view_scene(seed, N=5000, outlier_frac=0.4, sigma=0.5):
    """1024x768, f = 800, depths 4-12.  Returns xa, xb (noisy, outliers uniform over image B), is_inlier, F_true, clean xa, xb."""
    rng = np.random.default_rng(seed)
    K = np.array([[800.0, 0, W_IMG / 2], [0, 800.0, H_IMG / 2], [0, 0, 1]])
    R = rodrigues(rng.normal(size=3) * 0.08)
    t = np.array([1.0, 0.1 * rng.normal(), 0.1 * rng.normal()])
    n_in = int(round(N * (1 - outlier_frac)))
    pa, pb = [], []
    while sum(len(a) for a in pa) < n_in:
        u = np.stack([rng.uniform(0, W_IMG, 4 * n_in), rng.uniform(0, H_IMG, 4 * n_in)], -1)
        d = rng.uniform(4, 12, 4 * n_in)
        X = (np.linalg.inv(K) @ np.concatenate([u, np.ones((len(u), 1))], -1).T).T * d[:, None]
        Xb = X @ R.T + t
        ub = Xb @ K.T
        ub = ub[:, :2] / ub[:, 2:3]
        keep = (Xb[:, 2] > 0) & (ub[:, 0] >= 0) & (ub[:, 0] < W_IMG) & (ub[:, 1] >= 0) & (ub[:, 1] < H_IMG)
        pa.append(u[keep])
        pb.append(ub[keep])
    ca, cb = np.concatenate(pa)[:n_in], np.concatenate(pb)[:n_in]
    F = np.linalg.inv(K).T @ skew(t) @ R @ np.linalg.inv(K)
    n_out = N - n_in
    oa = np.stack([rng.uniform(0, W_IMG, n_out), rng.uniform(0, H_IMG, n_out)], -1)
    ob = np.stack([rng.uniform(0, W_IMG, n_out), rng.uniform(0, H_IMG, n_out)], -1)
    xa = np.concatenate([ca + rng.normal(0, sigma, ca.shape), oa])
    xb = np.concatenate([cb + rng.normal(0, sigma, cb.shape), ob])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(N)
    clean_a = np.concatenate([ca, oa])[perm]
    clean_b = np.concatenate([cb, ob])[perm]
    return xa[perm], xb[perm], truth[perm], sign_fixed(F), clean_a, clean_b


def planar_scene(seed, N=5000, outlier_frac=0.5, sigma=0.5):
    """A homography from corners moved by up to 80 px (well conditioned), matches uniform over image A.  xa, xb, is_inlier, H_true."""
    rng = np.random.default_rng(seed)
    src = np.array([[0, 0], [W_IMG, 0], [W_IMG, H_IMG], [0, H_IMG]], dtype=np.float64)
    dst = src + rng.uniform(-80, 80, src.shape)
    A = h_rows(src[:, 0], src[:, 1], dst[:, 0], dst[:, 1])
    H = np.linalg.svd(A)[2][-1].reshape(3, 3)
    H = H / H[2, 2]
    n_in = int(round(N * (1 - outlier_frac)))
    ca = np.stack([rng.uniform(0, W_IMG, n_in), rng.uniform(0, H_IMG, n_in)], -1)
    hb = np.concatenate([ca, np.ones((n_in, 1))], -1) @ H.T
    cb = hb[:, :2] / hb[:, 2:3]
    n_out = N - n_in
    oa = np.stack([rng.uniform(0, W_IMG, n_out), rng.uniform(0, H_IMG, n_out)], -1)
    ob = np.stack([rng.uniform(0, W_IMG, n_out), rng.uniform(0, H_IMG, n_out)], -1)
    xa = np.concatenate([ca + rng.normal(0, sigma, ca.shape), oa])
    xb = np.concatenate([cb + rng.normal(0, sigma, cb.shape), ob])
    truth = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(N)
    return xa[perm], xb[perm], truth[perm], H


def corner_error(H_est, H_true):
    c = np.array([[0, 0, 1], [W_IMG, 0, 1], [W_IMG, H_IMG, 1], [0, H_IMG, 1]], dtype=np.float64)
    a, b = c @ H_est.T, c @ H_true.T
    return float(np.linalg.norm(a[:, :2] / a[:, 2:3] - b[:, :2] / b[:, 2:3], axis=1).mean())


def recall_precision(mask, truth):
    tp = (mask & truth).sum()
    return tp / max(truth.sum(), 1), tp / max(mask.sum(), 1)
