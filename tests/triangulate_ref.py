"""numpy restatement of roma_amd.geometry.triangulate (csrc/triangulate.hip): two-view triangulation of matches under a known relative
pose, convention x_B ~ K_B (R X_A + t), points in camera A's frame, depths in units of |t|.

The per-pair constants (the pixel-space F = K_B^-T [t]x R K_A^-1 of unit Frobenius norm, the two inverse intrinsics) are computed in
fp64 and then rounded to `dtype`; everything per match runs in `dtype`, statement for statement what the kernel runs in fp32 (which
may fuse a multiply with an add and so is at least as accurate).  dtype = float64, the default, is the reference the tests compare
the device with; the float32 run of this very code measures what fp32 costs, and the tests derive their tolerance from it.

method "optimal": Lindstrom, "Triangulation made easy" (CVPR 2010), the closed-form two-step correction (niter2) in pixel space with F:
(x_A, x_B) moves by the smallest |d_A|^2 + |d_B|^2 onto x_B^T F x_A = 0, to first order twice; the corrected rays meet, and the depths
lambda_A, lambda_B of lambda_B b = lambda_A R a + t are the least-squares closed form that recover_pose votes with.  X_A = lambda_A a,
reproj = sqrt(|d_A|^2 + |d_B|^2).
method "midpoint": the same closed form on the uncorrected rays, X the midpoint of the two closest points, reproj the root of the sum
over both images of the squared pixel distance between the projection of X and the match."""
from __future__ import annotations

import numpy as np

from tests import geometry_ref as G

METHODS = ("optimal", "midpoint")


def pair_constants(KA, KB, R, t):
    """fp64: F (3,3) with x_B^T F x_A = 0 in pixels, unit Frobenius norm (all zeros when [t]x R vanishes), K_A^-1, K_B^-1."""
    KA, KB, R, t = (np.asarray(v, np.float64) for v in (KA, KB, R, t))
    iA, iB = np.linalg.inv(KA), np.linalg.inv(KB)
    F = iB.T @ G.skew(t) @ R @ iA
    n = np.sqrt((F * F).sum())
    F = F / n if n > 0 else np.zeros((3, 3))
    return F, iA, iB


def to_px_of(H_A, W_A, H_B, W_B):
    """the 8 numbers (sx_A, ox_A, sy_A, oy_A, sx_B, ox_B, sy_B, oy_B) of to_pixel_coordinates: pixel = s * c + o"""
    return np.array([W_A / 2, W_A / 2, H_A / 2, H_A / 2, W_B / 2, W_B / 2, H_B / 2, H_B / 2], np.float64)


def pixels(m, to_px, dtype):
    m = np.asarray(m).astype(dtype)
    if to_px is None:
        return m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    s = np.asarray(to_px, np.float64).astype(dtype)
    return m[:, 0] * s[0] + s[1], m[:, 1] * s[2] + s[3], m[:, 2] * s[4] + s[5], m[:, 3] * s[6] + s[7]


def correct(xa, ya, xb, yb, F):
    """Lindstrom's niter2 on arrays of pixel coordinates.  Returns (dxa, dya, dxb, dyb, ok): the corrected match is x - d; ok is False
    where b^2 - ac < 0 or a denominator is zero."""
    f = F.reshape(9)
    nb0, nb1 = f[0] * xa + f[1] * ya + f[2], f[3] * xa + f[4] * ya + f[5]                  # (F x_A)[:2]
    l2 = f[6] * xa + f[7] * ya + f[8]
    na0, na1 = f[0] * xb + f[3] * yb + f[6], f[1] * xb + f[4] * yb + f[7]                  # (F^T x_B)[:2]
    c = xb * nb0 + yb * nb1 + l2
    a = nb0 * (f[0] * na0 + f[1] * na1) + nb1 * (f[3] * na0 + f[4] * na1)
    b = (nb0 * nb0 + nb1 * nb1 + na0 * na0 + na1 * na1) * f.dtype.type(0.5)
    disc = b * b - a * c
    with np.errstate(all="ignore"):
        d = np.sqrt(disc)
        den1 = b + d
        lam = c / den1
        da0, da1, db0, db1 = lam * na0, lam * na1, lam * nb0, lam * nb1
        nb0, nb1 = nb0 - (f[0] * da0 + f[1] * da1), nb1 - (f[3] * da0 + f[4] * da1)
        na0, na1 = na0 - (f[0] * db0 + f[3] * db1), na1 - (f[1] * db0 + f[4] * db1)
        den2 = nb0 * nb0 + nb1 * nb1 + na0 * na0 + na1 * na1
        lam = lam * ((d + d) / den2)
    ok = (disc >= 0) & (den1 != 0) & (den2 != 0)
    return lam * na0, lam * na1, lam * nb0, lam * nb1, ok


def triangulate(m, KA, KB, R, t, method="optimal", to_px=None, mask=None, max_reproj=np.inf, max_cos_parallax=1.0, dtype=np.float64):
    """m (N,4) rows [xa, ya, xb, yb] -> dict of points (N,3), depth_a, depth_b, reproj, cos_parallax (N,) in `dtype`, valid (N,) bool,
    and (method optimal) corrected (N,4), the match moved onto the epipolar constraint."""
    if method not in METHODS:
        raise ValueError(method)
    F, iA, iB = pair_constants(KA, KB, R, t)
    F, iA, iB = F.astype(dtype), iA.astype(dtype), iB.astype(dtype)
    kA, kB = np.asarray(KA, np.float64).astype(dtype), np.asarray(KB, np.float64).astype(dtype)
    r, tt = np.asarray(R, np.float64).astype(dtype).reshape(9), np.asarray(t, np.float64).astype(dtype)
    xa, ya, xb, yb = pixels(m, to_px, dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        fin = np.isfinite(xa) & np.isfinite(ya) & np.isfinite(xb) & np.isfinite(yb)
        ua, va, ub, vb = xa, ya, xb, yb
        out = {}
        if method == "optimal":
            da0, da1, db0, db1, ok = correct(xa, ya, xb, yb, F)
            fin &= ok
            ua, va, ub, vb = xa - da0, ya - da1, xb - db0, yb - db1
            reproj = np.sqrt(da0 * da0 + da1 * da1 + db0 * db0 + db1 * db1)
            out["corrected"] = np.stack([ua, va, ub, vb], -1)
        a0, a1 = iA[0, 0] * ua + iA[0, 1] * va + iA[0, 2], iA[1, 1] * va + iA[1, 2]          # a = K_A^-1 x_A, a_z = 1
        b0, b1 = iB[0, 0] * ub + iB[0, 1] * vb + iB[0, 2], iB[1, 1] * vb + iB[1, 2]
        q0, q1, q2 = r[0] * a0 + r[1] * a1 + r[2], r[3] * a0 + r[4] * a1 + r[5], r[6] * a0 + r[7] * a1 + r[8]     # R a
        aa, bb, ab = q0 * q0 + q1 * q1 + q2 * q2, b0 * b0 + b1 * b1 + one, q0 * b0 + q1 * b1 + q2
        at, bt = q0 * tt[0] + q1 * tt[1] + q2 * tt[2], b0 * tt[0] + b1 * tt[1] + tt[2]
        det = aa * bb - ab * ab
        la, lb = (ab * bt - bb * at) / det, (aa * bt - ab * at) / det
        cosp = ab / np.sqrt(aa * bb)
        if method == "optimal":
            X, Y, Z = la * a0, la * a1, la
            zb = lb
        else:
            # the midpoint in B's frame, then back into A's: X_A = R^T (X_B - t)
            h = dtype(0.5)
            m0, m1, m2 = h * (la * q0 + tt[0] + lb * b0), h * (la * q1 + tt[1] + lb * b1), h * (la * q2 + tt[2] + lb)
            e0, e1, e2 = m0 - tt[0], m1 - tt[1], m2 - tt[2]
            X, Y, Z = r[0] * e0 + r[3] * e1 + r[6] * e2, r[1] * e0 + r[4] * e1 + r[7] * e2, r[2] * e0 + r[5] * e1 + r[8] * e2
            zb = m2
            pa0, pa1 = (kA[0, 0] * X + kA[0, 1] * Y) / Z + kA[0, 2] - xa, kA[1, 1] * Y / Z + kA[1, 2] - ya
            pb0, pb1 = (kB[0, 0] * m0 + kB[0, 1] * m1) / m2 + kB[0, 2] - xb, kB[1, 1] * m1 / m2 + kB[1, 2] - yb
            reproj = np.sqrt(pa0 * pa0 + pa1 * pa1 + pb0 * pb0 + pb1 * pb1)
        fin &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(zb) & np.isfinite(reproj) & np.isfinite(cosp)
        valid = fin & (Z > 0) & (zb > 0) & (reproj <= dtype(max_reproj)) & (cosp <= dtype(max_cos_parallax))
    if mask is not None:
        valid &= np.asarray(mask).astype(bool)
    z = dtype(0)
    out.update(points=np.where(fin[:, None], np.stack([X, Y, Z], -1), z), depth_a=np.where(fin, Z, z), depth_b=np.where(fin, zb, z),
               reproj=np.where(fin, reproj, z), cos_parallax=np.where(fin, cosp, z), valid=valid, finite=fin)
    if "corrected" in out:
        out["corrected"] = np.where(fin[:, None], out["corrected"], z)
    return out


def reprojection_sq(X, m, KA, KB, R, t):
    """fp64: the sum over both images of the squared pixel distance between the projection of X (N,3, A's frame) and the match"""
    X = np.asarray(X, np.float64)
    pa = X @ np.asarray(KA, np.float64).T
    pb = (X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)) @ np.asarray(KB, np.float64).T
    m = np.asarray(m, np.float64)
    return ((pa[:, :2] / pa[:, 2:] - m[:, :2]) ** 2).sum(-1) + ((pb[:, :2] / pb[:, 2:] - m[:, 2:]) ** 2).sum(-1)
