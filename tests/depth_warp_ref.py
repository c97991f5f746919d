"""numpy fp64 restatement of csrc/depth_warp.hip: warp_kpts / get_gt_warp of the reference (romatch/utils/utils.py:326-455) and
geometric_dist of its dense MegaDepth benchmark, with grid_sample (align_corners=False, zero padding; bilinear and nearest) written
out, plus the synthetic scene the tests and tests/golden/make_golden_depth_warp.py share.  Shapes are those of one pair unless a
function says otherwise: key-points (N,2), depth maps (H,W), T (3,4) or (4,4), K (3,3)."""
import numpy as np

MODES = ("bilinear", "nearest", "combined")


def adjugate_inverse(K):
    """K^-1 of any 3x3 by the adjugate, as the kernel computes it: inf / NaN entries for a singular K"""
    a, b, c, d, e, f, g, h, i = (float(v) for v in np.asarray(K, np.float64).reshape(9))
    A, B, C = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * A + b * B + c * C
    adj = np.array([[A, c * h - b * i, b * f - c * e], [B, a * i - c * g, c * d - a * f], [C, b * g - a * h, a * e - b * d]])
    with np.errstate(all="ignore"):
        return adj / det


def grid_sample(depth, x, y, mode):
    """F.grid_sample(depth[None, None], (x, y), mode, padding_mode='zeros', align_corners=False) at N points, in fp64.  Points that
    are NaN, inf or outside sample 0."""
    d = np.asarray(depth, np.float64)
    H, W = d.shape
    with np.errstate(all="ignore"):
        ix, iy = ((x + 1.0) * W - 1.0) / 2.0, ((y + 1.0) * H - 1.0) / 2.0

        def tap(xi, yi):
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)                      # NaN fails
            out = np.zeros(ix.shape)
            out[ok] = d[yi[ok].astype(np.int64), xi[ok].astype(np.int64)]
            return out

        if mode == "nearest":
            return tap(np.rint(ix), np.rint(iy))                                          # ties to even
        assert mode == "bilinear", mode
        fx, fy = np.floor(ix), np.floor(iy)
        wx1, wx0, wy1, wy0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
        inside = (ix > -1.0) & (ix < W) & (iy > -1.0) & (iy < H)
        out = tap(fx, fy) * (wx0 * wy0) + tap(fx + 1, fy) * (wx1 * wy0) + tap(fx, fy + 1) * (wx0 * wy1) + tap(fx + 1, fy + 1) * (wx1 * wy1)
        return np.where(inside, out, 0.0)


def warp_kpts(kpts, depth_A, depth_B, T, K_A, K_B, mode="bilinear", threshold=0.05):
    """-> dict: valid (N,) bool, x2 (N,2), rel_err (N,), and the intermediate u, v (pixels in B) the margin checks read"""
    if mode == "combined":
        o, n = (warp_kpts(kpts, depth_A, depth_B, T, K_A, K_B, m, threshold) for m in ("bilinear", "nearest"))
        take = ~o["valid"] & n["valid"]
        return {"valid": o["valid"] | n["valid"], "x2": np.where(take[:, None], n["x2"], o["x2"]),
                "rel_err": np.where(take, n["rel_err"], o["rel_err"])}
    k = np.asarray(kpts, np.float32).astype(np.float64)                                   # the kernel reads fp32
    x, y = k[:, 0], k[:, 1]
    dA, dB = np.asarray(depth_A, np.float32), np.asarray(depth_B, np.float32)
    Ha, Wa = dA.shape
    Hb, Wb = dB.shape
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    with np.errstate(all="ignore"):
        d = grid_sample(dA, x, y, mode)
        px, py = Wa * (x + 1.0) / 2.0, Ha * (y + 1.0) / 2.0
        XA = np.stack([px * d, py * d, d], -1) @ adjugate_inverse(K_A).T
        XB = XA @ R.T + t
        z = XB[:, 2]
        ph = XB @ np.asarray(K_B, np.float64).T
        u, v = ph[:, 0] / (ph[:, 2] + 1e-4), ph[:, 1] / (ph[:, 2] + 1e-4)
        covisible = (u > 0) & (u < Wb - 1) & (v > 0) & (v < Hb - 1)
        x2 = np.stack([2.0 * u / Wb - 1.0, 2.0 * v / Hb - 1.0], -1)
        d2 = grid_sample(dB, x2[:, 0], x2[:, 1], mode)
        rel = np.abs((d2 - z) / d2)
        valid = (d != 0) & covisible & (rel < threshold)
    return {"valid": valid, "x2": x2, "rel_err": rel, "u": u, "v": v, "nonzero": d != 0, "covisible": covisible}


def linspace_f32(n):
    """torch.linspace(-1 + 1/n, 1 - 1/n, n) in fp32 as ATen evaluates it on the CPU: start + step * i below the midpoint, end - step *
    (n - 1 - i) from it on, each a fused multiply-add (one rounding; the product of two fp32 is exact in fp64, and the sum is rounded
    once more to fp32 — double rounding cannot bite at these magnitudes for the sizes used here, the golden generator compares)"""
    start, end = np.float32(-1 + 1 / n), np.float32(1 - 1 / n)
    if n == 1:
        return np.array([start], np.float32)
    step = np.float64(np.float32((end - start) / np.float32(n - 1)))
    i = np.arange(n)
    lo = (np.float64(start) + step * i).astype(np.float32)
    hi = (np.float64(end) - step * (n - 1 - i)).astype(np.float32)
    return np.where(i < n // 2, lo, hi).astype(np.float32)


def gt_grid(H, W):
    """(H*W, 2) fp32 [x, y] pixel centres"""
    gx, gy = np.meshgrid(linspace_f32(W), linspace_f32(H), indexing="xy")
    return np.stack([gx, gy], -1).reshape(H * W, 2).astype(np.float32)


def get_gt_warp(depth_A, depth_B, T, K_A, K_B, mode="bilinear", threshold=0.05, H=None, W=None, grid=None):
    """-> x2 (H,W,2) fp64, prob (H,W) float32; grid: the (H*W,2) fp32 key-points to use instead of gt_grid(H, W)"""
    if H is None:
        H, W = np.asarray(depth_A).shape
    o = warp_kpts(gt_grid(H, W) if grid is None else grid, depth_A, depth_B, T, K_A, K_B, mode, threshold)
    return o["x2"].reshape(H, W, 2), o["valid"].astype(np.float32).reshape(H, W)


def geometric_dist(warp, depth_A, depth_B, T, K_A, K_B, mode="bilinear", threshold=0.05):
    """warp (H,W,4) fp32 -> dict: gd (H,W) fp64 of every pixel, valid (H,W) bool, epe_sum, counts (4,) int64 [valid, <1, <3, <5]"""
    w = np.asarray(warp, np.float32)
    H, W = w.shape[:2]
    o = warp_kpts(w[..., :2].reshape(-1, 2), depth_A, depth_B, T, K_A, K_B, mode, threshold)
    with np.errstate(all="ignore"):
        x2 = np.stack([W * (o["x2"][:, 0] + 1.0) / 2.0, H * (o["x2"][:, 1] + 1.0) / 2.0], -1)
        # fp32, in the reference's order: (w1 * (c + 1)) / 2 on the fp32 dense_matches
        hat = np.stack([(np.float32(W) * (w[..., 2] + np.float32(1))) / np.float32(2), (np.float32(H) * (w[..., 3] + np.float32(1))) / np.float32(2)], -1)
        assert hat.dtype == np.float32
        e = hat.reshape(-1, 2).astype(np.float64) - x2
        gd = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    valid = o["valid"]
    g = gd[valid]
    counts = np.array([valid.sum(), (g < 1.0).sum(), (g < 3.0).sum(), (g < 5.0).sum()], np.int64)
    return {"gd": gd.reshape(H, W), "valid": valid.reshape(H, W), "epe_sum": float(g.sum()), "counts": counts}


# ------------------------------------------------------------------------------------------------------------------ the scene
PLANES = ((np.array([0.2, 0.1, 1.0]), 5.0), (np.array([-0.1, 0.0, 1.0]), 3.0))          # n . X = d in A's frame
OCCLUDER_X = (-0.8, 0.3)                                                                # the second plane exists where its A-frame X lies here


def cameras(Ha, Wa, Hb, Wb, variant=0):
    """K_A, K_B, T (3,4).  variant 0 is the base recipe; others perturb focal lengths, angle and translation a little."""
    s = 1.0 + 0.05 * variant
    K_A = np.array([[0.9 * Wa * s, 0, Wa / 2], [0, 0.9 * Wa * s, Ha / 2], [0, 0, 1.0]])
    K_B = np.array([[1.1 * Wb / s, 0, Wb / 2 + 3], [0, 1.0 * Wb / s, Hb / 2 - 2], [0, 0, 1.0]])
    a = 0.12 + 0.02 * variant
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.6, 0.05, 0.1]) * (1.0 + 0.1 * variant)
    return K_A, K_B, np.concatenate([R, t[:, None]], 1)


def _render(H, W, K, R, t):
    """depth (z in this camera) of the nearest visible plane through every pixel centre; the camera sees X_cam = R X_A + t"""
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    ray = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T                     # X_cam = z * ray
    best = np.full((H, W), np.inf)
    for k, (n, d) in enumerate(PLANES):
        # X_A = R^T (z ray - t);  n . X_A = d  ->  z = (d + n . R^T t) / (n . R^T ray)
        nr = R @ n
        z = (d + nr @ t) / (ray @ nr)
        XA = (z[..., None] * ray - t) @ R
        ok = z > 0
        if k == 1:
            ok &= (XA[..., 0] > OCCLUDER_X[0]) & (XA[..., 0] < OCCLUDER_X[1])
        best = np.where(ok & (z < best), z, best)
    assert np.isfinite(best).all()
    return best


def scene(seed, Ha=23, Wa=37, Hb=29, Wb=31, variant=0):
    """-> dict of one pair: depth_A (Ha,Wa), depth_B (Hb,Wb) fp32 with 1 % multiplicative noise and 5 % holes, K_A, K_B, T (3,4) fp64,
    kpts (Ha*Wa, 2) fp32 = the pixel centres of A plus N(0, 0.7 / W_A) jitter."""
    rng = np.random.default_rng(seed)
    K_A, K_B, T = cameras(Ha, Wa, Hb, Wb, variant)
    maps = []
    for H, W, K, R, t in ((Ha, Wa, K_A, np.eye(3), np.zeros(3)), (Hb, Wb, K_B, T[:, :3], T[:, 3])):
        d = _render(H, W, K, R, t) * (1.0 + 0.01 * rng.standard_normal((H, W)))
        d[rng.random((H, W)) < 0.05] = 0.0
        maps.append(d.astype(np.float32))
    gx, gy = np.meshgrid(np.linspace(-1 + 1 / Wa, 1 - 1 / Wa, Wa), np.linspace(-1 + 1 / Ha, 1 - 1 / Ha, Ha), indexing="xy")
    kpts = np.stack([gx, gy], -1).reshape(-1, 2) + rng.normal(0, 0.7 / Wa, (Ha * Wa, 2))
    return {"depth_A": maps[0], "depth_B": maps[1], "K_A": K_A, "K_B": K_B, "T": T, "kpts": kpts.astype(np.float32)}


def margins(o, Hb, Wb, threshold=0.05):
    """how close any decision of a warp_kpts result comes to its threshold: (min |rel - threshold| over the points where rel is what
    decides, min distance in pixels of u, v to a covisibility border over the points with a depth)"""
    with np.errstate(all="ignore"):
        rel = np.abs(o["rel_err"] - threshold)[o["nonzero"] & o["covisible"]]
        nz = o["nonzero"] & np.isfinite(o["u"]) & np.isfinite(o["v"])
        b = np.minimum.reduce([np.abs(o["u"]), np.abs(o["u"] - (Wb - 1)), np.abs(o["v"]), np.abs(o["v"] - (Hb - 1))])[nz]
    return float(np.nanmin(rel)) if rel.size else np.inf, float(b.min()) if b.size else np.inf
