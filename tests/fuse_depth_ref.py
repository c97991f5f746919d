"""numpy fp64 restatement of roma_depth_fuse (include/roma_hip.h, roma_amd/csrc/depth_fuse.hip): the three passes exactly as they are
defined, by the plain chain X = R_r^T (K_r^-1 (u d, v d, d) - t_r), q = K_s (R_s X + t_s) — not by the kernel's pair constants —, and for
every decision its distance to the threshold.

fuse_depth_ref(depths, R, t, K, ...) -> dict
  per view (lists of (H_v, W_v) arrays): depth64 (the fused depth in fp64, 0 where not valid), depth (that rounded to fp32), valid, views
    (int32 bit patterns), num_views (uint8), emit (valid and not a duplicate), dup, owner ((H_v, W_v, 3) int: view, row, column of the
    LOWEST view a duplicate points to, -1 elsewhere), consistent ((V, H_v, W_v) bool, consistent[s] = view s is consistent)
  the cloud (max_points rows, or every emitted pixel with max_points=None): points64, points (fp32), view, pixel, point_views, counts
  margins: {name: 1-D array}, the distances of the decisions taken to their thresholds
    "qz" |q.z|, "tap" the distance of (u_s - 0.5, v_s - 0.5) to the border of the region in which all four taps are inside,
    "pz" |p.z|, "reproj" | |p.xy / p.z - (u, v)| - max_reproj_error |, "depth" | |p.z - d| / d - max_depth_error |,
    "border" the distance of (u_s, v_s) to the nearest pixel border at an ownership lookup
"""
from __future__ import annotations

import numpy as np


def scaled_intrinsics(K, dims, sizes):
    """K (3,3) or (V,3,3), dims the map shapes, sizes the image shapes K refers to (None = the maps') -> (V,3,3) for the maps"""
    V = len(dims)
    K = np.broadcast_to(np.asarray(K, np.float64), (V, 3, 3)).copy()
    if sizes is not None:
        for v, ((h, w), (hi, wi)) in enumerate(zip(dims, sizes)):
            K[v, 0] *= w / wi
            K[v, 1] *= h / hi
    return K


def inverse_k(K):
    """closed form of an upper-triangular K, as the kernel"""
    fx, s, cx, fy, cy, w = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2], K[2, 2]
    det = fx * fy * w
    with np.errstate(all="ignore"):
        return np.array([[1.0 / fx, -s / (fx * fy), (s * cy - cx * fy) / det], [0.0, 1.0 / fy, -cy / (fy * w)], [0.0, 0.0, 1.0 / w]])


def usable_view(K, R, t):
    if not (np.isfinite(K).all() and np.isfinite(R).all() and np.isfinite(t).all()):
        return False
    det = K[0, 0] * K[1, 1] * K[2, 2]
    with np.errstate(all="ignore"):
        return bool(K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and det != 0 and np.isfinite(1.0 / det))


def is_depth(d):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def lift(u, v, d, Kinv, R, t):
    """world points of pixels (u, v) at depth d: R^T (K^-1 (u d, v d, d) - t), (N,3)"""
    h = np.stack([u * d, v * d, d], -1)
    return (h @ Kinv.T - t) @ R


def project(X, K, R, t):
    return (X @ R.T + t) @ K.T


def fuse_depth_ref(depths, R, t, K, sizes=None, max_reproj_error=1.0, max_depth_error=0.01, min_views=2, max_points=None):
    depths = [np.asarray(d, np.float32) for d in depths]
    V = len(depths)
    dims = [d.shape for d in depths]
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    K = scaled_intrinsics(K, dims, sizes)
    Kinv = [inverse_k(K[v]) for v in range(V)]
    ok = [usable_view(K[v], R[v], t[v]) for v in range(V)]
    margins = {k: [] for k in ("qz", "tap", "pz", "reproj", "depth", "border")}
    out = {k: [] for k in ("depth64", "depth", "valid", "views", "num_views", "emit", "dup", "owner", "consistent")}
    proj = {}                                                     # (r, s) -> (u_s, v_s) of every pixel of r, NaN where not computed
    with np.errstate(all="ignore"):
        # ---- pass 1
        for r in range(V):
            H, W = dims[r]
            ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            u, v = (jj + 0.5).ravel(), (ii + 0.5).ravel()
            d = depths[r].astype(np.float64).ravel()
            has = is_depth(d) & ok[r]
            seen = np.where(has, np.uint32(1) << np.uint32(r), np.uint32(0)).astype(np.uint32)
            total = np.where(has, d, 0.0)
            cons = np.zeros((V, H * W), bool)
            for s in range(V):
                if s == r or not ok[s] or not ok[r]:
                    continue
                Hs, Ws = dims[s]
                idx = np.flatnonzero(has)
                q = project(lift(u[idx], v[idx], d[idx], Kinv[r], R[r], t[r]), K[s], R[s], t[s])
                margins["qz"].append(np.abs(q[:, 2]))
                front = q[:, 2] > 0
                idx, q = idx[front], q[front]
                us, vs = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
                uv = np.full((2, H * W), np.nan)
                uv[0, idx], uv[1, idx] = us, vs
                proj[r, s] = uv
                ix, iy = us - 0.5, vs - 0.5
                margins["tap"].append(np.minimum(np.minimum(np.abs(ix), np.abs(ix - (Ws - 1))), np.minimum(np.abs(iy), np.abs(iy - (Hs - 1)))))
                inside = (ix >= 0) & (ix < Ws - 1) & (iy >= 0) & (iy < Hs - 1)
                idx, us, vs, ix, iy = idx[inside], us[inside], vs[inside], ix[inside], iy[inside]
                fx, fy = np.floor(ix), np.floor(iy)
                x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
                ds_map = depths[s]
                nw, ne, sw, se = ds_map[y0, x0], ds_map[y0, x0 + 1], ds_map[y0 + 1, x0], ds_map[y0 + 1, x0 + 1]
                full = is_depth(nw) & is_depth(ne) & is_depth(sw) & is_depth(se)
                wx1, wx0, wy1, wy0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
                dsv = (nw.astype(np.float64) * (wx0 * wy0) + ne.astype(np.float64) * (wx1 * wy0) + sw.astype(np.float64) * (wx0 * wy1)
                       + se.astype(np.float64) * (wx1 * wy1))
                idx, us, vs, dsv = idx[full], us[full], vs[full], dsv[full]
                p = project(lift(us, vs, dsv, Kinv[s], R[s], t[s]), K[r], R[r], t[r])
                margins["pz"].append(np.abs(p[:, 2]))
                front = p[:, 2] > 0
                idx, p = idx[front], p[front]
                err = np.hypot(p[:, 0] / p[:, 2] - u[idx], p[:, 1] / p[:, 2] - v[idx])
                rel = np.abs(p[:, 2] - d[idx]) / d[idx]
                margins["reproj"].append(np.abs(err - max_reproj_error))
                margins["depth"].append(np.abs(rel - max_depth_error))
                good = (err < max_reproj_error) & (rel < max_depth_error)
                idx, pz = idx[good], p[good, 2]
                seen[idx] |= np.uint32(1) << np.uint32(s)
                total[idx] += pz                                  # ascending s: the kernel's order of addition
                cons[s, idx] = True
            num = np.array([bin(int(x)).count("1") for x in seen], np.uint8)
            valid = num >= min_views
            d64 = np.where(valid, total / np.maximum(num, 1), 0.0)
            out["depth64"].append(d64.reshape(H, W))
            out["depth"].append(d64.astype(np.float32).reshape(H, W))
            out["valid"].append(valid.reshape(H, W))
            out["views"].append(seen.view(np.int32).reshape(H, W))
            out["num_views"].append(num.reshape(H, W))
            out["consistent"].append(cons.reshape(V, H, W))
        # ---- pass 2
        for r in range(V):
            H, W = dims[r]
            valid = out["valid"][r].ravel()
            seen = out["views"][r].ravel().view(np.uint32)
            dup = np.zeros(H * W, bool)
            owner = np.full((H * W, 3), -1, np.int64)
            for s in range(r - 1, -1, -1):                        # descending, so that the lowest view is the one left in `owner`
                if (r, s) not in proj:
                    continue
                Hs, Ws = dims[s]
                idx = np.flatnonzero(valid & (((seen >> np.uint32(s)) & 1) == 1))
                us, vs = proj[r, s][0, idx], proj[r, s][1, idx]
                margins["border"].append(np.minimum(np.abs(us - np.round(us)), np.abs(vs - np.round(vs))))
                col, row = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
                assert ((col >= 0) & (col < Ws) & (row >= 0) & (row < Hs)).all()          # a consistent view was sampled inside
                hit = out["valid"][s][row, col] & (((out["views"][s][row, col].view(np.uint32) >> np.uint32(r)) & 1) == 1)
                dup[idx[hit]] = True
                owner[idx[hit]] = np.stack([np.full(hit.sum(), s), row[hit], col[hit]], -1)
            out["dup"].append(dup.reshape(H, W))
            out["emit"].append((valid & ~dup).reshape(H, W))
            out["owner"].append(owner.reshape(H, W, 3))
        # ---- pass 3
        pts, view, pixel, pviews = [], [], [], []
        for r in range(V):
            H, W = dims[r]
            n = np.flatnonzero(out["emit"][r].ravel())
            i, j = n // W, n % W
            d = out["depth"][r].ravel()[n].astype(np.float64)     # the fused depth as it is stored
            ray = np.stack([j + 0.5, i + 0.5, np.ones(len(n))], -1) @ Kinv[r].T
            pts.append((ray * d[:, None] - t[r]) @ R[r])
            view.append(np.full(len(n), r, np.uint8))
            pixel.append(n.astype(np.int32))
            pviews.append(out["views"][r].ravel()[n])
    pts, view, pixel, pviews = np.concatenate(pts), np.concatenate(view), np.concatenate(pixel), np.concatenate(pviews)
    emitted = len(pixel)
    if max_points is not None:
        T, k = int(max_points), min(emitted, int(max_points))
        pad = lambda a, fill: np.concatenate([a[:k], np.full((T - k,) + a.shape[1:], fill, a.dtype)])
        pts, view, pixel, pviews = pad(pts, 0.0), pad(view, 0), pad(pixel, -1), pad(pviews, 0)
    with np.errstate(all="ignore"):
        pts32 = pts.astype(np.float32)
    out.update(points64=pts, points=pts32, view=view, pixel=pixel, point_views=pviews,
               counts=np.array([emitted, sum(int(v.sum()) for v in out["valid"]), sum(int(d.sum()) for d in out["dup"]), 0], np.int32),
               margins={k: (np.concatenate(v) if v else np.zeros(0)) for k, v in margins.items()})
    return out
