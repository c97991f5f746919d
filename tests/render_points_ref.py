"""numpy fp64 restatement of roma_render_points (include/roma_hip.h, roma_amd/csrc/render_points.hip) by the plain chain q = K_v (R_v X
+ t_v) — not by the kernel's P_v = K_v [R_v | t_v] —, the splat as one np.minimum.at of 64-bit keys per footprint offset, and for every
decision its distance to the threshold.

render_points_ref(points, R, t, K, shape, ...) -> dict
  depth (V,H,W) fp32, index (V,H,W) int32, visible (N) int32, num_views (N) uint8, counts (4) int32: the outputs
  live (N) bool, usable (V) bool; inside (V,N) bool, row, col (V,N) int64 (-1 where not inside), z32 (V,N) fp32, z64 (V,N): the projections
  margins: {name: 1-D array}
    "qz"      |q.z| of every finite projection of a live point into a usable view
    "border"  the distance of (u, w) to the nearest pixel border — the map's edges are borders too — for every projection in front of
              its view that lies inside the map or less than a pixel outside it
    "order"   for every candidate of a pixel whose fp32 depth is less than 3 ulps behind the winner's (so that a device depth that rounds
              the other way could change the winner): the distance, in fp32 ulps, of its fp64 depth and of the winner's to the nearest
              point at which the rounding to fp32 changes.  The device's fp64 depth differs from the plain chain's by some 1e-8 ulp.
              Candidates at exactly the winner's fp64 depth are left out: they tie by construction and the lowest index wins
    "visible" | z32 / (depth (1 + depth_tol)) - 1 | of every visibility decision
"""
from __future__ import annotations

import numpy as np

from tests.fuse_depth_ref import usable_view

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def scaled_intrinsics(K, V, shape, sizes):
    """K (3,3) or (V,3,3) for images of sizes[v] = (H_img, W_img) (None = the maps' shape) -> (V,3,3) for maps of `shape`"""
    K = np.broadcast_to(np.asarray(K, np.float64), (V, 3, 3)).copy()
    if sizes is not None:
        for v, (hi, wi) in enumerate(sizes):
            K[v, 0] *= shape[1] / wi
            K[v, 1] *= shape[0] / hi
    return K


def _bits(z):
    """the bit patterns of positive fp64 depths rounded to fp32, as integers: they order as the depths do"""
    return z.astype(np.float32).view(np.uint32).astype(np.int64)


def _rounding_margin(z):
    """the distance of positive fp64 depths to the nearest point at which their rounding to fp32 changes, in fp32 ulps"""
    f = z.astype(np.float32)
    lo, hi = np.nextafter(f, np.float32(0)).astype(np.float64), np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return np.minimum(np.abs(z - 0.5 * (f + lo)), np.abs(z - 0.5 * (f + hi))) / (hi - f)


def render_points_ref(points, R, t, K, shape, sizes=None, radius=0, depth_tol=0.05, mask=None):
    X32 = np.asarray(points, np.float32)
    N, (H, W) = len(X32), shape
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    if R.ndim == 2:
        R, t = R[None], t[None]
    V = len(R)
    K = scaled_intrinsics(K, V, shape, sizes)
    usable = np.array([usable_view(K[v], R[v], t[v]) for v in range(V)])
    live = np.isfinite(X32).all(1) & (np.ones(N, bool) if mask is None else np.asarray(mask) != 0)
    X = X32.astype(np.float64)
    n_all = np.arange(N, dtype=np.uint64)
    keys = np.full((V, H, W), EMPTY, np.uint64)
    inside = np.zeros((V, N), bool)
    row, col = np.full((V, N), -1, np.int64), np.full((V, N), -1, np.int64)
    z32, z64 = np.zeros((V, N), np.float32), np.zeros((V, N))
    margins = {k: [] for k in ("qz", "border", "order", "visible")}
    with np.errstate(all="ignore"):
        for v in np.flatnonzero(usable):
            q = (X @ R[v].T + t[v]) @ K[v].T
            fin = live & np.isfinite(q).all(1)
            margins["qz"].append(np.abs(q[fin, 2]))
            front = fin & (q[:, 2] > 0)
            iz = 1.0 / q[:, 2]
            u, w = q[:, 0] * iz, q[:, 1] * iz
            near = front & (u > -1) & (u < W + 1) & (w > -1) & (w < H + 1)
            margins["border"].append(np.minimum(np.abs(u[near] - np.round(u[near])), np.abs(w[near] - np.round(w[near]))))
            zf = q[:, 2].astype(np.float32)
            ok = front & (u >= 0) & (u < W) & (w >= 0) & (w < H) & np.isfinite(zf) & (zf > 0)
            idx = np.flatnonzero(ok)
            inside[v, idx] = True
            col[v, idx], row[v, idx] = np.floor(u[idx]).astype(np.int64), np.floor(w[idx]).astype(np.int64)
            z32[v, idx], z64[v, idx] = zf[idx], q[idx, 2]
            key = (zf[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | n_all[idx]
            cand_pix, cand_z = [], []
            for di in range(-radius, radius + 1):
                for dj in range(-radius, radius + 1):
                    ii, jj = row[v, idx] + di, col[v, idx] + dj
                    on = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                    np.minimum.at(keys[v], (ii[on], jj[on]), key[on])
                    cand_pix.append(ii[on] * W + jj[on])
                    cand_z.append(q[idx[on], 2])
            if len(idx):
                pix, zz = np.concatenate(cand_pix), np.concatenate(cand_z)
                o = np.lexsort((zz, pix))
                pix, zz = pix[o], zz[o]
                first = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
                z1 = np.repeat(zz[first], np.diff(np.r_[first, len(pix)]))      # the winner's fp64 depth, per candidate
                close = (zz != z1) & (_bits(zz) - _bits(z1) < 3)
                margins["order"].append(np.minimum(_rounding_margin(zz[close]), _rounding_margin(z1[close])))
        covered = keys != EMPTY
        depth = np.where(covered, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
        index = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        visible = np.zeros(N, np.uint32)
        for v in np.flatnonzero(usable):
            idx = np.flatnonzero(inside[v])
            limit = depth[v, row[v, idx], col[v, idx]].astype(np.float64) * (1.0 + depth_tol)
            zd = z32[v, idx].astype(np.float64)
            margins["visible"].append(np.abs(zd / limit - 1.0))
            visible[idx[zd <= limit]] |= np.uint32(1) << np.uint32(v)
    num = np.array([bin(int(b)).count("1") for b in visible], np.uint8)
    counts = np.array([inside.sum(), covered.sum(), num.sum(dtype=np.int64), (~live).sum()], np.int64).astype(np.int32)
    return {"depth": depth.astype(np.float32), "index": index, "visible": visible.view(np.int32), "num_views": num, "counts": counts,
            "live": live, "usable": usable, "inside": inside, "row": row, "col": col, "z32": z32, "z64": z64,
            "margins": {k: (np.concatenate(m) if m else np.zeros(0)) for k, m in margins.items()}}
