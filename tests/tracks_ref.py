"""numpy restatement of roma_amd.geometry.build_tracks (csrc/tracks.hip), step for step; tests/test_tracks.py compares every output of
the kernels with it for equality.

Cells: view v has Hc_v = ceil(H_v / cell) by Wc_v = ceil(W_v / cell) cells with global ids base_v + cy * Wc_v + cx.  Endpoints: px =
(x + 1.0f) * (0.5f * W_v) in fp32, cell (floor(px * inv), floor(py * inv)) with inv = 1.0f / cell; inside when 0 <= px < W_v, 0 <= py
< H_v and the cell exists.  A match is usable when both endpoints are inside, its certainty is finite and above the threshold, its
mask is set and its two views are different views in [0, V).  A cell with a usable endpoint is a node, represented by the endpoint of
the highest certainty (the lowest endpoint index e = (m k + j) 2 + side on a tie); usable matches are edges; a component is labelled
by its lowest node, conflicts when two of its nodes share a view, qualifies otherwise with at least min_views views; qualifying
components take rows 0, 1, ... in label order, rows >= max_tracks are dropped."""
from __future__ import annotations

import numpy as np

F = np.float32


def grid(sizes, cell):
    """sizes: V pairs (H, W) -> base (V+1), Wc (V), Hc (V) as int64"""
    H = np.array([s[0] for s in sizes], np.int64)
    W = np.array([s[1] for s in sizes], np.int64)
    Hc, Wc = -(-H // cell), -(-W // cell)
    return np.concatenate([[0], np.cumsum(Hc * Wc)]), Wc, Hc


def endpoints(xy, view, sizes, cell):
    """xy (...,2) float32 normalised, view (...) int in [0, V) -> px, py float32, inside bool, global cell id int64 (-1 outside)"""
    base, Wc, Hc = grid(sizes, cell)
    Wf = np.array([s[1] for s in sizes], F)
    Hf = np.array([s[0] for s in sizes], F)
    inv = F(1.0) / F(cell)
    xy = np.asarray(xy, F)
    with np.errstate(invalid="ignore", over="ignore"):
        px = (xy[..., 0] + F(1.0)) * (F(0.5) * Wf)[view]
        py = (xy[..., 1] + F(1.0)) * (F(0.5) * Hf)[view]
        inside = (px >= 0) & (px < Wf[view]) & (py >= 0) & (py < Hf[view])
        cx = np.where(inside, np.floor(px * inv), 0).astype(np.int64)
        cy = np.where(inside, np.floor(py * inv), 0).astype(np.int64)
    inside &= (cx < Wc[view]) & (cy < Hc[view])
    return px, py, inside, np.where(inside, base[view] + cy * Wc[view] + cx, -1)


def build_tracks_ref(matches, certainty, pairs, sizes, *, cell=4, certainty_thresh=0.0, mask=None, min_views=2, max_tracks):
    """-> dict of x (V,T,2) float32, visible (V,T) bool, views (T) int32, num_views (T) uint8, track_of_match (M,k) int32,
    counts (4) int32 (the status word is 0: nothing here can give up)"""
    matches, certainty = np.asarray(matches, F), np.asarray(certainty, F)
    pairs = np.asarray(pairs, np.int64)
    M, k = certainty.shape
    V, T = len(sizes), int(max_tracks)
    base, _, _ = grid(sizes, cell)
    C = int(base[-1])
    a, b = pairs[:, 0], pairs[:, 1]
    pair_ok = (a >= 0) & (a < V) & (b >= 0) & (b < V) & (a != b)
    va = np.broadcast_to(np.where(pair_ok, a, 0)[:, None], (M, k))
    vb = np.broadcast_to(np.where(pair_ok, b, 0)[:, None], (M, k))
    pxa, pya, ina, ca = endpoints(matches[..., 0:2], va, sizes, cell)
    pxb, pyb, inb, cb = endpoints(matches[..., 2:4], vb, sizes, cell)
    with np.errstate(invalid="ignore"):
        usable = pair_ok[:, None] & ina & inb & np.isfinite(certainty) & (certainty > F(certainty_thresh))
    if mask is not None:
        usable &= np.asarray(mask).reshape(M, k) != 0

    # the representative of every node: the highest (certainty bits, 0xFFFFFFFF - endpoint index)
    cells = np.stack([ca, cb], -1).reshape(-1)                      # flat endpoint index e = (m k + j) 2 + side
    px, py = np.stack([pxa, pxb], -1).reshape(-1), np.stack([pya, pyb], -1).reshape(-1)
    view = np.stack([va, vb], -1).reshape(-1)
    live = np.repeat(usable.reshape(-1), 2)
    e = np.arange(2 * M * k, dtype=np.uint64)
    bits = np.repeat(certainty.reshape(-1).view(np.uint32).astype(np.uint64), 2)
    keys = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - e)
    best = np.zeros(C, np.uint64)
    np.maximum.at(best, cells[live], keys[live])
    nodes = np.flatnonzero(best)
    rep = (np.uint64(0xFFFFFFFF) - (best[nodes] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    node_view = np.searchsorted(base, nodes, side="right") - 1

    # components: union-find, the larger root under the smaller, so a root is its component's lowest node
    parent = {int(n): int(n) for n in nodes}

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    ua, ub = ca[usable], cb[usable]
    for p, q in zip(ua.tolist(), ub.tolist()):
        p, q = find(p), find(q)
        if p != q:
            parent[max(p, q)] = min(p, q)
    root = np.array([find(int(n)) for n in nodes], np.int64)

    # per component
    labels, comp = np.unique(root, return_inverse=True)             # ascending label
    seen = np.zeros(len(labels), np.int64)
    np.bitwise_or.at(seen, comp, np.int64(1) << node_view)
    n_nodes = np.bincount(comp, minlength=len(labels))
    n_views = np.array([bin(int(s)).count("1") for s in seen], np.int64)
    conflicting = n_nodes > n_views
    too_short = ~conflicting & (n_views < min_views)
    qualifies = ~conflicting & ~too_short
    row = np.where(qualifies, np.cumsum(qualifies) - 1, -1)
    row[row >= T] = -1

    x = np.full((V, T, 2), np.nan, F)
    visible = np.zeros((V, T), bool)
    views = np.zeros(T, np.int64)
    r = row[comp]
    keep = r >= 0
    x[node_view[keep], r[keep], 0] = px[rep[keep]]
    x[node_view[keep], r[keep], 1] = py[rep[keep]]
    visible[node_view[keep], r[keep]] = True
    views[row[row >= 0]] = seen[row >= 0]
    row_of_cell = np.full(C + 1, -1, np.int64)                     # the extra slot takes the -1 of unusable matches
    row_of_cell[nodes] = r
    track_of_match = np.where(usable, row_of_cell[ca], -1).astype(np.int32)
    counts = np.array([qualifies.sum(), conflicting.sum(), too_short.sum(), 0], np.int32)
    num_views = np.array([bin(int(s)).count("1") for s in views], np.uint8)
    return {"x": x, "visible": visible, "views": (views & 0xFFFFFFFF).astype(np.uint32).view(np.int32), "num_views": num_views,
            "track_of_match": track_of_match, "counts": counts}
