"""numpy restatement of the MAGSAC++ scoring of roma_amd.geometry (csrc/ransac_common.h): the closed forms of the loss
L and the weight W, their 1 025-node tables, the piecewise-linear interpolants in fp64, and the whole RANSAC for F, H and E with
either scoring — the hypotheses, errors, refit and projections are those of tests/geometry_ref.py and tests/pose_ref.py; only the
cost of a model and the weights of the refit differ.  With scoring = "msac" `ransac` / `ransac_essential` restate G.ransac /
PR.ransac_essential (tests/test_magsac.py checks that they agree), so one set of hypotheses serves both scorings of a scene."""
from __future__ import annotations

import math

import numpy as np

from tests import geometry_ref as G
from tests import pose_ref as PR

K_SIGMA = 3.64                         # sigma_max = threshold / k; n = 4 degrees of freedom
CELLS = 1024
XK = K_SIGMA * K_SIGMA / 2.0


def upper_gamma_15(x):
    r = math.sqrt(x)
    return 0.5 * math.sqrt(math.pi) * math.erfc(r) + r * math.exp(-x)


def lower_gamma_25(x):
    r = math.sqrt(x)
    return 0.75 * math.sqrt(math.pi) * math.erf(r) - math.exp(-x) * r * (x + 1.5)


def loss_closed(u):
    """L(u), u = e / threshold^2 in [0, 1]: the MAGSAC++ loss over its value at the threshold"""
    x = u * XK
    return (lower_gamma_25(x) + x * (upper_gamma_15(x) - upper_gamma_15(XK))) / lower_gamma_25(XK)


def weight_closed(u):
    x = u * XK
    return (upper_gamma_15(x) - upper_gamma_15(XK)) / (upper_gamma_15(0.0) - upper_gamma_15(XK))


def tables():
    """(loss nodes, weight nodes) at u_j = j / 1024: fp64 closed forms rounded to fp32, returned as fp64"""
    u = [j / CELLS for j in range(CELLS + 1)]
    return (np.array([loss_closed(v) for v in u]).astype(np.float32).astype(np.float64),
            np.array([weight_closed(v) for v in u]).astype(np.float32).astype(np.float64))


LOSS_NODES, WEIGHT_NODES = tables()


def interpolate(nodes, e, t2, beyond):
    """the interpolant at u = e / t2 where e < t2, `beyond` elsewhere (NaN included)"""
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inl = e < t2
    f = np.where(inl, e, 0.0) / t2 * CELLS
    i = np.minimum(f.astype(np.int64), CELLS - 1)
    v = nodes[i] + (f - i) * (nodes[i + 1] - nodes[i])
    return np.where(inl, v, beyond)


def loss(e, t2):
    return interpolate(LOSS_NODES, e, t2, 1.0)


def weight(e, t2):
    return interpolate(WEIGHT_NODES, e, t2, 0.0)


def cost(e, t2, scoring="magsac"):
    """cost of a model from its squared errors (..., N): threshold^2 * sum L, or the MSAC cost"""
    if scoring == "magsac":
        return t2 * loss(e, t2).sum(-1)
    with np.errstate(invalid="ignore"):
        return np.where(e < t2, e, t2).sum(-1)


def _weights(e, t2, scoring):
    with np.errstate(invalid="ignore"):
        return weight(e, t2) if scoring == "magsac" else (e < t2).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ F and H
def hypotheses(model, xa, xb, iters, seed):
    """what G.ransac does before it scores: (slot-ordered normalised models, xh, xh2, T_A, T_B)"""
    ok = G.usable(xa, xb)
    cA, cB = G.normalisation(xa, ok), G.normalisation(xb, ok)
    xh, xh2 = (xa - cA[:2]) * cA[2], (xb - cB[:2]) * cB[2]
    idx = G.minimal_samples(xa[None], xb[None], model, iters, seed)[0]
    cands = []
    for h in range(iters):
        if idx[h, 0] < 0:
            continue
        s = idx[h]
        if model == "fundamental":
            cands += G.seven_point(xh[s], xh2[s])[0]
        elif not (G.collinear(xh[s]) or G.collinear(xh2[s])):
            cands.append(G.four_point(xh[s], xh2[s])[0])
    return cands, xh, xh2, G.transform(cA), G.transform(cB)


def ransac(model, xa, xb, threshold, iters, seed, lo_iters=3, scoring="magsac", hyp=None):
    """One pair (N,2) -> (model (3,3) in pixels, inlier mask), fp64.  G.ransac with the cost and the refit weights of `scoring`."""
    N = xa.shape[0]
    cands, xh, xh2, TA, TB = hyp if hyp is not None else hypotheses(model, xa, xb, iters, seed)
    if not cands:
        return np.zeros((3, 3)), np.zeros(N, dtype=bool)
    t2 = threshold ** 2
    e = G.errors(model, np.stack([G.denormalise(model, m, TA, TB) for m in cands]), xa, xb)
    c = cost(e, t2, scoring)
    best = int(np.argmin(c))
    cur, cc, ce = cands[best], c[best], e[best]
    rows_of = G.f_rows if model == "fundamental" else G.h_rows
    for _ in range(lo_iters):
        with np.errstate(invalid="ignore"):
            if (ce < t2).sum() < (8 if model == "fundamental" else 4):
                break
        w = _weights(ce, t2, scoring)
        i = np.nonzero(w > 0)[0] if scoring == "magsac" else np.nonzero(w)[0]
        rows = rows_of(xh[i, 0], xh[i, 1], xh2[i, 0], xh2[i, 1]).reshape(-1, 9)
        wr = w[i] if model == "fundamental" else np.concatenate([w[i], w[i]])       # both rows of a match share its weight
        cand = np.linalg.eigh(rows.T @ (rows * wr[:, None]))[1][:, 0].reshape(3, 3)
        if model == "fundamental":
            U, S, Vt = np.linalg.svd(cand)
            cand = U @ np.diag([S[0], S[1], 0.0]) @ Vt
        cand = G.unit(cand)
        e2 = G.errors(model, G.denormalise(model, cand, TA, TB), xa, xb)
        c2 = cost(e2, t2, scoring)
        if not c2 < cc:
            break
        cur, cc, ce = cand, c2, e2
    M = G.finish(model, G.denormalise(model, cur, TA, TB))
    with np.errstate(invalid="ignore"):
        return M, G.errors(model, M, xa, xb) < t2


# ------------------------------------------------------------------------------------------------------------------- E
def hypotheses_essential(xa, xb, KA, KB, iters, seed):
    xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    idx = PR.minimal_samples(xa[None], xb[None], iters, seed)[0]
    cands = []
    for h in range(iters):
        if idx[h, 0] >= 0:
            cands += PR.five_point(xh[idx[h]], xh2[idx[h]])[0]
    return cands, xh, xh2


def ransac_essential(xa, xb, KA, KB, threshold, iters, seed, lo_iters=3, scoring="magsac", hyp=None):
    """One pair -> (E unit norm, sign-fixed, calibrated coordinates; inlier mask).  PR.ransac_essential with the cost and weights of `scoring`."""
    N = xa.shape[0]
    cands, xh, xh2 = hyp if hyp is not None else hypotheses_essential(xa, xb, KA, KB, iters, seed)
    if not cands:
        return np.zeros((3, 3)), np.zeros(N, dtype=bool)
    t2 = threshold ** 2
    e = G.errors("fundamental", np.stack(cands), xh, xh2)
    c = cost(e, t2, scoring)
    best = int(np.argmin(c))
    cur, cc, ce = cands[best], c[best], e[best]
    for _ in range(lo_iters):
        with np.errstate(invalid="ignore"):
            if (ce < t2).sum() < 8:
                break
        w = _weights(ce, t2, scoring)
        i = np.nonzero(w > 0)[0] if scoring == "magsac" else np.nonzero(w)[0]
        rows = G.f_rows(xh[i, 0], xh[i, 1], xh2[i, 0], xh2[i, 1])
        cand = PR.project_essential(np.linalg.eigh(rows.T @ (rows * w[i, None]))[1][:, 0].reshape(3, 3))
        e2 = G.errors("fundamental", cand, xh, xh2)
        c2 = cost(e2, t2, scoring)
        if not c2 < cc:
            break
        cur, cc, ce = cand, c2, e2
    E = G.sign_fixed(PR.project_essential(cur))
    with np.errstate(invalid="ignore"):
        return E, G.errors("fundamental", E, xh, xh2) < t2


# -------------------------------------------------------------------------------- the accuracy cases of DESIGN.md §3.4
SCENES = {"F": (11, 12, 13, 14, 15, 16), "H": (1, 2, 3, 4, 5, 6), "E": (11, 12, 13, 14, 15, 16)}
CASES = {                              # row -> (threshold, samples, seed), N = 2000
    "F": (6.0, 300, 3),
    "H": (25.0, 300, 4),
    "E": (6.0 / 800, 200, 5),
}
TIGHT = {"F": 1.5, "H": 3.0, "E": 1.5 / 800}


def case_scene(row, scene, N=2000):
    """(xa, xb, the scene's truth for `criteria`)"""
    if row == "H":
        xa, xb, _, H = G.planar_scene(scene, N=N)
        return xa, xb, H
    xa, xb, truth, _, ca, cb = G.two_view_scene(scene, N=N)
    return xa, xb, ((ca[truth], cb[truth]) if row == "F" else scene)


def criteria(row, M, mask, xa, xb, truth):
    """F: (median Sampson distance of the clean true inliers, px,); H: (corner error, px,); E: (rotation, translation error, deg)"""
    if row == "F":
        return (float(np.median(np.sqrt(G.errors("fundamental", M, truth[0], truth[1])))),)
    if row == "H":
        return (G.corner_error(M, truth),)
    K, R_true, t_true = PR.scene_pose(truth)
    R, t = PR.recover_pose(M, xa, xb, K, K, mask)[:2]
    return PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)
