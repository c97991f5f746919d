"""The argument path that recover_pose, refine_pose, refine_fundamental, refine_homography and triangulate share in
roma_amd.geometry: what a wrapper hands to its kernel does not depend on how the caller holds the points and the mask.  Contiguous
fp64 points and a contiguous bool mask against non-contiguous fp32 views of a (P,N,4) match tensor and a uint8 column of a (P,N,2)
tensor, the same values in both: every returned tensor is bit for bit the same, and a single pair is its row of the batch.
The models come from the host RANSAC of tests/geometry_ref.py and tests/pose_ref.py, so no device estimator is involved."""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_ref as G
from tests import pose_ref as PR
from tests.helpers import dev

P, N, SEEDS = 3, 64, (11, 12, 13)
SAMPLES = 100
THR = 1.5                                                    # pixels; THR / 800 in calibrated units
CALLS = ("recover_pose", "refine_pose", "refine_fundamental", "refine_homography", "triangulate")


@functools.lru_cache(maxsize=None)
def _inputs(planar):
    """-> (x_A, x_B (P,N,2) fp64 holding fp32 values, models): the scenes rounded to fp32 once and their host RANSAC models"""
    scenes = [(G.planar_scene if planar else G.two_view_scene)(seed, N=N)[:2] for seed in SEEDS]
    xa = np.stack([s[0] for s in scenes]).astype(np.float32).astype(np.float64)
    xb = np.stack([s[1] for s in scenes]).astype(np.float32).astype(np.float64)
    K = PR.K_SCENE
    if planar:
        fits = [G.ransac("homography", xa[i], xb[i], THR, SAMPLES, seed=s) for i, s in enumerate(SEEDS)]
        return xa, xb, {"H": np.stack([f[0] for f in fits]), "mask_H": np.stack([f[1] for f in fits])}
    fits = [G.ransac("fundamental", xa[i], xb[i], THR, SAMPLES, seed=s) for i, s in enumerate(SEEDS)]
    ess = [PR.ransac_essential(xa[i], xb[i], K, K, THR / 800, SAMPLES, seed=s) for i, s in enumerate(SEEDS)]
    poses = [PR.recover_pose(e[0], xa[i], xb[i], K, K, e[1]) for i, e in enumerate(ess)]
    return xa, xb, {"F": np.stack([f[0] for f in fits]), "mask_F": np.stack([f[1] for f in fits]),
                    "E": np.stack([e[0] for e in ess]), "mask_E": np.stack([e[1] for e in ess]),
                    "R": np.stack([p[0] for p in poses]), "t": np.stack([p[1] for p in poses]),
                    "mask_pose": np.stack([p[2] for p in poses])}


def _call(name, xa, xb, mask, models, i=None):
    """the wrapper `name` on the whole batch, or on pair i alone (the points and the mask then come 2-D / 1-D)"""
    from roma_amd import geometry
    K = PR.K_SCENE
    M = {k: dev(v if i is None else v[i]) for k, v in models.items() if not k.startswith("mask")}
    if name == "recover_pose":
        return geometry.recover_pose(M["E"], xa, xb, K, K, mask)
    if name == "refine_pose":
        return geometry.refine_pose(M["R"], M["t"], xa, xb, K, K, THR / 800, mask=mask, return_info=True)
    if name == "refine_fundamental":
        return geometry.refine_fundamental(M["F"], xa, xb, THR, mask=mask, return_info=True)
    if name == "refine_homography":
        return geometry.refine_homography(M["H"], xa, xb, THR, mask=mask, return_info=True)
    return geometry.triangulate(xa, xb, M["R"], M["t"], K, K, mask=mask)


def _tensors(out):
    """every tensor a wrapper returned, in a fixed order: tuple entries, the values of the info dict, the fields of a Triangulation"""
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        return [out[k] for k in sorted(out)]
    if isinstance(out, tuple):
        return [t for o in out for t in _tensors(o)]
    return [getattr(out, k) for k in out.__slots__]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CALLS)
def test_points_and_mask_are_coerced_alike_however_they_are_held(name):
    xa, xb, models = _inputs(name == "refine_homography")
    truth = models[{"recover_pose": "mask_E", "refine_pose": "mask_pose", "refine_fundamental": "mask_F",
                    "refine_homography": "mask_H", "triangulate": "mask_pose"}[name]]
    assert truth.shape == (P, N) and 0 < truth.sum() < truth.size          # a mask that says something
    # (a) contiguous fp64 points, contiguous bool mask
    a64, b64, mask_a = dev(xa), dev(xb), dev(truth)
    assert a64.dtype == torch.float64 and a64.is_contiguous() and mask_a.dtype == torch.bool
    # (b) the two halves of one (P,N,4) fp32 tensor, and column 0 of a (P,N,2) uint8 tensor whose other column says the opposite
    m = dev(np.concatenate([xa, xb], -1).astype(np.float32))
    a32, b32 = m[..., :2], m[..., 2:]
    cols = dev(np.stack([truth, ~truth], -1).astype(np.uint8))
    mask_b = cols[..., 0]
    assert not a32.is_contiguous() and not b32.is_contiguous() and not mask_b.is_contiguous() and mask_b.dtype == torch.uint8
    assert torch.equal(a32.double(), a64) and torch.equal(b32.double(), b64) and torch.equal(mask_b != 0, mask_a)
    out_a = _tensors(_call(name, a64, b64, mask_a, models))
    out_b = _tensors(_call(name, a32, b32, mask_b, models))
    assert len(out_a) == len(out_b) >= 3
    for ta, tb in zip(out_a, out_b):
        assert ta.shape[0] == P and ta.dtype == tb.dtype and torch.equal(ta, tb), (name, ta.dtype, tuple(ta.shape))
    # pair 0 alone, 2-D points and a 1-D mask, is row 0 of the batch
    for single in (_call(name, a64[0], b64[0], mask_a[0], models, 0), _call(name, a32[0], b32[0], mask_b[0], models, 0)):
        single = _tensors(single)
        assert len(single) == len(out_a)
        for ts, ta in zip(single, out_a):
            assert ts.shape == ta.shape[1:] and torch.equal(ts, ta[0]), (name, ts.dtype, tuple(ts.shape))
