#!/usr/bin/env python3
"""Generate tests/golden/fb_consistency.npz by RUNNING THE REFERENCE's RegressionMatcher.conf_from_fb_consistency on the CPU.

    python tests/golden/make_golden_fb.py

Input (H = 24, W = 32, th = 2, so th_n = 0.125): the forward flow is an affine map of the pixel grid, the backward flow its exact
inverse plus a ramp in x that grows from 0 to 5 px from the left to the right edge — bilinear sampling reproduces an affine map, so
the round trip misses by the ramp and the mask flips where it passes 2 px.  `ff_base` is that input; `ff` is the same with a few
forward positions pushed outside [-1, 1] (beyond the border, and into the half-pixel band where zero padding blends in), which pins
zero padding: two of them sit at the image centre, where the (0, 0) that zero padding returns is consistent and a border value is not.
Stored: the inputs, the reference's masks for both (unbatched call -> (H,W)), its mask for the stack [ff, ff_base] (batched call ->
(2,H,W)), and the round-trip distance per pixel (recomputed here with torch on the CPU and checked against the reference's masks)
that the tests use to excuse pixels on the threshold.  Like make_golden.py this is not imported by any test."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from make_golden import import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, TH = 24, 32, 2
A = np.array([[0.90, 0.05], [-0.04, 0.92]])
B = np.array([0.02, -0.03])
OUTSIDE = [((2, 3), (1.30, 0.10)), ((5, 30), (-1.20, -0.40)), ((11, 7), (0.20, 1.25)), ((17, 20), (-0.30, -1.50)),
           ((20, 12), (0.99, 0.50)), ((8, 25), (-0.985, 0.97)), ((22, 1), (1.02, -1.01)),
           ((12, 16), (1.40, 0.00)), ((11, 15), (-0.20, -1.30))]      # the last two: zero padding returns (0, 0), next to these pixels


def grid():
    x, y = np.meshgrid(np.linspace(-1 + 1 / W, 1 - 1 / W, W), np.linspace(-1 + 1 / H, 1 - 1 / H, H), indexing="xy")
    return np.stack([x, y], -1)


def flows():
    g = grid()
    ff = g @ A.T + B
    ramp = (g[..., 0] - g[0, 0, 0]) / (g[0, -1, 0] - g[0, 0, 0]) * 5 * (2 / W)          # 0 .. 5 px in normalised x units, per column
    fb = (g - B) @ np.linalg.inv(A).T
    fb[..., 0] += ramp
    ff_out = ff.copy()
    for (r, c), v in OUTSIDE:
        ff_out[r, c] = v
    return ff.astype(np.float32), ff_out.astype(np.float32), fb.astype(np.float32)


def distance(ff, fb):
    """the round-trip distance per pixel: the backward flow sampled where the forward flow points, against the pixel grid"""
    back = F.grid_sample(torch.from_numpy(fb).permute(2, 0, 1)[None], torch.from_numpy(ff)[None], mode="bilinear", padding_mode="zeros",
                         align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.linalg.norm(grid().astype(np.float32) - back, axis=-1)


def main():
    romatch = import_reference()
    from romatch.models.matcher import RegressionMatcher
    fn = RegressionMatcher.conf_from_fb_consistency                        # the method does not use self
    ff_base, ff, fb = flows()
    th_n = 2 * TH / max(H, W)
    out = {"ff_base": ff_base, "ff": ff, "fb": fb, "th": np.int64(TH)}
    for name, f in (("base", ff_base), ("out", ff)):
        mask = fn(None, torch.from_numpy(f), torch.from_numpy(fb), th=TH)
        assert mask.shape == (H, W) and mask.dtype == torch.float32
        dist = distance(f, fb)
        assert np.array_equal(dist < th_n, mask.numpy() > 0)
        margin = np.abs(dist - th_n).min() / th_n
        print(f"{name}: {mask.mean():.4f} of the pixels consistent; the closest distance is {margin:.3e} th_n from the threshold")
        out["mask_" + name], out["dist_" + name] = mask.numpy(), dist
    both = fn(None, torch.from_numpy(np.stack([ff, ff_base])), torch.from_numpy(np.stack([fb, fb])), th=TH)
    assert both.shape == (2, H, W)
    out["mask_batched"] = both.numpy()
    changed = out["mask_out"] != out["mask_base"]
    print(f"{int(changed.sum())} pixels change with the outside positions")
    path = os.path.join(HERE, "fb_consistency.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
