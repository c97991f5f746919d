#!/usr/bin/env python3
"""Generate tests/golden/depth_warp.npz by RUNNING THE REFERENCE's warp_kpts, get_gt_warp (romatch/utils/utils.py) and
MegadepthDenseBenchmark.geometric_dist (romatch/benchmarks/megadepth_dense_benchmark.py) on the CPU.

    python tests/golden/make_golden_depth_warp.py

Three pairs of the scene of tests/depth_warp_ref.py (23 x 37 -> 29 x 31), each with its own cameras, pose and seed.  Stored: the
inputs; the reference's warp_kpts (valid, x2, relative depth error) for "bilinear" and "nearest" on the jittered key-points;
get_gt_warp; and geometric_dist on a predicted warp = its ground truth + N(0, 2 px) noise (gd per pair, the three PCK of the
batch, prob).  The reference is called as its own callers call it: fp32 tensors, .double() at the call.

The script asserts the margins the tests rely on, so that no decision of the recorded results sits within rounding of its
threshold — if a seed violates one, pick another:
  |rel - threshold| > 1e-6;  distance to a covisibility border > 1e-6 px;  |gd - {1, 3, 5}| > 1e-6 px;  every recorded |x2| <= 20.
A key-point in a hole of depth_A (d = 0) projects t alone, and one at the border, where zero padding leaves a fraction of the depth,
nearly so: with this pose |x2| is about 13 there whatever the seed, so the bound on |x2| is 20, and the tests compare every finite x2,
those included, relative to its size.  Like make_golden.py this is not imported by any test."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

from make_golden import REF, import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import depth_warp_ref as D  # noqa: E402

SEEDS = (11, 12, 13)
HA, WA, HB, WB = 23, 37, 29, 31
THRESHOLD = 0.05


def load_benchmark():
    """megadepth_dense_benchmark.py as a module of its own: the package's __init__ imports every benchmark, and those import
    packages that are absent here.  Its own imports reach tqdm and romatch.datasets, which only benchmark() and __init__ use: an
    empty stand-in for each that does not import; geometric_dist itself runs unchanged."""
    for name in ("tqdm", "romatch.datasets"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].MegadepthBuilder = None
    spec = importlib.util.spec_from_file_location("megadepth_dense_benchmark", os.path.join(REF, "romatch", "benchmarks", "megadepth_dense_benchmark.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import_reference()
    from romatch.utils.utils import get_gt_warp, warp_kpts
    geometric_dist = load_benchmark().MegadepthDenseBenchmark.geometric_dist    # the method does not use self
    pairs = [D.scene(seed, HA, WA, HB, WB, variant=i) for i, seed in enumerate(SEEDS)]
    stack = lambda k: np.stack([p[k] for p in pairs])  # noqa: E731
    out = {k: stack(k) for k in ("depth_A", "depth_B", "K_A", "K_B", "T", "kpts")}
    out["seeds"] = np.array(SEEDS)
    t = {k: torch.from_numpy(v) for k, v in out.items()}
    args = (t["depth_A"].double(), t["depth_B"].double(), t["T"].double(), t["K_A"].double(), t["K_B"].double())

    for mode in ("bilinear", "nearest"):
        valid, x2 = warp_kpts(t["kpts"].double(), *args, depth_interpolation_mode=mode)
        rel, x2b = warp_kpts(t["kpts"].double(), *args, depth_interpolation_mode=mode, return_relative_depth_error=True)
        assert torch.equal(x2, x2b) and valid.dtype == torch.bool and x2.dtype == torch.float64
        out[f"valid_{mode}"], out[f"x2_{mode}"], out[f"rel_{mode}"] = valid.numpy(), x2.numpy(), rel.numpy()
        for p, pair in enumerate(pairs):
            o = D.warp_kpts(pair["kpts"], pair["depth_A"], pair["depth_B"], pair["T"], pair["K_A"], pair["K_B"], mode, THRESHOLD)
            m_rel, m_border = D.margins(o, HB, WB, THRESHOLD)
            print(f"{mode} pair {p}: {valid[p].float().mean():.3f} valid; closest rel to the threshold {m_rel:.2e}, closest border "
                  f"{m_border:.2e} px; restatement - reference x2 {np.abs(o['x2'] - x2[p].numpy()).max():.1e}")
            assert m_rel > 1e-6 and m_border > 1e-6, "a decision sits on its threshold: pick another seed"
            assert np.array_equal(o["valid"], valid[p].numpy())
            assert np.abs(x2[p].numpy()).max() <= 20                        # holes and border points: see the module docstring

    gt, prob = get_gt_warp(t["depth_A"], t["depth_B"], t["T"], t["K_A"], t["K_B"])
    assert gt.shape == (3, HA, WA, 2) and gt.dtype == torch.float64 and prob.dtype == torch.float32
    out["gt_x2"], out["gt_prob"] = gt.numpy(), prob.numpy()
    assert np.abs(out["gt_x2"]).max() <= 20
    for p, pair in enumerate(pairs):
        o = D.warp_kpts(D.gt_grid(HA, WA), pair["depth_A"], pair["depth_B"], pair["T"], pair["K_A"], pair["K_B"], "bilinear", THRESHOLD)
        m_rel, m_border = D.margins(o, HB, WB, THRESHOLD)
        print(f"get_gt_warp pair {p}: {prob[p].mean():.3f} valid; margins {m_rel:.2e}, {m_border:.2e} px")
        assert m_rel > 1e-6 and m_border > 1e-6, "a decision sits on its threshold: pick another seed"

    # the predicted warp: the grid the reference builds, and its ground truth + N(0, 2 px) in the normalised units of the warp
    rng = np.random.default_rng(99)
    lin = [torch.linspace(-1 + 1 / n, 1 - 1 / n, n) for n in (HA, WA)]
    gy, gx = torch.meshgrid(*lin, indexing="ij")
    grid = torch.stack((gx, gy), -1)[None].expand(3, HA, WA, 2)
    noise = rng.normal(0, 2.0, (3, HA, WA, 2)) * np.array([2 / WA, 2 / HA])
    assert np.array_equal(grid[0].reshape(-1, 2).numpy(), D.gt_grid(HA, WA)), "the restated fp32 linspace is not torch's"
    pred = torch.cat((grid, (gt + torch.from_numpy(noise)).float()), -1).contiguous()
    assert pred.dtype == torch.float32 and bool(torch.isfinite(pred).all())
    out["pred_warp"] = pred.numpy()
    gd, pck_1, pck_3, pck_5, prob2 = geometric_dist(None, t["depth_A"], t["depth_B"], t["T"], t["K_A"], t["K_B"], pred)
    assert gd.dtype == torch.float64 and torch.equal(prob2, prob)
    out["gd"], out["pck"], out["gd_prob"] = gd.numpy(), np.array([pck_1.item(), pck_3.item(), pck_5.item()], np.float32), prob2.numpy()
    out["gd_pairs"] = prob2.reshape(3, -1).sum(1).numpy().astype(np.int64)                # gd is the three pairs' valid pixels in a row
    near = np.abs(out["gd"][:, None] - np.array([1.0, 3.0, 5.0])).min()
    print(f"geometric_dist: {len(out['gd'])} valid pixels, epe {out['gd'].mean():.4f} px, pck {out['pck']}; closest gd to 1, 3 or 5 px {near:.2e}")
    assert near > 1e-6, "a distance sits on a PCK threshold: pick another seed"

    path = os.path.join(HERE, "depth_warp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
