"""RegressionMatcher.conf_from_fb_consistency against the reference's own output (tests/golden/fb_consistency.npz, written by
tests/golden/make_golden_fb.py, whose docstring describes the input).

The rule.  The mask must equal the reference's at every pixel except those whose reference distance lies within 1e-4 th_n of the
threshold th_n — the device's bilinear weights and its linspace may differ from the CPU's in the last bits, 1e-4 th_n = 1.25e-5 is
two hundred fp32 roundings of a coordinate —, and at most 1 % of the pixels may be excused that way.  The fixture keeps every
distance at least 2.6e-4 th_n away from the threshold (checked below, on the CPU), so in fact no pixel is excused."""
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fb_consistency.npz")
H, W = 24, 32


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _th_n(g):
    return 2 * int(g["th"]) / max(H, W)


def _matcher():
    from roma_amd.matcher import RegressionMatcher
    return RegressionMatcher(None, None)


def _assert_mask(mask, ref, dist, th_n):
    excused = np.abs(dist - th_n) <= 1e-4 * th_n
    assert excused.mean() <= 0.01
    differ = (mask > 0) != (ref > 0)
    print(f"{int(differ.sum())} pixels differ, {int(excused.sum())} excused")
    assert not (differ & ~excused).any()
    assert set(np.unique(mask)) <= {0.0, 1.0}


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_is_what_the_rule_assumes(golden):
    th_n = _th_n(golden)
    assert golden["ff"].shape == (H, W, 2) and golden["fb"].shape == (H, W, 2) and golden["mask_batched"].shape == (2, H, W)
    for name in ("base", "out"):
        mask, dist = golden["mask_" + name], golden["dist_" + name]
        assert np.array_equal(dist < th_n, mask > 0)
        margin = np.abs(dist - th_n).min() / th_n
        print(f"{name}: {mask.mean():.4f} consistent, closest distance {margin:.3e} th_n from the threshold")
        assert margin >= 2.6e-4                                   # no pixel near the threshold: nothing is excused
        assert 0.3 < mask.mean() < 0.45                           # both classes are well populated
    outside = (np.abs(golden["ff"]) > 1).any(-1)
    assert outside.sum() >= 4 and not (np.abs(golden["ff_base"]) > 1).any()
    # zero padding is visible in the mask: pixels that are consistent only because a position outside returns (0, 0)
    assert ((golden["mask_out"] > 0) & (golden["mask_base"] == 0) & outside).sum() >= 2
    assert np.array_equal(golden["mask_batched"][0], golden["mask_out"]) and np.array_equal(golden["mask_batched"][1], golden["mask_base"])


def test_conf_from_fb_consistency_refuses_cpu_tensors(golden):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _matcher().conf_from_fb_consistency(torch.from_numpy(golden["ff"]), torch.from_numpy(golden["fb"]), th=2)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_conf_from_fb_consistency_matches_the_reference(golden):
    m, th, th_n = _matcher(), int(golden["th"]), _th_n(golden)
    fb = torch.from_numpy(golden["fb"]).to(DEV)
    for name, key in (("base", "ff_base"), ("out", "ff")):
        ff = torch.from_numpy(golden[key]).to(DEV)
        mask = m.conf_from_fb_consistency(ff, fb, th=th)
        assert mask.shape == (H, W) and mask.dtype == torch.float32 and mask.is_cuda          # no batch in, none out
        _assert_mask(mask.cpu().numpy(), golden["mask_" + name], golden["dist_" + name], th_n)
    both = m.conf_from_fb_consistency(torch.from_numpy(np.stack([golden["ff"], golden["ff_base"]])).to(DEV), torch.stack([fb, fb]), th=th)
    assert both.shape == (2, H, W) and both.dtype == torch.float32
    _assert_mask(both[0].cpu().numpy(), golden["mask_batched"][0], golden["dist_out"], th_n)
    _assert_mask(both[1].cpu().numpy(), golden["mask_batched"][1], golden["dist_base"], th_n)
    one = m.conf_from_fb_consistency(torch.from_numpy(golden["ff"]).to(DEV)[None], fb[None], th=th)
    assert one.shape == (1, H, W)                                                              # a batch of one stays a batch
    # another threshold moves the mask the way th_n = 2 th / max(H, W) says
    wide = m.conf_from_fb_consistency(torch.from_numpy(golden["ff_base"]).to(DEV), fb, th=4).cpu().numpy()
    d = golden["dist_base"]
    clear = np.abs(d - 2 * th_n) > 1e-4 * th_n
    assert np.array_equal((wide > 0)[clear], (d < 2 * th_n)[clear])
