"""matcher.mid_block_impl: which `split_mfma` blocks run as one launch (ops.refiner_block_mid) — host logic, no device."""
import torch

from roma_amd.matcher import MID_ONE_MIN_PIXELS, block_impl, mid_block_impl


def test_mid_block_impl_at_the_product_shapes():
    """The flagship step runs the scale-2 refiner (Dp = 144, B = 2) at 280^2 (coarse pass) and 432^2 (upsample pass)."""
    for dtype in (torch.float16, torch.bfloat16):
        assert block_impl(144, dtype, 2, 280, 280) == block_impl(144, dtype, 2, 432, 432) == "split_mfma"
        assert mid_block_impl(dtype, 144, 2, 432, 432) == "one"
        assert mid_block_impl(dtype, 144, 2, 280, 280) == "one"


def test_mid_block_impl_boundary():
    """The rule is a pixel count: one launch from MID_ONE_MIN_PIXELS pixels on, two calls below."""
    n = MID_ONE_MIN_PIXELS
    assert 0 < n <= 2 * 280 * 280
    for dtype in (torch.float16, torch.bfloat16):
        assert mid_block_impl(dtype, 144, 1, 1, n) == "one"
        assert mid_block_impl(dtype, 144, 1, 1, n - 1) == "two"
        assert mid_block_impl(dtype, 144, 2, 1, (n + 1) // 2) == "one"
        assert mid_block_impl(dtype, 144, 1, 19, 23) == "two"
        assert mid_block_impl(dtype, 160, 1, 1, n) == "one" and mid_block_impl(dtype, 40, 1, 1, n) == "one"


def test_mid_block_impl_never_for_fp32_or_narrow_or_wide():
    for shape in ((2, 432, 432), (2, 280, 280), (1, 5, 3)):
        assert mid_block_impl(torch.float32, 144, *shape) == "two"
        for dtype in (torch.float16, torch.bfloat16, torch.float32):
            for Dp in (8, 24, 32, 168, 576):
                assert mid_block_impl(dtype, Dp, *shape) == "two"
