"""The small kernels at the tail of match(): ops.match_finalize, ops.nn_argmin, preproc.resize_device / preprocess_device — at the
layouts, sizes and values their golden tests leave out.

match_finalize against oracle.roma_oracle.match_finalize (literal torch on the CPU) with the golden test's bounds (1e-6 on the warp
and on the certainty) and the SAME set of zeroed certainties: non-symmetric layout, no coarse certainty, P > 1, non-integer coarse
ratios, a single pixel, the grid-stride loop, and flow components planted at exactly +-1 (kept) and one ulp beyond (zeroed).
nn_argmin on a dyadic lattice, where every fp32 distance is exact and the answer is an integer arg-min with the lowest index on ties:
torch.equal, across the 1024-point LDS tile and the 256-thread block.  The resampler against PIL itself, bit for bit: up-scaling,
an unchanged axis, one-to-three-pixel images, a 140-fold reduction, and saturated images whose bicubic overshoot is clipped at both
ends.

Measured on MI355X: match_finalize — the warp equals the oracle's bit for bit in all seven cases, the certainty differs by at most
1.19e-7 (0 in the one-pixel cases), the zeroed sets are equal (196 298 of 2 109 440 in the grid-stride case); nn_argmin — equal in all
twenty (NQ, NR) pairs, with up to 185 of 700 queries on a tied minimum; the resampler — equal to PIL in all 10 x 5 images.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import roma_oracle as O

torch.set_grad_enabled(False)
DEV = "cuda:0"


# ---- match_finalize -----------------------------------------------------------------------------------------------------------
ONE_UP, MINUS_ONE_DOWN = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(-1), np.float32(-2)))
PLANTED = (1.0, -1.0, ONE_UP, MINUS_ONE_DOWN)
#                name                 B  symmetric (H, W)        cert16
FINALIZE_CASES = [("symmetric_P3",     6, True,  (33, 47),     (5, 6)),
                  ("single_c16",       3, False, (33, 47),     (5, 6)),
                  ("single_plain",     3, False, (33, 47),     None),
                  ("ratio_10.8",       2, True,  (54, 54),     (5, 5)),
                  ("one_pixel",        2, True,  (1, 1),       (1, 1)),
                  ("one_pixel_single", 4, False, (1, 1),       None),
                  ("grid_stride",      2, True,  (1030, 1024), (5, 6))]      # 2 109 440 outputs > 8192 * 256 threads


def finalize_inputs(B, H, W, c16, seed):
    """cases.post_inputs' flow (identity grid * 1.05 + noise: the border is out of bounds by itself) with, per batch item, eight
    pixels whose one component is planted at +-1 or one ulp beyond while the other is well inside."""
    g = torch.Generator().manual_seed(seed)
    flow = O.pixel_grid(B, H, W) * 1.05 + 0.02 * torch.randn(B, 2, H, W, generator=g)
    cert = 2.0 * torch.randn(B, 1, H, W, generator=g)
    low = None if c16 is None else 2.0 * torch.randn(B, 1, *c16, generator=g)
    planted = torch.zeros(B, H, W, dtype=torch.bool)
    fv = flow.reshape(B, 2, H * W)
    for b in range(B):
        for k in range(len(PLANTED)):
            for comp in (0, 1):
                pix = ((2 * k + comp) * 7919 + 31 * b + (H * W) // 3) % (H * W)
                fv[b, :, pix] = 0.25
                fv[b, comp, pix] = PLANTED[(k + b) % 4]              # on a single pixel the last one stays: another per item
                planted.reshape(B, -1)[b, pix] = True
    return flow, cert, low, planted


def finalize_reference(flow, cert, low, symmetric):
    H, W = flow.shape[-2:]
    return O.match_finalize(flow, cert, low, H, W, symmetric=symmetric, attenuate_cert=low is not None)


def test_planted_flow_values_decide_the_reference_certainty():
    """+-1 keeps the certainty, one ulp beyond zeroes it — in the reference, at the planted pixels of a case."""
    flow, cert, low, planted = finalize_inputs(3, 33, 47, (5, 6), seed=1)
    _, c = finalize_reference(flow, cert, low, False)
    kept = (flow.abs() == 1).any(dim=1) & planted
    cut = ((flow == ONE_UP) | (flow == MINUS_ONE_DOWN)).any(dim=1) & planted
    assert int(kept.sum()) == 12 and int(cut.sum()) == 12
    assert bool((c[kept] > 0).all()) and bool((c[cut] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,symmetric,size,c16", FINALIZE_CASES, ids=[c[0] for c in FINALIZE_CASES])
def test_match_finalize_against_the_oracle(name, B, symmetric, size, c16):
    from roma_amd import ops
    flow, cert, low, planted = finalize_inputs(B, *size, c16, seed=len(name) + B)
    ref_w, ref_c = finalize_reference(flow, cert, low, symmetric)
    warp, c = ops.match_finalize(flow.to(DEV), cert.to(DEV), None if low is None else low.to(DEV), symmetric=symmetric)
    assert warp.shape == ref_w.shape and c.shape == ref_c.shape
    warp, c = warp.cpu(), c.cpu()
    assert torch.equal(c == 0, ref_c == 0)
    assert 0 < int((ref_c == 0).sum()) < ref_c.numel()
    ew, ec = float((warp - ref_w).abs().max()), float((c - ref_c).abs().max())
    print(f"{name}: warp {ew:.3e}  certainty {ec:.3e}  zeroed {int((ref_c == 0).sum())} of {ref_c.numel()}")
    assert ew < 1e-6 and ec < 1e-6
    # the planted components come back exactly: +-1 unclamped, the ulp beyond clamped to +-1
    P = B // 2 if symmetric else B
    W = size[1]
    got = torch.cat((warp[:, :, :W, 2:], warp[:, :, W:, :2]), dim=0) if symmetric else warp[..., 2:]
    assert got.shape[0] == B and torch.equal(got[planted], flow.permute(0, 2, 3, 1)[planted].clamp(-1, 1))
    assert P * (2 if symmetric else 1) == B


# ---- nn_argmin ----------------------------------------------------------------------------------------------------------------
NN_REF = [1, 1023, 1024, 1025, 2500]           # the LDS tile holds 1024 reference points
NN_QUERY = [1, 255, 257, 700]                  # a block handles 256 queries


@functools.lru_cache(maxsize=None)
def nn_inputs(NQ, NR):
    """Integer lattice coordinates k in [-64, 64] (points are k / 64: every fp32 difference, square and sum is exact).  The same
    reference point sits at index 5 and at the last index — in the second tile from NR = 1025 on — and at 1030 where that exists;
    three queries lie exactly on it, so that only the tie rule decides their answer."""
    g = torch.Generator().manual_seed(1000 * NR + NQ)
    q = torch.randint(-64, 65, (NQ, 2), generator=g)
    r = torch.randint(-64, 65, (NR, 2), generator=g)
    on_it = []
    if NR > 6:
        twin = torch.tensor([37, -21])
        r[(r == twin).all(dim=1)] += 1                      # nowhere else
        r[5] = r[NR - 1] = twin
        if NR > 1030:
            r[1030] = twin
        on_it = sorted({0, NQ // 2, NQ - 1})
        q[on_it] = twin
    d = ((q[:, None, :] - r[None, :, :]) ** 2).sum(dim=-1).numpy()                  # int64, exact
    ref = torch.from_numpy(np.argmin(d, axis=1))                                    # numpy: the first minimum
    ties = int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return q, r, ref, on_it, ties


@pytest.mark.parametrize("NR", NN_REF)
def test_nn_reference_has_ties_settled_at_the_lower_index(NR):
    for NQ in NN_QUERY:
        q, r, ref, on_it, ties = nn_inputs(NQ, NR)
        assert int(ref.max()) < NR
        if NR > 6:
            assert ref[on_it].tolist() == [5] * len(on_it) and ties >= len(on_it)
    assert NR < 2500 or nn_inputs(700, NR)[4] > 3          # duplicates beyond the planted ones occur by themselves


@pytest.mark.gpu
@pytest.mark.parametrize("NR", NN_REF)
def test_nn_argmin_is_exact_on_a_dyadic_lattice(NR):
    from roma_amd import ops
    for NQ in NN_QUERY:
        q, r, ref, on_it, ties = nn_inputs(NQ, NR)
        got = ops.nn_argmin((q.float() / 64).to(DEV), (r.float() / 64).to(DEV))
        assert got.dtype == torch.int64 and got.shape == (NQ,)
        assert torch.equal(got.cpu(), ref), (NQ, NR, int((got.cpu() != ref).sum()))
        print(f"NQ={NQ} NR={NR}: {ties} queries with tied minima, all at the lowest index")


# ---- resize_device / preprocess_device ----------------------------------------------------------------------------------------
RESIZE_PAIRS = [((37, 53), (53, 37)), ((37, 53), (74, 106)), ((100, 90), (864, 864)), ((1, 1), (5, 5)), ((2, 3), (7, 2)),
                ((1000, 700), (7, 9)), ((64, 64), (64, 33)), ((64, 64), (33, 64)), ((5, 1000), (5, 3)), ((3, 2), (1, 1))]
SATURATED = ("checkerboard", "random_cells")


def cell(n_in, n_out):
    """Cell size of the saturated images along one axis: one sample when the axis grows or stays, otherwise wide enough that a cell
    covers two output samples — a one-sample pattern reduced 140-fold is a flat grey and would exercise no clipping."""
    return 1 if n_out >= n_in else -(-2 * n_in // n_out)


@functools.lru_cache(maxsize=None)
def images(src, dst):
    """uint8 (H, W, 3): uniform noise; a 0/255 checkerboard with the colour channels in opposite phase and random 0/255 per channel, both
    once per sample and once per cell of cell() samples (SATURATED: the ones that still hold 0 and 255 after any reduction)."""
    (H, W), (h, w) = src, dst
    rs = np.random.RandomState(7 * H + 13 * W + 17 * h + w)
    cy, cx = cell(H, h), cell(W, w)
    yy, xx = np.mgrid[:H, :W]
    par, one = ((yy // cy + xx // cx) % 2).astype(np.uint8), ((yy + xx) % 2).astype(np.uint8)
    ny, nx = -(-H // cy), -(-W // cx)
    for _ in range(64):                                              # a draw that has both values, however few the cells
        cells = rs.randint(0, 2, (ny, nx, 3)).astype(np.uint8)
        if cells.min() != cells.max():
            break
    return {"noise": rs.randint(0, 256, (H, W, 3)).astype(np.uint8),
            "random_samples": (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8),
            "checkerboard_samples": np.stack((one, 1 - one, one), axis=-1) * np.uint8(255),
            "checkerboard": np.stack((par, 1 - par, par), axis=-1) * np.uint8(255),
            "random_cells": cells[yy // cy, xx // cx] * np.uint8(255)}


def pil_resize(img, dst):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BICUBIC))


@pytest.mark.parametrize("src,dst", RESIZE_PAIRS)
def test_saturated_images_are_clipped_at_both_ends_by_pil(src, dst):
    for kind in SATURATED:
        out = pil_resize(images(src, dst)[kind], dst)
        assert out.shape == (*dst, 3) and bool((out == 0).any()) and bool((out == 255).any()), (kind, int(out.min()), int(out.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", RESIZE_PAIRS)
def test_device_resize_equals_pil(src, dst):
    from PIL import Image
    from roma_amd.matcher import preprocess
    from roma_amd.preproc import preprocess_device, resize_device
    for kind, img in images(src, dst).items():
        ref = pil_resize(img, dst)
        if kind in SATURATED:
            assert bool((ref == 0).any()) and bool((ref == 255).any()), kind
        got = resize_device(torch.from_numpy(img).to(DEV), dst)
        assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
        assert np.array_equal(got.cpu().numpy(), ref), (kind, int((got.cpu().numpy() != ref).sum()))
        host = preprocess(Image.fromarray(img), dst)
        for source in (Image.fromarray(img), torch.from_numpy(img)):
            dev = preprocess_device(source, dst, DEV)
            assert dev.shape == host.shape and torch.equal(dev.cpu(), host), kind
