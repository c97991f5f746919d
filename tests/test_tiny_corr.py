"""ops.tiny_corr_posembed (TinyRoMa's corr_volume + pos_embed in one fp32 MFMA kernel) at its edges: every channel instantiation,
partial tiles and blocks, unequal image sizes, the online softmax under a rising maximum and under logits whose exp overflows, the
fast path where the stride-4 sub-grid softmax carries weight, arg-max ties, the batch offset.

The yardstick is oracle.roma_oracle.tiny_corr_volume + tiny_pos_embed in float64 on the CPU, one call per batch item (the oracle's
fast path is B = 1 only; the kernel applies those semantics to every item).  The tolerance is measured inside each test: the oracle's
own fp32 evaluation is compared with its fp64 evaluation on the same inputs, and the kernel may be at most 4 times as far from the
fp64 result (both sum in fp32; only the order differs), with the floor 2e-5 that test_tiny_corr_posembed_full_size uses.

Conditions on the inputs that need no device (enough fast-path pixels whose extra logit neither swallows the softmax nor vanishes
from it, a score above 100, the reference's arg-max at the lower of two tied indices) are asserted in the unmarked tests and again
where the kernel runs.

Measured on MI355X (worst max |difference| to the fp64 yardstick, oracle fp32 / kernel; the bound was the floor 2e-5 everywhere but
for the large logits, 2.1e-5):
    exact, over the six shapes   C=16 1.09e-6 / 7.5e-7    C=32 1.25e-6 / 8.0e-7    C=64 1.37e-6 / 1.37e-6    C=128 1.77e-6 / 1.91e-6
    rising maximum 2.3e-7 / 1.6e-7    falling maximum 7.7e-7 / 3.2e-7    large logits (top score 190) 5.3e-6 / 3.4e-6
    fast, over the ten shapes    C=16 1.05e-7 / 1.13e-7   C=64 1.25e-7 / 1.17e-7   C=128 2.30e-7 / 2.15e-7
    fast, over the 746 pixels with 0.05 < P(extra logit) < 0.95 alone: 2.30e-7 / 2.15e-7
    ties 1.04e-7 / 1.61e-7
"""
import functools

import pytest
import torch

from oracle import roma_oracle as O

torch.set_grad_enabled(False)
DEV = "cuda:0"
FLOOR = 2e-5

CHANNELS = [16, 32, 64, 128]
EXACT_SHAPES = [(5, 7, 3, 5),        # N0 = 35, N1 = 15: less than one tile, clamped tail lanes on both operands
                (7, 9, 5, 13),       # N1 = 65: two tiles and one row
                (6, 6, 7, 9),
                (1, 1, 1, 1),        # lin(n == 1) on both axes, the upper lane half has nothing to sum
                (12, 20, 12, 20),    # N = 240: 16-lane tail, fourth wave partly live
                (9, 15, 4, 8)]       # N0 = 135: one live wave in the second block, three beyond N0
FAST_CHANNELS = [16, 64, 128]
FAST_TARGETS = [(4, 4), (4, 8), (8, 4), (8, 12), (12, 20)]      # one sub-grid point (j = 0); two (j = 0, 4) in opposite lane halves; ...
FAST_SOURCES = [(5, 7), (9, 13)]
FAST_BATCH = 3
FAST_SEED = 7
# (lower, upper) tied target rows at (H1, W1) = (8, 12); a lane holds rows j0 + (r & 3) + 8 (r >> 2) + 4 half of tile j0, so:
TIES = [(3, 40),     # tiles 0 and 1, both in the lower lane half: settled within a lane, across tiles
        (3, 44),     # tiles 0 and 1, lower and upper half
        (1, 5),      # one tile, lower and upper half
        (6, 41)]     # tiles 0 and 1, the LOWER index in the upper half: the half combine has to hand it over
TIE_SOURCES = (2, 11, 33, 50, 116)


def reference(f0, f1, exact, dtype):
    """The oracle per batch item, evaluated in `dtype`; returned in float64."""
    out = [O.tiny_pos_embed(O.tiny_corr_volume(f0[b:b + 1].to(dtype), f1[b:b + 1].to(dtype)), exact_softmax=exact) for b in range(f0.shape[0])]
    return torch.cat(out).double()


def extra_logit_probability(f0, f1):
    """(B, H0, W0): the probability the fast path's softmax gives the extra logit (the arg-max index), from the fp64 volume."""
    cv = O.tiny_corr_volume(f0.double(), f1.double())
    B, H1, W1, H0, W0 = cv.shape
    best = cv.reshape(B, H1 * W1, H0, W0).argmax(dim=1)
    low = cv[:, ::4, ::4].reshape(B, -1, H0, W0)
    return torch.cat((low, best[:, None].to(low.dtype)), dim=1).softmax(dim=1)[:, -1]


def features(B, C, H0, W0, H1, W1, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H0, W0, generator=g) * scale, torch.randn(B, C, H1, W1, generator=g) * scale


def check(f0, f1, exact, label, rows=None):
    """Run the kernel, print the two distances, assert the bound.  rows: a (B, H0, W0) mask of pixels to report and bound separately."""
    from roma_amd import ops
    ref = reference(f0, f1, exact, torch.float64)
    assert bool(torch.isfinite(ref).all())
    e32 = (reference(f0, f1, exact, torch.float32) - ref).abs()
    out = ops.tiny_corr_posembed(f0.to(DEV), f1.to(DEV), exact=exact)
    assert out.shape == ref.shape and out.dtype == torch.float32
    out = out.cpu().double()
    assert bool(torch.isfinite(out).all()), label
    e = (out - ref).abs()
    tol = max(4 * float(e32.max()), FLOOR)
    print(f"{label}: oracle fp32 {float(e32.max()):.3e}  kernel {float(e.max()):.3e}  bound {tol:.3e}")
    assert float(e.max()) <= tol, (label, float(e.max()), tol)
    if rows is not None:
        m = rows[:, None].expand_as(e)
        tol_m = max(4 * float(e32[m].max()), FLOOR)
        print(f"{label}: over the {int(rows.sum())} chosen pixels: oracle fp32 {float(e32[m].max()):.3e}  kernel {float(e[m].max()):.3e}")
        assert float(e[m].max()) <= tol_m, (label, float(e[m].max()), tol_m)
    return float(e32.max()), float(e.max())


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def ramp_inputs(rising):
    """Every source pixel points along u; target j is a_j u + noise with a_j monotonic in j over N1 = 5 * 32 + 7 targets, so that
    with a_j rising the running maximum of the online softmax rises in every tile (scores from 0 to about 40)."""
    g = torch.Generator().manual_seed(11)
    C, N1 = 64, 5 * 32 + 7
    u = torch.randn(C, generator=g)
    u = u / u.norm()
    f0 = (4.0 + torch.rand(1, 1, 5, 7, generator=g)) * u[None, :, None, None] + 0.05 * torch.randn(1, C, 5, 7, generator=g)
    a = torch.linspace(0.0, 64.0, N1)
    if not rising:
        a = a.flip(0)
    f1 = a[None, None, :] * u[None, :, None] + 0.05 * torch.randn(1, C, N1, generator=g)
    return f0, (f1.reshape(1, C, 1, N1) if rising else f1.reshape(1, C, N1, 1))       # a row of targets, a column of targets


def large_logit_inputs():
    return features(2, 64, 6, 6, 7, 9, seed=13, scale=7.0)


@functools.lru_cache(maxsize=None)
def fast_inputs(C, H0, W0, H1, W1):
    f0, f1 = features(FAST_BATCH, C, H0, W0, H1, W1, seed=FAST_SEED + 1000 * C + 100 * H1 + 10 * W1 + H0)
    p = extra_logit_probability(f0, f1)
    return f0, f1, (p > 0.05) & (p < 0.95)


def fast_cases():
    return [(C, h0, w0, h1, w1) for C in FAST_CHANNELS for (h1, w1) in FAST_TARGETS for (h0, w0) in FAST_SOURCES]


def tie_inputs(lo, hi):
    """(9,13) sources, (8,12) targets: target rows lo and hi are bitwise equal and a multiple of the features that the source pixels
    TIE_SOURCES share (up to a positive factor each), so that they are those pixels' best match by a wide margin."""
    C, H0, W0, H1, W1 = 64, 9, 13, 8, 12
    f0, f1 = features(1, C, H0, W0, H1, W1, seed=17)
    g = torch.Generator().manual_seed(19)
    v = torch.randn(C, generator=g)
    f0v, f1v = f0.reshape(1, C, -1), f1.reshape(1, C, -1)
    for n, i in enumerate(TIE_SOURCES):
        f0v[0, :, i] = v * (0.75 + 0.25 * n)
    f1v[0, :, lo] = f1v[0, :, hi] = 0.5 * v
    assert torch.equal(f1v[0, :, lo], f1v[0, :, hi])
    return f0, f1


def reference_argmax(f0, f1):
    cv = O.tiny_corr_volume(f0.double(), f1.double())
    B, H1, W1, H0, W0 = cv.shape
    return cv.reshape(B, H1 * W1, H0 * W0).argmax(dim=1)


# ---- conditions on the inputs: no device --------------------------------------------------------------------------------------
def count_mixed_pixels():
    return sum(int(fast_inputs(*case)[2].sum()) for case in fast_cases())


def test_fast_inputs_have_pixels_whose_subgrid_softmax_matters():
    per_target = {t: sum(int(fast_inputs(*c)[2].sum()) for c in fast_cases() if c[3:] == t) for t in FAST_TARGETS}
    print("pixels with 0.05 < P(extra logit) < 0.95 per (H1,W1):", per_target)
    assert count_mixed_pixels() >= 20
    assert per_target[(4, 4)] >= 20          # lin(n == 1) on both axes of grid_lr, on pixels where grid_lr carries weight


def test_large_logit_inputs_overflow_exp_in_fp32():
    f0, f1 = large_logit_inputs()
    top = O.tiny_corr_volume(f0.double(), f1.double()).max()
    assert float(top) > 100 and not bool(torch.isfinite(torch.exp(top.float())))
    assert bool(torch.isfinite(reference(f0, f1, True, torch.float64)).all())


@pytest.mark.parametrize("rising", [True, False])
def test_ramp_inputs_raise_the_maximum_in_every_tile(rising):
    f0, f1 = ramp_inputs(rising)
    cv = O.tiny_corr_volume(f0.double(), f1.double()).reshape(167, 35)
    tile_max = torch.stack([cv[j:j + 32].max(dim=0).values for j in range(0, 167, 32)])          # (6 tiles, 35 source pixels)
    step = tile_max[1:] - tile_max[:-1]
    assert bool((step > 1).all()) if rising else bool((step < -1).all())
    assert bool(torch.isfinite(reference(f0, f1, True, torch.float64)).all())


@pytest.mark.parametrize("lo,hi", TIES)
def test_reference_settles_a_tie_at_the_lower_index(lo, hi):
    f0, f1 = tie_inputs(lo, hi)
    best = reference_argmax(f0, f1)[0]
    assert best[list(TIE_SOURCES)].tolist() == [lo] * len(TIE_SOURCES)
    cv = O.tiny_corr_volume(f0.double(), f1.double()).reshape(96, -1)
    assert torch.equal(cv[lo], cv[hi])                                   # a tie in the reference's own scores as well
    assert (lo // 12) % 4 or (lo % 12) % 4                               # neither row is on the stride-4 sub-grid
    assert (hi // 12) % 4 or (hi % 12) % 4


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_exact_path_every_instantiation(C):
    worst = (0.0, 0.0)
    for n, (H0, W0, H1, W1) in enumerate(EXACT_SHAPES):
        f0, f1 = features(2, C, H0, W0, H1, W1, seed=100 * C + n, scale=2.0)
        assert not torch.equal(f0[0], f0[1])
        worst = tuple(map(max, worst, check(f0, f1, True, f"exact C={C} ({H0},{W0})->({H1},{W1})")))
    print(f"exact C={C} worst: oracle fp32 {worst[0]:.3e}  kernel {worst[1]:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("rising", [True, False])
def test_online_softmax_with_a_monotonic_maximum(rising):
    check(*ramp_inputs(rising), True, f"ramp rising={rising}")


@pytest.mark.gpu
def test_online_softmax_with_logits_beyond_exp_range():
    f0, f1 = large_logit_inputs()
    assert float(O.tiny_corr_volume(f0.double(), f1.double()).max()) > 100
    check(f0, f1, True, "large logits")


@pytest.mark.gpu
@pytest.mark.parametrize("C", FAST_CHANNELS)
def test_fast_path_where_the_subgrid_softmax_matters(C):
    assert count_mixed_pixels() >= 20
    worst = (0.0, 0.0)
    for case in fast_cases():
        if case[0] != C:
            continue
        f0, f1, mixed = fast_inputs(*case)
        worst = tuple(map(max, worst, check(f0, f1, False, "fast C=%d (%d,%d)->(%d,%d)" % case, rows=mixed if bool(mixed.any()) else None)))
    print(f"fast C={C} worst: oracle fp32 {worst[0]:.3e}  kernel {worst[1]:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", TIES)
def test_fast_path_settles_a_tie_at_the_lower_index(lo, hi):
    f0, f1 = tie_inputs(lo, hi)
    assert reference_argmax(f0, f1)[0][list(TIE_SOURCES)].tolist() == [lo] * len(TIE_SOURCES)
    rows = torch.zeros(1, 9 * 13, dtype=torch.bool)
    rows[0, list(TIE_SOURCES)] = True
    check(f0, f1, False, f"tie ({lo},{hi})", rows=rows.reshape(1, 9, 13))


@pytest.mark.gpu
def test_refusals():
    from roma_amd import ops
    with pytest.raises(ValueError, match="C=24"):
        ops.tiny_corr_posembed(*(t.to(DEV) for t in features(1, 24, 4, 4, 4, 4, seed=0)), exact=True)
    for H1, W1 in [(4, 6), (6, 4)]:
        f0, f1 = (t.to(DEV) for t in features(1, 64, 4, 4, H1, W1, seed=0))
        with pytest.raises(ValueError, match="divisible by 4"):
            ops.tiny_corr_posembed(f0, f1, exact=False)
        assert ops.tiny_corr_posembed(f0, f1, exact=True).shape == (1, 2, 4, 4)      # the exact path takes them
