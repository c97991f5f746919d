"""CPU checks of tests/transformer_ref.py, which keep tests/test_transformer_kernels.py honest: the fp64 restatements equal torch's own
float64 operators, and every input builder separates a right kernel from the specific wrong one it was built for — the wrong
restatement misses the tolerance the GPU test applies to that input by at least ten times."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import transformer_ref as TF

torch.set_grad_enabled(False)
TEETH = 10.0


def _rand(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- the references are the operators they claim to be -----------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 520, 2048])
def test_add_layernorm_ref_is_layer_norm_in_float64(C):
    x, y = _rand((7, C), 1) * 3 + 2, _rand((7, C), 2)
    ls, g, b = _rand((C,), 3).abs() + 0.5, _rand((C,), 4).abs() + 0.5, _rand((C,), 5) * 0.1
    for use_ls in (None, ls):
        s = x + (y if use_ls is None else ls * y)
        new_x, out = TF.add_layernorm_ref(x, y, use_ls, g, b, 1e-6, torch.float64)
        assert torch.equal(new_x, s) and maxerr(out, F.layer_norm(s, (C,), g, b, 1e-6)) <= 1e-12
        new_x, out = TF.add_layernorm_ref(x, y, use_ls, None, None, 0.0, torch.float32)
        assert torch.equal(new_x, s) and torch.equal(out, s.float())
    new_x, out = TF.add_layernorm_ref(x, None, None, g, b, 1e-5, torch.float64)
    assert torch.equal(new_x, x) and maxerr(out, F.layer_norm(x, (C,), g, b, 1e-5)) <= 1e-12


def test_add_layernorm_ref_rounds_the_stream_once_and_normalises_what_it_stored():
    x, y = _rand((5, 96), 6, torch.bfloat16), _rand((5, 96), 7, torch.bfloat16)
    g, b = torch.ones(96), torch.zeros(96)
    new_x, out = TF.add_layernorm_ref(x, y, None, g, b, 1e-6, torch.float32)
    assert new_x.dtype == torch.bfloat16 and torch.equal(new_x, (x.double() + y.double()).to(torch.bfloat16))
    assert out.dtype == torch.float32 and maxerr(out, F.layer_norm(new_x.double(), (96,), g.double(), b.double(), 1e-6)) <= 1e-6


def test_to_stream_rounds_where_the_data_path_rounds():
    # the case that showed it: 63.9375 + 0.9018976 * -0.22521973 = 63.734374867, just below the fp16 midpoint 63.734375 that float32 gives
    v = torch.tensor([63.9375], dtype=torch.float64) + torch.tensor([0.9018976092338562]).double() * torch.tensor([-0.2252197265625]).double()
    assert 63.71875 < float(v) < 63.734375 and float(v.float()) == 63.734375
    assert float(TF.to_stream(v, torch.float16)) == 63.75 and float(v.to(torch.float16)) == 63.75          # a single rounding: 63.71875
    assert torch.equal(TF.to_stream(v, torch.float32), v.float())
    x = _rand((1 << 16,), 14) * 64
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(TF.to_stream(x, dtype), x.to(dtype))


@pytest.mark.parametrize("N,nv", [(1, None), (65, 65), (200, 137), (128, 1)])
def test_attention_ref_is_sdpa_in_float64(N, nv):
    qkv = _rand((2, N, 3, 3, 64), 8 + N)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    n = N if nv is None else nv
    ref = F.scaled_dot_product_attention(q, k[:, :, :n], v[:, :, :n]).transpose(1, 2).reshape(2, N, 192)
    assert maxerr(TF.attention_ref(qkv, nv), ref) <= 1e-12


@pytest.mark.parametrize("style", ["dino", "decoder"])
def test_block_stack_ref_is_block_forward_in_float64(style):
    from roma_amd.transformer import Block
    kw = dict(qkv_bias=True, init_values=1.0, ln_eps=1e-6) if style == "dino" else {}
    blocks = TF.init_module(nn.ModuleList([Block(128, 2, **kw) for _ in range(3)]), 1).double()
    final = TF.init_module(nn.LayerNorm(128, eps=1e-6), 2).double() if style == "dino" else None
    x = _rand((2, 256, 128), 9)
    t = x
    for blk in blocks:
        t = blk(t, 200)
    t = t if final is None else final(t)
    ref = TF.block_stack_ref(blocks, x, 200, final)
    assert maxerr(ref[:, :200], t[:, :200]) <= 1e-10
    # the padding rows are queries only: the real rows are those of the unpadded sequence
    assert maxerr(ref[:, :200], TF.block_stack_ref(blocks, x[:, :200], None, final)) <= 1e-10


# ---- teeth: add_layernorm ----------------------------------------------------------------------------------------------------------
def _affine(C):
    return torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5, _rand((C,), C + 1, torch.float32) * 0.1


@pytest.mark.parametrize("C", [512, 2048])
def test_offset_rows_tell_one_pass_variance_from_two_pass(C):
    x = TF.offset_rows(259, C)
    g, b = _affine(C)
    _, ref = TF.add_layernorm_ref(x, None, None, g, b, 1e-6, torch.float32)
    tol = TF.ln_out_tolerance(torch.float32, ref, offset=True)
    mean = x.mean(dim=-1, keepdim=True)
    one_pass = (x - mean) * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) - mean * mean + 1e-6) * g + b      # all fp32
    two_pass = (x - mean) * torch.rsqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + 1e-6) * g + b
    assert maxerr(one_pass, ref) >= TEETH * tol
    assert maxerr(two_pass, ref) <= tol


def test_offset_tolerance_is_the_derived_figure():
    assert abs(TF.offset_tolerance() - 8 * 2 ** -24 * 64 / 0.25) < 1e-12 and 1.2e-4 < TF.offset_tolerance() < 1.3e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rounded_stream_statistics_are_told_from_unrounded_ones(dtype):
    C = 1024
    x, y = _rand((259, C), 11, dtype), _rand((259, C), 12, dtype)
    ls, (g, b) = torch.rand(C, generator=torch.Generator().manual_seed(13)) + 0.5, _affine(C)
    _, ref = TF.add_layernorm_ref(x, y, ls, g, b, 1e-6, torch.float32)
    wrong = TF.layernorm64(x.double() + ls.double() * y.double(), g, b, 1e-6).float()
    assert maxerr(wrong, ref) >= TEETH * TF.ln_out_tolerance(torch.float32, ref)


# ---- teeth: attention --------------------------------------------------------------------------------------------------------------
def online_softmax_attention(qkv, n_valid, rescale=True, drop_tile0=False, swap_keys=False):
    """The kernel's loop over 64-key tiles in float64, with three ways of being wrong: the accumulator is not rescaled when the running
    maximum grows; tile 0 is skipped; keys 4 g + 1 and 4 g + 2 of every 4-key group change places in the second product."""
    B, N, _, H, d = qkv.shape
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    k, v = k[:, :, :n_valid], v[:, :, :n_valid].clone()
    if swap_keys:
        a = torch.arange(1, n_valid - 1, 4)
        v[:, :, a], v[:, :, a + 1] = v[:, :, a + 1].clone(), v[:, :, a].clone()
    m = torch.full((B, H, N, 1), -float("inf"), dtype=torch.float64)
    l, o = torch.zeros(B, H, N, 1, dtype=torch.float64), torch.zeros(B, H, N, d, dtype=torch.float64)
    for t0 in range(64 if drop_tile0 else 0, n_valid, 64):
        s = q @ k[:, :, t0:t0 + 64].transpose(-1, -2) * TF.ATT_SCALE
        m_new = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        o = (o * alpha if rescale else o) + p @ v[:, :, t0:t0 + 64]
        m = m_new
    return (o / l).permute(0, 2, 1, 3).reshape(B, N, H * d)


@pytest.mark.parametrize("N,nv", [(200, 137), (192, 128), (64, 64)])
def test_online_softmax_restatement_is_attention(N, nv):
    qkv = TF.noise_attention(1, N, 2, torch.float16)
    assert maxerr(online_softmax_attention(qkv, nv), TF.attention_ref(qkv, nv)) <= 1e-12


def _one_hot_excess(out, qkv, Nk):
    """largest |out - v[i mod Nk]| in units of the GPU test's element-wise bound, one ulp of |v|"""
    want = TF.one_hot_expected(qkv, Nk).double()
    return float(((out.double() - want).abs() / (TF.ULP[qkv.dtype] * want.abs())).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,Nk", TF.ONE_HOT_SHAPES)
def test_one_hot_attention_margin_and_teeth(N, Nk, dtype):
    qkv = TF.one_hot_attention(N, Nk, dtype)
    q, k = qkv[0, :, 0].permute(1, 0, 2).double(), qkv[0, :, 1].permute(1, 0, 2).double()     # (H, N, 64)
    u = k[:, :Nk] / 2.75
    assert torch.equal(u.abs(), torch.ones_like(u))
    for h in range(u.shape[0]):
        assert torch.unique(u[h], dim=0).shape[0] == Nk                                        # no two valid keys coincide
    logits = q @ k.transpose(-1, -2) * TF.ATT_SCALE                                            # (H, N, N)
    own = torch.arange(N) % Nk
    valid = logits[:, :, :Nk].clone()
    hit = valid[:, torch.arange(N), own]
    assert torch.equal(hit, torch.full_like(hit, 60.5))
    valid[:, torch.arange(N), own] = -float("inf")
    assert float((hit - valid.max(dim=-1).values).min()) >= 30.0
    p = torch.softmax(logits[:, :, :Nk], dim=-1)
    assert float((1 - p[:, torch.arange(N), own]).max()) <= 1e-13
    assert float(logits[:, :, Nk:].max()) == 121.0 and bool((qkv[0, Nk:, 2] == 1000).all())    # a leaked key wins, and shows
    # the right answer meets the GPU test's bound; one leaked key, or two keys swapped in the second product, miss it tenfold
    assert _one_hot_excess(TF.attention_ref(qkv, Nk), qkv, Nk) <= 1.0
    assert _one_hot_excess(TF.attention_ref(qkv, Nk + 1), qkv, Nk) >= TEETH
    assert _one_hot_excess(online_softmax_attention(qkv, Nk, swap_keys=True), qkv, Nk) >= TEETH
    # ... and on EVERY row the swap touches, so each key position is checked on its own
    want = TF.one_hot_expected(qkv, Nk).double()
    bad = ((online_softmax_attention(qkv, Nk, swap_keys=True) - want).abs() > TF.ULP[dtype] * want.abs()).any(dim=-1)[0]
    touched = torch.zeros(Nk, dtype=torch.bool)
    a = torch.arange(1, Nk - 1, 4)
    touched[a], touched[a + 1] = True, True
    assert torch.equal(bad, touched[own])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,Nk", TF.RAMP_SHAPES)
def test_ramp_attention_teeth(N, Nk, dtype):
    down, up = TF.ramp_attention(N, Nk, dtype, -1), TF.ramp_attention(N, Nk, dtype, +1)
    for qkv, sign in ((down, -1), (up, +1)):
        s = (qkv[0, :, 0].permute(1, 0, 2).double() @ qkv[0, :Nk, 1].permute(1, 2, 0).double()) * TF.ATT_SCALE   # (H, N, Nk)
        tile_max = torch.stack([s[:, :, t:t + 64].max(dim=-1).values for t in range(0, Nk, 64)])
        moves = tile_max[1:] > torch.cummax(tile_max, dim=0).values[:-1]
        assert bool(moves.all()) if sign > 0 else not bool(moves.any())                        # both branches of `grew`
    ref = TF.attention_ref(down, Nk)
    assert maxerr(online_softmax_attention(down, Nk, drop_tile0=True), ref) >= TEETH * TF.att_tolerance(dtype, ref)
    ref = TF.attention_ref(up, Nk)
    assert maxerr(online_softmax_attention(up, Nk, rescale=False), ref) >= TEETH * TF.att_tolerance(dtype, ref)
    if Nk < N:
        assert maxerr(TF.attention_ref(up, Nk + 1), ref) >= TEETH * TF.att_tolerance(dtype, ref)
