"""The 16-bit transformer path on the MI355X against tests/transformer_ref.py (fp64 on the CPU): ops.add_layernorm at every chunk count,
dtype pair, mode and row pitch; ops.attention in both instantiations on inputs that show a leaked, dropped or misplaced key on its own;
run_blocks_fused / TransformerDecoder.forward_rows / DinoViT.patch_tokens against the literal pre-LN block.
tests/test_transformer_ref.py proves on the CPU that each input used here would expose the wrong kernel it was built for."""
import contextlib
import copy
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import transformer_ref as TF

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def _ops():
    from roma_amd import ops
    return ops


def _L():
    from roma_amd import _lib
    return _lib


def _code(dtype):
    L = _L()
    return {F32: L.ROMA_F32, F16: L.ROMA_F16, BF16: L.ROMA_BF16}[dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- add_layernorm -----------------------------------------------------------------------------------------------------------------
PAIRS = [(F32, F32), (F32, F16), (F32, BF16), (F16, F16), (BF16, BF16)]                         # (stream, branch)
ODTS = [F32, F16, BF16]
NCH1, NCH4, MID = [8, 96, 512], [1544, 2040, 2048], [520, 1024, 1536]                          # 1 chunk; 4 chunks; 2, 2 and 3 chunks


def _aln_cases():
    """Every (pair, out dtype) at one 1-chunk and one 4-chunk width, and every C with every pair."""
    out = []
    for pi, (xdt, ydt) in enumerate(PAIRS):
        for oi, odt in enumerate(ODTS):
            out += [(xdt, ydt, odt, NCH1[(pi + oi) % 3]), (xdt, ydt, odt, NCH4[(pi + oi) % 3])]
        out += [(xdt, ydt, ODTS[(pi + k) % 3], C) for k, C in enumerate(MID)]
    return out


@functools.lru_cache(maxsize=None)
def _aln_rows(kind, rows, C):
    """fp32 masters (x, y) on the CPU: N(0, 1) rows, or rows of mean 64 and std 0.25 with a zero-mean branch of the same spread."""
    if kind == "offset":
        return TF.offset_rows(rows, C), TF.offset_rows(rows, C, mean=0.0, seed=1)
    g = torch.Generator().manual_seed(rows * 4099 + C)
    return torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)


@functools.lru_cache(maxsize=None)
def _aln_affine(C):
    g = torch.Generator().manual_seed(C)
    return torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1     # ls, gamma, beta


def _check_stream(xs, new_x):
    """the bound of test_gpu_ops.py::test_add_layernorm_vs_torch on the stream written back"""
    bound = float(new_x.double().abs().max()) * (2 ** -10 if new_x.dtype != F32 else 1e-7)
    assert xs.dtype == new_x.dtype and (torch.equal(xs.cpu(), new_x) or maxerr(xs, new_x) <= bound)


@pytest.mark.parametrize("xdt,ydt,odt,C", _aln_cases())
def test_add_layernorm_vs_fp64(xdt, ydt, odt, C):
    ops = _ops()
    ls, g, b = _aln_affine(C)
    lsd, gd, bd = ls.to(DEV), g.to(DEV), b.to(DEV)
    for kind in ("normal", "offset"):
        for rows in (1, 5, 259):
            x, y = _aln_rows(kind, rows, C)
            x, y = x.to(xdt), y.to(ydt)
            yd = y.to(DEV)
            for use_ls in (False, True):
                # add (+ LayerScale) + LayerNorm
                xs = x.to(DEV)
                out = ops.add_layernorm(xs, yd, gd, bd, 1e-6, odt, ls=lsd if use_ls else None)
                new_x, ref = TF.add_layernorm_ref(x, y, ls if use_ls else None, g, b, 1e-6, odt)
                _check_stream(xs, new_x)
                err, tol = maxerr(out, ref), TF.ln_out_tolerance(odt, ref, offset=kind == "offset")
                assert out.dtype == odt and out.shape == x.shape and err <= tol, (kind, rows, use_ls, err, tol)
                # add (+ LayerScale) + cast: the output is the stored stream, cast
                xs = x.to(DEV)
                cast = ops.add_layernorm(xs, yd, None, None, 0.0, odt, ls=lsd if use_ls else None)
                _check_stream(xs, new_x)
                assert cast.dtype == odt and torch.equal(cast, xs.to(odt)), (kind, rows, use_ls)
            # LayerNorm only: the stream comes back bit-identical
            xs = x.to(DEV)
            out = ops.add_layernorm(xs, None, gd, bd, 1e-5, odt)
            _, ref = TF.add_layernorm_ref(x, None, None, g, b, 1e-5, odt)
            assert torch.equal(bits(xs), bits(x))
            err, tol = maxerr(out, ref), TF.ln_out_tolerance(odt, ref, offset=kind == "offset")
            assert out.dtype == odt and err <= tol, (kind, rows, err, tol)


def _aln_raw(x, y, ls, g, b, out, rows, C, xs, ys, os_, eps=1e-6, x_off=0, xdt=None, ydt=None):
    p = lambda t: None if t is None else t.data_ptr()
    rc = _L().load().roma_add_layernorm(x.data_ptr() + x_off, _code(xdt or x.dtype), xs, p(y), _code(ydt or y.dtype) if y is not None else 0, ys,
                                        p(ls), p(g), p(b), out.data_ptr(), _code(out.dtype), os_, rows, C, eps, _stream())
    torch.cuda.synchronize()
    return rc


SENTINEL = -12345.0


def _pitched(t, stride):
    buf = torch.full((t.shape[0], stride), SENTINEL, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf


@pytest.mark.parametrize("pads", [(8, 64, 8), (64, 8, 64)])
@pytest.mark.parametrize("xdt,ydt,odt,C", [(F32, F16, F16, 520), (F16, F16, F32, 96), (BF16, BF16, BF16, 2040), (F32, F32, F32, 1544),
                                           (F32, BF16, F16, 1024)])
def test_add_layernorm_pitched_rows_equal_dense_and_leave_the_gaps(xdt, ydt, odt, C, pads):
    rows = 37
    x, y = _aln_rows("normal", 259, C)
    x, y = x[:rows].to(xdt).to(DEV), y[:rows].to(ydt).to(DEV)
    ls, g, b = (t.to(DEV) for t in _aln_affine(C))
    for gamma, beta in ((g, b), (None, None)):
        dense_x = x.clone()
        dense_out = _ops().add_layernorm(dense_x, y, gamma, beta, 1e-6, odt, ls=ls)
        px, py, po = _pitched(x, C + pads[0]), _pitched(y, C + pads[1]), torch.full((rows, C + pads[2]), SENTINEL, dtype=odt, device=DEV)
        before = [t.clone() for t in (px, py, po)]
        assert _aln_raw(px, py, ls, gamma, beta, po, rows, C, C + pads[0], C + pads[1], C + pads[2]) == 0
        assert torch.equal(bits(px[:, :C]), bits(dense_x)) and torch.equal(bits(po[:, :C]), bits(dense_out))
        assert torch.equal(bits(py), bits(before[1]))
        for buf, old in ((px, before[0]), (po, before[2])):
            assert torch.equal(bits(buf[:, C:]), bits(old[:, C:]))                              # every gap byte as it was


def test_add_layernorm_refusals_launch_nothing():
    L = _L()
    C = 96
    x = torch.randn(4, 2064, device=DEV)
    x16 = x.half()
    y = torch.randn(4, 2064, device=DEV)
    out = torch.full((4, 2064), SENTINEL, device=DEV)
    v = torch.ones(2064, device=DEV)
    x0, x16_0, out0 = x.clone(), x16.clone(), out.clone()
    cases = [
        ("C % 8", L.ROMA_E_SHAPE, dict(C=12)),
        ("C = 2056", L.ROMA_E_SHAPE, dict(C=2056)),
        ("x stride < C", L.ROMA_E_SHAPE, dict(xs=88)),
        ("y stride < C", L.ROMA_E_SHAPE, dict(ys=88)),
        ("out stride < C", L.ROMA_E_SHAPE, dict(os_=88)),
        ("x stride % 8", L.ROMA_E_SHAPE, dict(xs=100)),
        ("out stride % 8", L.ROMA_E_SHAPE, dict(os_=100)),
        ("x base + 8 bytes", L.ROMA_E_ALIGN, dict(x_off=8)),
        ("gamma without beta", L.ROMA_E_ARG, dict(b=None)),
        ("beta without gamma", L.ROMA_E_ARG, dict(g=None)),
    ]
    for name, code, kw in cases:
        a = dict(x=x, y=y, ls=v, g=v, b=v, out=out, rows=4, C=C, xs=2064, ys=2064, os_=2064)
        a.update(kw)
        assert _aln_raw(**a) == code, name
        assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(out), bits(out0)), name
    # a 16-bit stream takes a branch of its own dtype only
    assert _aln_raw(x16, y, v, v, v, out, 4, C, 2064, 2064, 2064) == L.ROMA_E_UNSUPPORTED
    assert torch.equal(bits(x16), bits(x16_0)) and torch.equal(bits(out), bits(out0))
    with pytest.raises(ValueError):
        _ops().add_layernorm(x16[:, :C].contiguous(), y[:, :C].contiguous(), v[:C].contiguous(), v[:C].contiguous(), 1e-6, F16)


# ---- attention ---------------------------------------------------------------------------------------------------------------------
DT16 = [F16, BF16]
NOISE_SHAPES = [(1, 1), (17, 17), (64, 64), (65, 65), (129, 129), (128, 1), (128, 63), (128, 64), (192, 65), (192, 128), (256, 129), (200, 137)]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _big_batch(H):
    """the smallest B at which a two-slab sequence (128 < N <= 256) is given the 128-query kernel: 2 * B * H >= CU count"""
    return -(-_cus() // (2 * H))


def _att_close(out, ref, dtype):
    assert out.dtype == dtype and out.shape[1:] == ref.shape[1:]
    err, tol = maxerr(out, ref.expand(out.shape[0], -1, -1)), TF.att_tolerance(dtype, ref)
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("N,nv", NOISE_SHAPES)
def test_attention_noise_vs_fp64(N, nv, dtype):
    qkv = TF.noise_attention(1, N, 2, dtype)
    _att_close(_ops().attention(qkv.to(DEV), nv), TF.attention_ref(qkv, nv), dtype)


@pytest.mark.parametrize("dtype", DT16)
def test_attention_both_instantiations_at_a_ragged_length(dtype):
    """N = 200, 137 keys, 4 heads: B = 1 gives 2 * 4 workgroups of 128 queries, fewer than the CU count -> the 64-query kernel;
    B = ceil(CUs / 8) (32 on 256 CUs) gives at least the CU count -> the 128-query kernel, whose second workgroup per head has a
    16-query slab that starts past N."""
    assert "ROMA_ATT_QS" not in os.environ, "ROMA_ATT_QS forces one instantiation; this test needs the library's own choice"
    cus, H = _cus(), 4
    B = _big_batch(H)
    assert 2 * 1 * H < cus <= 2 * B * H
    print(f"CU count {cus}: B = 1 -> 64-query kernel, B = {B} -> 128-query kernel")
    qkv = TF.noise_attention(1, 200, H, dtype)
    ref = TF.attention_ref(qkv, 137)
    _att_close(_ops().attention(qkv.to(DEV), 137), ref, dtype)
    big = _ops().attention(qkv.to(DEV).expand(B, -1, -1, -1, -1).contiguous(), 137)
    _att_close(big, ref, dtype)                                                                # every batch entry
    assert torch.equal(big, big[:1].expand_as(big))


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("N,nv", [(200, 137), (192, 128)])
@pytest.mark.parametrize("big", [False, True])
def test_attention_padding_rows_are_never_read_as_keys(N, nv, big, dtype):
    """NaN, or +-6e4, in rows >= n_valid of q, k and v: the real rows come out finite and bit-identical to the run with zero padding —
    pad keys / values are never loaded, and a pad query shares nothing but the wave-uniform `grew` flag with the real ones."""
    H = 4
    B = _big_batch(H) if big else 1
    base = TF.noise_attention(1, N, H, dtype).to(DEV).expand(B, -1, -1, -1, -1).contiguous()
    base[:, nv:] = 0
    want = _ops().attention(base, nv)[:, :nv]
    sign = (torch.rand(base[:, nv:].shape, generator=torch.Generator().manual_seed(5)) < 0.5).to(DEV)
    for fill in (torch.full_like(base[:, nv:], float("nan")), torch.where(sign, 6e4, -6e4).to(dtype)):
        poisoned = base.clone()
        poisoned[:, nv:] = fill
        got = _ops().attention(poisoned, nv)[:, :nv]
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("N,Nk", TF.ONE_HOT_SHAPES)
def test_attention_one_hot_rows_return_their_own_value(N, Nk, dtype):
    """Query i scores 30 nats more on key i mod Nk than on any other valid key (asserted in test_transformer_ref.py), so p rounds to
    exactly 1 there and everything else is at most e^-30: row i is v[i mod Nk] to one ulp of the storage type, element by element.
    Checks every key position of a tile, the last valid key of a masked tile and the refusal of the (winning, 1000-valued) pad keys."""
    qkv = TF.one_hot_attention(N, Nk, dtype)
    out = _ops().attention(qkv.to(DEV), Nk).cpu().double()
    want = TF.one_hot_expected(qkv, Nk).double()
    bad = (out - want).abs() > TF.ULP[dtype] * want.abs()
    assert not bool(bad.any()), f"rows {sorted(set(bad.nonzero()[:, 1].tolist()))[:16]} differ from v[i mod Nk]"


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("N,Nk", TF.RAMP_SHAPES)
def test_attention_ramp_moves_the_running_maximum_every_tile_or_never(N, Nk, sign, dtype):
    qkv = TF.ramp_attention(N, Nk, dtype, sign)
    _att_close(_ops().attention(qkv.to(DEV), Nk), TF.attention_ref(qkv, Nk), dtype)


def _att_raw(q, k, v, o, Nq, Nk, B=1, H=2, d=64, dtype=None, **strides):
    s = dict(q_sb=Nq * H * 64, q_sn=H * 64, q_sh=64, k_sb=Nk * H * 64, k_sn=H * 64, k_sh=64, v_sb=Nk * H * 64, v_sn=H * 64, v_sh=64,
             o_sb=Nq * H * 64, o_sn=H * 64, o_sh=64)
    s.update(strides)
    rc = _L().load().roma_attention_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Nq, Nk, d,
                                        *(s[n] for n in ("q_sb", "q_sn", "q_sh", "k_sb", "k_sn", "k_sh", "v_sb", "v_sn", "v_sh", "o_sb", "o_sn", "o_sh")),
                                        TF.ATT_SCALE, _code(dtype or q.dtype), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DT16)
def test_attention_separate_buffers_with_fewer_keys_than_queries(dtype):
    g = torch.Generator().manual_seed(41)
    q = (torch.randn(1, 100, 2, 64, generator=g) * 1.5).to(dtype)
    k, v = ((torch.randn(1, 37, 2, 64, generator=g) * 1.5).to(dtype) for _ in range(2))
    o = torch.full((1, 100, 128), SENTINEL, dtype=dtype, device=DEV)
    assert _att_raw(q.to(DEV), k.to(DEV), v.to(DEV), o, 100, 37) == 0
    p = torch.softmax(q.double().permute(0, 2, 1, 3) @ k.double().permute(0, 2, 3, 1) * TF.ATT_SCALE, dim=-1)
    ref = (p @ v.double().permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(1, 100, 128)
    _att_close(o, ref, dtype)


def test_attention_refusals_launch_nothing():
    L = _L()
    q, k, v = (torch.randn(1, 64, 2, 64, device=DEV).half() for _ in range(3))
    o = torch.full((1, 64, 128), SENTINEL, dtype=F16, device=DEV)
    o0 = o.clone()
    assert _att_raw(q, k, v, o, 64, 64, d=32) == L.ROMA_E_UNSUPPORTED
    assert _att_raw(q, k, v, o, 64, 64, dtype=F32) == L.ROMA_E_DTYPE
    assert _att_raw(q, k, v, o, 32, 32, q_sn=132) == L.ROMA_E_ALIGN
    assert _att_raw(q, k, v, o, 32, 32, o_sh=60) == L.ROMA_E_ALIGN
    assert torch.equal(bits(o), bits(o0))
    qkv = torch.randn(1, 64, 3, 2, 64, device=DEV).half()
    for nv in (0, 65, -1):
        with pytest.raises(ValueError):
            _ops().attention(qkv, nv, out=o)
    with pytest.raises(ValueError):
        _ops().attention(torch.randn(1, 64, 3, 2, 32, device=DEV).half())
    with pytest.raises(ValueError):
        _ops().attention(qkv.float())
    assert torch.equal(bits(o), bits(o0))
    assert torch.equal(_ops().attention(qkv, 64), _ops().attention(qkv))


# ---- the block runner --------------------------------------------------------------------------------------------------------------
ATT_SETTINGS = ["sdpa", True]
N_REAL, N_PAD, DIM = 200, 256, 128


@contextlib.contextmanager
def _attention(setting):
    import roma_amd.transformer as TR
    old = TR.ATTENTION_KERNEL
    TR.ATTENTION_KERNEL = setting
    try:
        yield TR
    finally:
        TR.ATTENTION_KERNEL = old


def _errs(a, ref):
    d = a.detach().double().cpu() - ref.double().cpu()
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def _no_worse(name, fused, unfused):
    """the fused path's rms and max error against fp64 are at most twice the unfused torch path's"""
    print(f"{name}: fused rms {fused[0]:.3e} max {fused[1]:.3e}; unfused rms {unfused[0]:.3e} max {unfused[1]:.3e}")
    assert fused[0] <= 2 * unfused[0] and fused[1] <= 2 * unfused[1], (name, fused, unfused)


def _tokens(seed, n=N_REAL, pad=N_PAD, garbage=False):
    """(2, pad, DIM) fp32 on the CPU: n real rows, then padding rows of zeros or of 1e3 * N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(2, pad, DIM)
    t[:, :n] = torch.randn(2, n, DIM, generator=g)
    if garbage:
        t[:, n:] = 1e3 * torch.randn(2, pad - n, DIM, generator=g)
    return t


def _dino_stack(dtype):
    from roma_amd.transformer import Block
    blocks = TF.init_module(nn.ModuleList([Block(DIM, 2, qkv_bias=True, init_values=1.0, ln_eps=1e-6) for _ in range(3)]), 1)
    norm = TF.init_module(nn.LayerNorm(DIM, eps=1e-6), 2)
    return blocks.to(dtype).to(DEV), norm.to(dtype).to(DEV)


def _decoder(dtype):
    """(fp32 module, its copy with 16-bit Linear weights and fp32 LayerNorms: what the matcher runs in the 16-bit modes)"""
    from roma_amd.transformer import Block, TransformerDecoder
    td32 = TF.init_module(TransformerDecoder(nn.Sequential(*[Block(DIM, 2) for _ in range(3)]), DIM, 65), 3).to(DEV)
    td16 = copy.deepcopy(td32)
    for m in td16.modules():
        if isinstance(m, nn.Linear):
            m.to(dtype)
    return td32, td16


def _run_dino_fused(TR, blocks, norm, x16):
    params, fin = TR._seam_params(blocks, norm)
    return TR.run_blocks_fused(list(blocks), params, x16.clone(), N_REAL, x16.dtype, final=fin)[:, :N_REAL]


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("att", ATT_SETTINGS)
def test_dino_style_stack_fused_vs_literal_block(att, dtype):
    """3 DINOv2-style blocks + final LayerNorm, 16-bit stream, 200 tokens row-padded to 256, against block_stack_ref (fp64); the bound is
    the error of the unfused torch path of the same modules (`t = blk(t, n_valid)`, then the norm), which rounds in the same places.
    Measured on MI355X, error against fp64 as rms / max, fused | unfused:
      fp16 sdpa 1.162e-3 / 7.27e-3 | 1.157e-3 / 7.30e-3      fp16 hip 1.157e-3 / 8.73e-3 | 1.151e-3 / 7.19e-3
      bf16 sdpa 9.172e-3 / 6.08e-2 | 9.160e-3 / 6.08e-2      bf16 hip 9.171e-3 / 6.08e-2 | 9.173e-3 / 6.08e-2"""
    blocks, norm = _dino_stack(dtype)
    x16 = _tokens(21).to(dtype).to(DEV)
    ref = TF.block_stack_ref(blocks, x16, N_REAL, norm)[:, :N_REAL]
    with _attention(att) as TR:
        fused = _run_dino_fused(TR, blocks, norm, x16)
        t = x16
        for blk in blocks:
            t = blk(t, N_REAL)
        unfused = norm(t)[:, :N_REAL]
    assert fused.dtype == dtype and fused.shape == (2, N_REAL, DIM)
    _no_worse(f"dino {dtype} att={att}", _errs(fused, ref), _errs(unfused, ref))


def _decoder_ref(td16, tokens):
    return TF.linear64(td16.to_out, TF.block_stack_ref(td16.blocks, tokens, None, None))


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("att", ATT_SETTINGS)
def test_decoder_style_stack_fused_vs_literal_block(att, dtype):
    """3 plain blocks inside a TransformerDecoder with 16-bit GEMM weights: fp32 stream, no LayerScale, no final norm, logits through
    to_out; against block_stack_ref + to_out in fp64.  The bound is the error of the same blocks under torch.autocast on fp32 tokens.
    Measured on MI355X, error of the logits against fp64 as rms / max, fused | unfused:
      fp16 sdpa 5.26e-3 / 3.26e-2 | 5.34e-3 / 3.26e-2        fp16 hip 5.32e-3 / 3.06e-2 | 5.33e-3 / 3.58e-2
      bf16 sdpa 4.27e-2 / 2.97e-1 | 4.26e-2 / 3.04e-1        bf16 hip 4.27e-2 / 3.36e-1 | 4.27e-2 / 3.36e-1"""
    td32, td16 = _decoder(dtype)
    tokens = _tokens(22)[:, :N_REAL].contiguous()
    ref = _decoder_ref(td16, tokens)
    with _attention(att):
        fused = td16.forward_rows(tokens.to(DEV))
        with torch.autocast("cuda", dtype):
            unfused = td32.to_out(td32.blocks(tokens.to(DEV)))
    assert fused.dtype == dtype and unfused.dtype == dtype and fused.shape == (2, N_REAL, 65)
    _no_worse(f"decoder {dtype} att={att}", _errs(fused, ref), _errs(unfused, ref))


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("att", ATT_SETTINGS)
def test_padding_rows_cannot_reach_a_real_token(att, dtype):
    """Zero padding rows against 1e3 * N(0, 1) padding rows: the real tokens' outputs are bit-identical.  (A GEMM's output row does not
    depend on the other rows' values at a fixed shape; attention never reads a pad key.)"""
    blocks, norm = _dino_stack(dtype)
    _, td16 = _decoder(dtype)
    clean, dirty = _tokens(23), _tokens(23, garbage=True)
    assert torch.equal(clean[:, :N_REAL], dirty[:, :N_REAL]) and not torch.equal(clean, dirty)
    with _attention(att) as TR:
        a = _run_dino_fused(TR, blocks, norm, clean.to(dtype).to(DEV))
        b = _run_dino_fused(TR, blocks, norm, dirty.to(dtype).to(DEV))
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        a = td16.forward_rows(clean.to(DEV), n_valid=N_REAL, owned=True)
        b = td16.forward_rows(dirty.to(DEV), n_valid=N_REAL, owned=True)
        assert a.shape == (2, N_REAL, 65) and bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("dtype", DT16)
def test_forward_rows_buffer_paths_agree_and_respect_ownership(dtype):
    td32, td16 = _decoder(dtype)
    # 200 real tokens: F.pad of the caller's unpadded rows == the caller's own row-padded buffer, updated in place
    padded = _tokens(24).to(DEV)
    short = padded[:, :N_REAL].contiguous()
    keep = short.clone()
    via_pad = td16.forward_rows(short)
    assert torch.equal(bits(short), bits(keep))
    not_owned = td16.forward_rows(padded, n_valid=N_REAL)                                      # n % 128 != 0: F.pad again
    assert torch.equal(bits(padded), bits(_tokens(24)))
    owned = td16.forward_rows(padded, n_valid=N_REAL, owned=True)
    assert via_pad.shape == (2, N_REAL, 65) and torch.equal(via_pad, owned) and torch.equal(via_pad, not_owned)
    # 256 real tokens: the clone path leaves the caller's tensor alone and equals the in-place path
    full = _tokens(25, n=N_PAD).to(DEV)
    keep = full.clone()
    cloned = td16.forward_rows(full)
    assert torch.equal(bits(full), bits(keep))
    owned = td16.forward_rows(full, owned=True)
    assert cloned.shape == (2, N_PAD, 65) and torch.equal(cloned, owned)
    # fp32 weights: the plain module
    assert torch.equal(td32.forward_rows(keep, n_valid=N_REAL), td32.to_out(td32.blocks(keep[:, :N_REAL])))
    assert torch.equal(td32.forward_rows(keep), td32.to_out(td32.blocks(keep)))


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("att", ATT_SETTINGS)
@pytest.mark.parametrize("hw", [(70, 70), (84, 56)])
def test_dino_vit_fused_branch_vs_its_fp32_branch(hw, att, dtype):
    """DinoViT.patch_tokens, 16-bit fused branch, against the module's own fp32 branch; (84, 56) takes the interpolated, non-square
    position table.  Bound: the error of the unfused 16-bit blocks on the same tokens, as above.  Measured on MI355X (rms, fused |
    unfused): fp16 1.66e-3 | 1.66e-3 at (70, 70), 1.56e-3 | 1.56e-3 at (84, 56); bf16 1.25e-2 | 1.25e-2 and 1.36e-2 | 1.36e-2; the
    maxima coincide (1.1e-2 fp16, 7.8e-2 / 7.4e-2 bf16)."""
    from roma_amd.transformer import DinoViT
    vit32 = TF.init_module(DinoViT(img_size=70, patch_size=14, dim=DIM, depth=2, heads=2), 5).to(DEV)
    vit16 = copy.deepcopy(vit32).to(dtype)
    x = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(26)).to(DEV)
    n = (hw[0] // 14) * (hw[1] // 14) + 1
    ref = vit32.patch_tokens(x)
    assert ref.shape == (2, n - 1, DIM)
    with _attention(att):
        fused = vit16.patch_tokens(x.to(dtype))
        t = vit16.patch_embed(x.to(dtype))
        t = torch.cat((vit16.cls_token.expand(2, -1, -1), t), dim=1) + vit16.pos_encoding(hw[0], hw[1], t.dtype)
        t = F.pad(t, (0, 0, 0, -n % 128))
        for blk in vit16.blocks:
            t = blk(t, n)
        unfused = vit16.norm(t[:, 1:n])
    assert fused.dtype == dtype and fused.shape == (2, n - 1, DIM)                             # class token and padding dropped
    _no_worse(f"vit {hw} {dtype} att={att}", _errs(fused, ref), _errs(unfused, ref))
