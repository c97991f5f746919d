"""ops.refiner_block_mid (one launch: depthwise 5x5 + BN + ReLU + 1x1 at 32 < C <= 160) against the two calls it joins,
ops.pointwise_mfma(ops.dwconv5x5_bn_relu(x)), on the same operands.  The one-launch kernel runs the two kernels' own device code
(roma_amd/csrc/refiner_mid_device.h), so the comparison is of BITS; one case is also held against torch so that the project is not
only compared with itself.  Input and output sit inside sentinel guards as in test_refiner_assemble.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GUARD = 256                                  # elements in front of and behind a buffer (a multiple of 8: the buffer stays 16-byte aligned)
SENTINEL = -7.25

WIDTHS = [(144, 144), (144, 160), (40, 40), (152, 152), (160, 160)]           # (C, pitch)
# (B, h, w): less than one strip, every strip a border strip / width no multiple of 8, tiles wrap rows and images / interior and border
# strips in one wave / 59 166 px > 256 x 224: every workgroup of a full grid gets a second tile and the last round is partial
MAPS = [(1, 5, 3), (2, 7, 33), (1, 37, 45), (2, 171, 173)]


def _ops():
    from roma_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _operands(C, dtype, gen):
    """The records of a `split_mfma` row (matcher.BlockOutIn): fp32 taps / scale / shift, the 1x1 zero-padded to 160."""
    w25 = torch.randn(25, C, generator=gen) * 0.2
    scale = torch.rand(C, generator=gen) + 0.5
    shift = torch.randn(C, generator=gen) * 0.3
    wt = torch.zeros(160, 160)
    wt[:C, :C] = torch.randn(C, C, generator=gen) / C ** 0.5
    bias = torch.zeros(160)
    bias[:C] = torch.randn(C, generator=gen) * 0.1
    return w25.to(DEV), scale.to(DEV), shift.to(DEV), wt.to(dtype).to(DEV), bias.to(DEV)


def _guarded(B, h, w, pitch, dtype, fill=None):
    n = B * h * w * pitch
    flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype)
    if fill is not None:
        flat[GUARD:GUARD + n] = fill.reshape(-1)
    flat = flat.to(DEV)
    return flat, flat[GUARD:GUARD + n].view(B, h, w, pitch)


def _two_calls(ops, x, C, w25, scale, shift, wt, bias):
    """The reference: the two launches of the `split_mfma` row on the same (pitched) buffers."""
    B, h, w, pitch = x.shape
    t = torch.zeros_like(x)
    ops.dwconv5x5_bn_relu(x[..., :C].permute(0, 3, 1, 2), w25, scale, shift, out=t[..., :C].permute(0, 3, 1, 2))
    return ops.pointwise_mfma(t.view(B * h * w, pitch), wt, bias, C).view(B, h, w, pitch)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,h,w", MAPS)
@pytest.mark.parametrize("C,pitch", WIDTHS)
def test_refiner_block_mid_has_the_bits_of_the_two_calls(C, pitch, B, h, w, dtype):
    ops = _ops()
    gen = torch.Generator().manual_seed(1000 * C + 10 * h + pitch)
    w25, scale, shift, wt, bias = _operands(C, dtype, gen)
    x_flat, x = _guarded(B, h, w, pitch, dtype, torch.randn((B, h, w, pitch), generator=gen).to(dtype))
    x_orig = x_flat.clone()
    out_flat, out = _guarded(B, h, w, pitch, dtype)
    out_orig = out_flat.clone()

    ref = _two_calls(ops, x, C, w25, scale, shift, wt, bias)
    got = ops.refiner_block_mid(x, w25, scale, shift, wt, bias, C, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isfinite(ref[..., :C].float()).all()

    bad = (_bits(got[..., :C]) != _bits(ref[..., :C])).nonzero()
    for b_, y_, x_, c_ in bad[:8].tolist():
        print(f"differs at b={b_} y={y_} x={x_} channel {c_}: {got[b_, y_, x_, c_].item()!r} vs {ref[b_, y_, x_, c_].item()!r}")
    assert len(bad) == 0, f"{len(bad)} of {ref[..., :C].numel()} elements differ in bits from pointwise_mfma(dwconv5x5_bn_relu(x))"
    n = B * h * w * pitch
    if pitch > C:
        o = out_orig[GUARD:GUARD + n].view(B, h, w, pitch)
        assert torch.equal(_bits(got[..., C:]), _bits(o[..., C:])), "pad channels [C, pitch) of the output written"
    assert torch.equal(_bits(out_flat[:GUARD]), _bits(out_orig[:GUARD])) and \
        torch.equal(_bits(out_flat[GUARD + n:]), _bits(out_orig[GUARD + n:])), "guard region of the output written"
    assert torch.equal(_bits(x_flat), _bits(x_orig)), "input buffer (or its guards) changed"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_refiner_block_mid_vs_torch(dtype):
    """conv2d(groups) + BN + ReLU rounded to the dtype + fp32 matmul on the same rounded operands — the reference and the tolerance of
    test_gpu_ops.py::test_refiner_block_vs_torch."""
    import torch.nn.functional as F
    ops = _ops()
    C, B, h, w = 144, 1, 37, 45
    gen = torch.Generator().manual_seed(C * 1000 + h)
    w25, scale, shift, wt, bias = _operands(C, dtype, gen)
    x = torch.randn(B, h, w, C, generator=gen).to(DEV).to(dtype)
    out = ops.refiner_block_mid(x, w25, scale, shift, wt, bias, C)
    xf = x.float().permute(0, 3, 1, 2)
    t = F.conv2d(xf, w25.t().reshape(C, 1, 5, 5), padding=2, groups=C)
    t = torch.relu(t * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)).to(dtype).float()
    ref = torch.einsum("bkhw,nk->bhwn", t, wt.float()[:C, :C]) + bias[:C]
    tol = 4e-3 if dtype == torch.float16 else 3e-2
    err = (out.float() - ref).abs().max().item()
    assert err < tol * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv_refiner_body_one_launch_equals_two(dtype, monkeypatch):
    """The scale-2 refiner (D = 144 = 2 x 64 features + 16 embedding channels, no local correlation: model_zoo.REFINER_SPEC["2"]; a
    radius of 2 would add 25 channels, which no feature width makes 144) with two hidden blocks on a 19 x 23 map, the decision function
    forced to either answer: the same bits."""
    from roma_amd import matcher
    from roma_amd.matcher import ConvRefiner
    torch.manual_seed(3)
    ref = ConvRefiner(144, 144, 3, hidden_blocks=2, displacement_emb_dim=16, local_corr_radius=None).to(DEV).eval()
    for mod in ref.modules():                                    # non-trivial BN statistics
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    B, C, h, w = 2, 64, 19, 23
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((B, C, h, w), generator=gen).to(DEV)
    y = torch.randn((B, C, h, w), generator=gen).to(DEV)
    flow = (torch.rand((B, 2, h, w), generator=gen) * 2 - 1).to(DEV)
    outs = {}
    for how in ("one", "two"):
        monkeypatch.setattr(matcher, "mid_block_impl", lambda *a, how=how: how)
        cur, P = ref._body(x.to(dtype), y.to(dtype), flow, 1.0, dtype)
        torch.cuda.synchronize()
        assert P.Dp == 144 and cur.shape == (B, h, w, 144)
        outs[how] = cur.clone()
    assert torch.isfinite(outs["two"].float()).all()
    assert torch.equal(_bits(outs["one"]), _bits(outs["two"]))


def test_refiner_block_mid_argument_checks():
    """Aliasing out, C = 168, C = 36 and pitch C + 4 return the error codes and launch nothing (the buffers keep their contents)."""
    from roma_amd import _lib
    lib = _lib.load()
    dtype, C, B, h, w = torch.float16, 144, 1, 6, 9
    gen = torch.Generator().manual_seed(11)
    w25, scale, shift, wt, bias = _operands(160, dtype, gen)     # wide enough for every C below
    x = torch.randn((B, h, w, 176), generator=gen).to(dtype).to(DEV)
    out = torch.full((B, h, w, 176), SENTINEL, dtype=dtype, device=DEV)
    x0 = x.clone()

    def call(xp, yp, C, xpitch, ypitch):
        return lib.roma_refiner_block_mid(xp, w25.data_ptr(), scale.data_ptr(), shift.data_ptr(), wt.data_ptr(), bias.data_ptr(), yp,
                                          B, C, h, w, _lib.ROMA_F16, xpitch, ypitch, None)

    assert call(x.data_ptr(), x.data_ptr(), C, 176, 176) == _lib.ROMA_E_ARG                       # out is x
    assert call(x.data_ptr(), x.data_ptr() + 176 * 2 * 9, C, 176, 176) == _lib.ROMA_E_ARG         # out overlaps x, one image row later
    assert b"overlap" in lib.roma_last_error()
    assert call(x.data_ptr(), out.data_ptr(), 168, 176, 176) == _lib.ROMA_E_UNSUPPORTED
    assert call(x.data_ptr(), out.data_ptr(), 36, 176, 176) == _lib.ROMA_E_UNSUPPORTED
    assert call(x.data_ptr(), out.data_ptr(), C, C + 4, 176) == _lib.ROMA_E_ALIGN
    assert call(x.data_ptr(), out.data_ptr(), C, 176, C + 4) == _lib.ROMA_E_ALIGN
    assert call(x.data_ptr(), out.data_ptr(), C, 176, 176) == 0                                   # and the valid call does run
    torch.cuda.synchronize()
    assert (out[..., :C] != SENTINEL).any() and torch.equal(_bits(out[..., C:]), _bits(torch.full_like(out[..., C:], SENTINEL)))
    bad = torch.full_like(out, SENTINEL)
    for xp, yp, c, px, py in ((x.data_ptr(), x.data_ptr(), C, 176, 176), (x.data_ptr(), bad.data_ptr(), 168, 176, 176),
                              (x.data_ptr(), bad.data_ptr(), 36, 176, 176), (x.data_ptr(), bad.data_ptr(), C, C + 4, 176)):
        assert call(xp, yp, c, px, py) < 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(bad), _bits(torch.full_like(bad, SENTINEL))), "a refused call wrote"
    xc = x[..., :C].contiguous()
    with pytest.raises(ValueError):                              # the wrapper hands the code on
        _ops().refiner_block_mid(xc, w25[:, :C].contiguous(), scale[:C], shift[:C], wt, bias, C, out=xc)
