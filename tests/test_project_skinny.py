"""ops.project_skinny (the decoder's 64 -> 9 and 128 -> 64 projections as a streaming MFMA kernel) against an fp64 product of the
rounded operands.  Per element the bound is the final rounding plus fp32 accumulation:
    eps * |ref| + K * 2^-24 * sum_k |a_k * w_k| + 2^-24 (one fp16 denormal),
eps = half a unit in the last place: 2^-11 for fp16 (11-bit significand) and 2^-8 for bf16 (8-bit significand: no bf16 result, the
GEMM library's included, can promise 2^-11; measured on MI355X, the largest error / bound is 0.97 for fp16 and 0.98 for bf16).
Decoder.project's choice between this kernel and the GEMM library is project_impl, whose table has a CPU test here."""
import pytest
import torch
import torch.nn as nn

torch.set_grad_enabled(False)
DEV = "cuda"
GUARD = 256
SENTINEL = -7.25
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
PITCH = {9: 24, 64: 144}                                         # the concat buffers of the scale-1 and scale-2 refiners


def _ops():
    from roma_amd import ops
    return ops


def _bound(ref, absum, K, dtype):
    return EPS[dtype] * ref.abs() + K * 2.0 ** -24 * absum + 2.0 ** -24


def _operands(K, N, M, dtype, gen):
    rows = torch.randn((M, K), generator=gen).to(dtype)
    wt = (torch.randn((K, N), generator=gen) / K ** 0.5).to(dtype)
    bias = torch.randn((N,), generator=gen).to(dtype)
    ref = rows.double() @ wt.double() + bias.double()
    absum = rows.double().abs() @ wt.double().abs()
    return rows, wt, bias, ref, absum


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 15, 17, 874])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,N", [(64, 9), (128, 64)])
def test_project_skinny_vs_fp64(K, N, dtype, M):
    ops = _ops()
    gen = torch.Generator().manual_seed(K + M)
    rows, wt, bias, ref, absum = _operands(K, N, M, dtype, gen)
    pitch, extra = PITCH[N], 3                                   # three more rows behind the M that are written
    n = (M + extra) * pitch
    flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    orig = flat.clone()
    buf = flat[GUARD:GUARD + n].view(M + extra, pitch)
    wp, bp = ops.project_skinny_pack(wt.to(DEV), bias.to(DEV))
    assert wp.shape == ((N + 15) // 16 * 16, K) and bp.dtype == torch.float32
    ops.project_skinny(rows.to(DEV), wp, bp, N, buf[:M, :N])
    torch.cuda.synchronize()
    err = (buf[:M, :N].double().cpu() - ref).abs()
    bound = _bound(ref, absum, K, dtype)
    print(f"K={K} N={N} {dtype} M={M}: max err {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    bits = lambda t: t.contiguous().view(torch.int16)
    o = orig[GUARD:GUARD + n].view(M + extra, pitch)
    assert torch.equal(bits(buf[:M, N:]), bits(o[:M, N:])), "columns behind N were written"
    assert torch.equal(bits(buf[M:]), bits(o[M:])), "rows outside [0, M) were written"
    assert torch.equal(bits(flat[:GUARD]), bits(orig[:GUARD])) and torch.equal(bits(flat[GUARD + n:]), bits(orig[GUARD + n:])), "guard region written"


def _decoder(K, N, gen):
    from roma_amd.matcher import Decoder
    conv, bn = nn.Conv2d(K, N, 1), nn.BatchNorm2d(N)
    bn.running_mean.copy_(torch.randn(N, generator=gen) * 0.1)
    bn.running_var.copy_(torch.rand(N, generator=gen) + 0.5)
    bn.weight.copy_(torch.rand(N, generator=gen) + 0.5)
    bn.bias.copy_(torch.randn(N, generator=gen) * 0.1)
    return Decoder(None, None, nn.ModuleDict({"s": nn.Sequential(conv, bn)}), None).to(DEV).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["planar", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,N", [(64, 9), (128, 64)])
def test_decoder_project_takes_the_library_for_planar_maps_and_the_kernel_for_channels_last(K, N, dtype, layout):
    from roma_amd.matcher import project_impl
    gen = torch.Generator().manual_seed(K)
    dec = _decoder(K, N, gen)
    B, h, w = 2, 19, 23
    f = torch.randn((B, K, h, w), generator=gen).to(dtype).to(DEV)
    if layout == "channels_last":
        f = f.contiguous(memory_format=torch.channels_last)
    if layout == "planar":                                       # (what channels-last maps take is test_project_impl_table's to pin)
        assert project_impl(dtype, False, K, N, PITCH[N]) == "gemm"
    buf = torch.full((B, h, w, PITCH[N]), SENTINEL, dtype=dtype, device=DEV)
    x = dec.project("s", f, dtype, out=buf[..., :N])
    assert x.shape == (B, N, h, w) and x.data_ptr() == buf.data_ptr()
    y = dec.project("s", f, dtype)                               # no destination given: project allocates one
    wt, b = dec.folded_proj(dtype)["s"]
    a = f.permute(0, 2, 3, 1).reshape(-1, K).double().cpu()
    ref = a @ wt.double().cpu() + b.double().cpu()
    bound = _bound(ref, a.abs() @ wt.double().abs().cpu(), K, dtype)
    for got in (x, y):
        err = (got.permute(0, 2, 3, 1).reshape(-1, N).double().cpu() - ref).abs()
        print(f"K={K} N={N} {dtype} {layout}: max err {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
    assert (buf[..., 16 if N < 16 else N:] == SENTINEL).all()    # the library path at N = 9 stores 16 columns: the next 7 are the refiner's to overwrite


def test_project_impl_table():
    from roma_amd.matcher import project_impl
    h, b, f = torch.float16, torch.bfloat16, torch.float32
    for dt in (h, b):
        assert project_impl(dt, True, 64, 9, 24) == "skinny"
        assert project_impl(dt, True, 128, 64, 144) == "skinny"
        assert project_impl(dt, True, 64, 9, 16) == "skinny"
        assert project_impl(dt, False, 64, 9, 24) == "gemm"      # planar feature map
        assert project_impl(dt, False, 128, 64, 144) == "gemm"
        assert project_impl(dt, True, 64, 9, 9) == "gemm"        # rows the kernel cannot store packets to
        for K, N, P in ((512, 256, 576), (1024, 512, 1152), (1024, 512, 1408), (64, 64, 144), (128, 9, 24)):
            assert project_impl(dt, True, K, N, P) == "gemm"     # scales 4, 8, 16 and anything that is not one of the two pairs
    assert project_impl(f, True, 64, 9, 24) == "gemm" and project_impl(f, True, 128, 64, 144) == "gemm"


def test_assemble_impl_table():
    from roma_amd.matcher import assemble_impl
    for dt in (torch.float16, torch.bfloat16):
        for C, E, D, Dp in ((9, 6, 24, 24), (64, 16, 144, 144), (256, 32, 569, 576), (512, 64, 1137, 1152), (512, 128, 1377, 1408)):
            assert assemble_impl(dt, True, Dp, C, E, D, Dp) == "fused"               # y is x inside the buffer
            assert assemble_impl(dt, False, C, C, E, D, Dp) == "split"               # planar y
            assert assemble_impl(torch.float32, True, Dp, C, E, D, Dp) == "split"
        assert assemble_impl(dt, True, 16, 9, 6, 24, 24) == "fused"
        assert assemble_impl(dt, True, 9, 9, 6, 24, 24) == "split"                   # a 9-channel y of pitch 9: no packets
        assert assemble_impl(dt, True, 8, 9, 6, 24, 24) == "split"
        assert assemble_impl(dt, True, 24, 12, 8, 32, 32) == "split"                 # C not whole packets and not the scale-1 pixel
