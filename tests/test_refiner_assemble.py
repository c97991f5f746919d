"""ops.refiner_assemble (one launch: warp of y, displacement embedding, channel padding) against the three calls it replaces, run on a
copy of the same buffer: ops.warp_bilinear and ops.disp_emb (pinned to F.grid_sample and the oracle in test_gpu_ops.py) and zero_().
The new kernels evaluate the old kernels' expressions and round where they round, so the comparison is of BITS (NaN embeddings of
NaN flow included).
Also the one-launch flow + certainty upsample against two ops.interp_bilinear calls."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GUARD = 256                                  # elements in front of and behind the buffer (a multiple of 8: the buffer stays 16-byte aligned)
SENTINEL = -7.25

# (C, E, D, Dp) of the five refiners (scale 1, 2, 4, 8, 16)
LEVELS = [(9, 6, 24, 24), (64, 16, 144, 144), (256, 32, 569, 576), (512, 64, 1137, 1152), (512, 128, 1377, 1408)]
CASES = [(lv, hw) for lv in LEVELS for hw in (((5, 7), (19, 23)) if lv[0] <= 64 else ((5, 7),))]


def _ops():
    from roma_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _flow(B, h, w, gen):
    flow = (torch.rand((B, 2, h, w), generator=gen) * 2.6 - 1.3)
    flat = flow.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=gen)[:12]
    for i, v in zip(idx.tolist(), [1.0, -1.0, 1.0, -1.0, float("nan"), float("nan"), float("inf"), -float("inf"), float("inf"), -float("inf"), 1.0, -1.0]):
        flat[i] = v
    return flow


@pytest.mark.parametrize("source", ["in_buffer", "separate"])
@pytest.mark.parametrize("B,shift", [(2, 1), (4, 2)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("level,hw", CASES)
def test_refiner_assemble_matches_the_three_calls(level, hw, dtype, B, shift, source):
    ops = _ops()
    C, E, D, Dp = level
    h, w = hw
    gen = torch.Generator().manual_seed(1000 * C + 10 * h + B + (source == "separate"))
    n = B * h * w * Dp
    flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype)
    buf_cpu = flat[GUARD:GUARD + n].view(B, h, w, Dp)
    buf_cpu[..., :C] = torch.randn((B, h, w, C), generator=gen).to(dtype)
    flow = _flow(B, h, w, gen).to(DEV)
    we = torch.randn((E, 2), generator=gen).to(DEV)
    be = torch.randn((E,), generator=gen).to(DEV)
    gain = 1.25 * 0.7
    if source == "separate":                                     # its own size and its own pitch
        pitch = 16 if C == 9 else C + 8
        y_store = torch.randn((B, 6, 9, pitch), generator=gen).to(dtype).to(DEV)
    got_flat, ref_flat = flat.to(DEV), flat.to(DEV)
    orig = flat.to(DEV)

    def views(fl):
        buf = fl[GUARD:GUARD + n].view(B, h, w, Dp)
        d = buf.permute(0, 3, 1, 2)
        src = y_store[..., :C].permute(0, 3, 1, 2) if source == "separate" else d[:, :C]
        return buf, d, src

    buf, d, src = views(ref_flat)
    if Dp > D:
        buf[..., D:].zero_()
    ops.warp_bilinear(src, flow, out=d[:, C:2 * C], batch_shift=shift)
    ops.disp_emb(flow, we, be, gain, out=d[:, 2 * C:2 * C + E])
    ref = buf

    buf, d, src = views(got_flat)
    ops.refiner_assemble(buf, src, flow, we, be, gain, C, D, batch_shift=shift)
    torch.cuda.synchronize()
    got = buf

    bad = (_bits(got[..., C:2 * C + E]) != _bits(ref[..., C:2 * C + E])).nonzero()
    for b_, y_, x_, c_ in bad[:8].tolist():                      # what differs, should anything: (pixel, channel), both values, the flow
        print(f"differs at b={b_} y={y_} x={x_} channel {C + c_}: {got[b_, y_, x_, C + c_].item()!r} vs {ref[b_, y_, x_, C + c_].item()!r}, "
              f"flow {flow[b_, :, y_, x_].tolist()}")
    assert len(bad) == 0, f"{len(bad)} warp / embedding elements differ in bits from the separate kernels"
    if Dp > D:
        assert torch.equal(_bits(got[..., D:]), torch.zeros_like(_bits(got[..., D:]))), "padding is not zero"
    o = orig[GUARD:GUARD + n].view(B, h, w, Dp)
    assert torch.equal(_bits(got[..., :C]), _bits(o[..., :C])), "x channels were written"
    keep = D // 8 * 8 if Dp > D else D                           # of the correlation slice only the packet that holds channel D may be touched
    assert torch.equal(_bits(got[..., 2 * C + E:keep]), _bits(o[..., 2 * C + E:keep])), "correlation slice written outside the last packet"
    assert torch.equal(_bits(got_flat[:GUARD]), _bits(orig[:GUARD])) and torch.equal(_bits(got_flat[GUARD + n:]), _bits(orig[GUARD + n:])), \
        "guard region written"
    if source == "separate":
        assert y_store.isfinite().all()


@pytest.mark.parametrize("sizes", [((5, 7), (10, 14)), ((40, 40), (70, 70))])
def test_interp_bilinear_pair_is_two_interp_bilinear_calls(sizes):
    ops = _ops()
    (hi, wi), out = sizes
    gen = torch.Generator().manual_seed(hi)
    flow = torch.randn((2, 2, hi, wi), generator=gen).to(DEV)
    cert = torch.randn((2, 1, hi, wi), generator=gen).to(DEV)
    f, c = ops.interp_bilinear_pair(flow, cert, out)
    assert f.shape == (2, 2, *out) and c.shape == (2, 1, *out)
    assert torch.equal(f, ops.interp_bilinear(flow, out)) and torch.equal(c, ops.interp_bilinear(cert, out))
