"""fp64 truths, per-element bounds and deliberately wrong variants ("mutants") for the decoder's sampling kernels (sampling.hip:
warp, displacement embedding, bilinear resize, flow update, refiner_assemble) and the refiner head (refiner_head.hip).  CPU only;
test_sampling_kernels.py compares the kernels with what is here.

Truths are evaluated in fp64 from the operands as the kernel sees them: sources and activations rounded to their storage type; flow,
embedding weights and head weights in fp32.

Bound, per element:  |out - truth| <= slop + r * |truth| (+ 2^-25 for fp16, the half spacing of its subnormals)
  r     the half spacing of the OUTPUT type relative to the value: 0 (fp32), 2^-11 (fp16), 2^-8 (bf16) - one rounding of the result;
  slop  what evaluating the operation in fp32 costs, measured on the reference and not on the kernel: the worst difference between
        torch's fp32 CPU evaluation of the same operation on the same inputs and the fp64 truth, times SLACK = 4 because the kernel
        orders its fp32 operations differently (fused multiply-adds, another summation order).

What the truths do not define is left out, and counted: F.grid_sample returns NaN where a flow component is NaN or infinite (its
weights become inf - inf), so pixels with a non-finite flow are not compared with the warp truth.  They are the planted entries only
(nonfinite_pixels, at most MAX_EXCLUDED per map); the library's own rule for them - exactly 0 - is asserted separately."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.golden import recipes as R

HALF_SPACING = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUBNORMAL = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
SLACK = 4.0
MAX_EXCLUDED = 12                            # pixels per map whose flow is NaN or infinite
HUGE = 8.0                                   # |flow| beyond this is a planted far-out-of-range entry (the others stay below 2)
F64 = torch.float64


def bound(truth, dtype, slop):
    return slop + HALF_SPACING[dtype] * truth.abs() + SUBNORMAL[dtype]


def slop_of(eval32, truth, where=None):
    """SLACK x the worst |fp32 CPU evaluation - fp64 truth| (over `where`)."""
    d = (eval32.to(F64) - truth).abs()
    if where is not None:
        d = d[where.expand_as(d)]
    return SLACK * float(d.max())


def excess(out, truth, dtype, slop, where=None):
    """The worst |out - truth| / bound (over `where`): <= 1 passes."""
    q = (out.to(F64) - truth).abs() / bound(truth, dtype, slop).clamp_min(1e-300)
    if where is not None:
        q = q[where.expand_as(q)]
    return float(q.max())


# ------------------------------------------------------------------------------------------------ flow with the edges planted
def pixel_of(k, n):
    """The normalised coordinate whose sample position is pixel k of n (align_corners=False)."""
    return (2 * k + 1) / n - 1


def planted_entries(hs, ws):
    """(fx, fy) pairs: the cell edges of a (hs, ws) source, and what is not a position at all."""
    e = 2.0 ** -9                                                # in normalised units: a few thousandths of a pixel, far above fp32 rounding
    inf, nan = math.inf, math.nan
    return [(-1.0, -1.0), (1.0, 1.0), (-1.0, 0.3), (0.2, 1.0),                                       # exactly -1 and +1
            (pixel_of(4, ws), pixel_of(6, hs)), (pixel_of(0, ws), 0.37), (0.11, pixel_of(hs - 1, hs)),  # on integer positions: a weight is 0
            (pixel_of(-1, ws), pixel_of(-1, hs)), (pixel_of(ws, ws), pixel_of(hs, hs)),               # the first position with every tap outside ...
            (pixel_of(-1, ws) - e, 0.1), (pixel_of(ws, ws) + e, 0.1), (0.1, pixel_of(-1, hs) - e), (0.1, pixel_of(hs, hs) + e),  # ... and just beyond
            (inf, 0.1), (0.1, -inf), (nan, 0.1), (0.2, nan), (nan, nan),                              # not positions (the excluded ones)
            (1e30, 0.0), (0.0, -1e30), (-7.0, 0.3), (0.3, -7.0), (-7.0, -7.0)]


@functools.lru_cache(maxsize=None)
def planted_flow(name, B, h, w, hs, ws):
    """(B,2,h,w) fp32: coherent_flow with a pasted adversarial_flow block and planted_entries(hs, ws) at seeded places of every map.
    Shared between tests: treat as read-only."""
    flow = R.coherent_flow(name, B, h, w)
    adv = R.adversarial_flow(name + ".adv", B, h, w, lim=1.3)
    y0, y1, x0, x1 = h // 8, h // 8 + max(2, h // 3), w // 8, w // 8 + max(2, w // 3)
    flow[:, :, y0:y1, x0:x1] = adv[:, :, y0:y1, x0:x1]
    entries = planted_entries(hs, ws)
    rs = R.rs_for(name + ".plant")
    for b in range(B):
        for p, (fx, fy) in zip(rs.permutation(h * w)[:len(entries)], entries):
            flow[b, 0, p // w, p % w] = fx
            flow[b, 1, p // w, p % w] = fy
    return torch.from_numpy(flow)


def nonfinite_pixels(flow):
    """(B,1,h,w) bool: a flow component is NaN or infinite - the pixels the warp truth does not define."""
    return ~flow.isfinite().all(dim=1, keepdim=True)


def huge_pixels(flow):
    """(B,1,h,w) bool: finite flow far outside anything a position can be (1e30, -7)."""
    return flow.isfinite().all(dim=1, keepdim=True) & (flow.abs() > HUGE).any(dim=1, keepdim=True)


def sample_position(flow, hs, ws):
    f = flow.to(F64)
    px, py = ((f[:, 0:1] + 1) * ws - 1) / 2, ((f[:, 1:2] + 1) * hs - 1) / 2
    return px.nan_to_num(-1e6, 1e6, -1e6).clamp(-1e6, 1e6), py.nan_to_num(-1e6, 1e6, -1e6).clamp(-1e6, 1e6)


def tap_classes(flow, hs, ws, margin=1e-4):
    """(outside, ring, inner), each (B,1,h,w) bool, for a (hs, ws) source, whatever way an fp32 evaluation rounds the position (it is
    good to ~1e-6 pixel; margin is in pixels): outside - every tap is outside the source for sure (non-finite flow included);
    inner - every tap that can carry weight is off the source's border ring for sure; ring - the rest."""
    px, py = sample_position(flow, hs, ws)

    def axis(p, n):
        lo, hi = torch.floor(p - margin).clamp_min(0), (torch.floor(p + margin) + 1).clamp_max(n - 1)
        return lo > hi, (lo == 0) | (hi == n - 1)
    ex, rx = axis(px, ws)
    ey, ry = axis(py, hs)
    outside = ex | ey | nonfinite_pixels(flow)
    ring = ~outside & (rx | ry)
    return outside, ring, ~outside & ~ring


# ------------------------------------------------------------------------------------------------ warp
def warp_truth(src, flow, shift=0, dtype=F64, **kw):
    """F.grid_sample of src[(b + shift) % B] at flow: bilinear, zero padding, align_corners=False.  dtype=float32 is the fp32 evaluation
    the slop is measured with; kw overrides a mode (the mutants)."""
    opts = dict(mode="bilinear", padding_mode="zeros", align_corners=False)
    opts.update(kw)
    return F.grid_sample(torch.roll(src.to(dtype), -shift, 0), flow.to(dtype).permute(0, 2, 3, 1), **opts)


def warp_manual(src, flow, shift=0, weights_as=None, accumulate_as=None, swap_xy=False):
    """The same sum written out in fp64, tap by tap in the kernels' order, so that single steps can be made wrong: weights rounded to
    `weights_as`, products and partial sums rounded to `accumulate_as`, x and y of the position exchanged."""
    s = torch.roll(src.to(F64), -shift, 0)
    B, C, hs, ws = s.shape
    px, py = sample_position(flow.flip(1) if swap_xy else flow, hs, ws)
    px, py = px[:, 0], py[:, 0]
    x0, y0 = torch.floor(px), torch.floor(py)
    ax, ay = px - x0, py - y0
    x0, y0 = x0.long(), y0.long()
    bi = torch.arange(B)[:, None, None]
    acc = torch.zeros((B, C) + tuple(px.shape[1:]), dtype=F64)
    for dy, dx, wgt in ((0, 0, (1 - ay) * (1 - ax)), (0, 1, (1 - ay) * ax), (1, 0, ay * (1 - ax)), (1, 1, ay * ax)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < ws) & (yy >= 0) & (yy < hs)
        v = s[bi, :, yy.clamp(0, hs - 1), xx.clamp(0, ws - 1)].permute(0, 3, 1, 2)
        v = torch.where(ok[:, None], v, torch.zeros((), dtype=F64))
        if weights_as is not None:
            wgt = wgt.to(weights_as).to(F64)
        term = wgt[:, None] * v
        if accumulate_as is not None:
            acc = (acc + term.to(accumulate_as).to(F64)).to(accumulate_as).to(F64)
        else:
            acc = acc + term
    return acc


def warp_mutants(dtype):
    """name -> f(src, flow, shift): wrong in one way each."""
    m = {"align_corners=True": lambda s, f, k: warp_truth(s, f, k, align_corners=True),
         "border padding": lambda s, f, k: warp_truth(s, f, k, padding_mode="border"),
         "nearest sampling": lambda s, f, k: warp_truth(s, f, k, mode="nearest"),
         "x / y taps swapped": lambda s, f, k: warp_manual(s, f, k, swap_xy=True),
         "batch shift off by one": lambda s, f, k: warp_truth(s, f, k + 1)}
    if dtype != torch.float32:
        m["weights rounded to the output type"] = lambda s, f, k: warp_manual(s, f, k, weights_as=dtype)
        m["accumulation in the 16-bit type"] = lambda s, f, k: warp_manual(s, f, k, accumulate_as=dtype)
    return m


# ------------------------------------------------------------------------------------------------ displacement embedding
def emb_truth(flow, weight, bias, gain, centre_shift=0.0, drop_gain=False, swap_w=False):
    """b + w0 * gain * (fx - cx) + w1 * gain * (fy - cy), cx = (2x + 1) / W - 1: the oracle's pixel_grid, exactly.  (B,E,h,w) fp64.
    The keywords are the mutants: pixel centre `centre_shift` pixels off, gain dropped, w0 / w1 exchanged."""
    B, _, h, w = flow.shape
    f = flow.to(F64)
    cx = (2 * (torch.arange(w, dtype=F64) + centre_shift) + 1) / w - 1
    cy = (2 * (torch.arange(h, dtype=F64) + centre_shift) + 1) / h - 1
    g = 1.0 if drop_gain else float(np.float32(gain))
    wd = weight.reshape(-1, 2).to(F64)
    w0, w1 = (wd[:, 1], wd[:, 0]) if swap_w else (wd[:, 0], wd[:, 1])
    dx, dy = g * (f[:, 0:1] - cx[None, None, None, :]), g * (f[:, 1:2] - cy[None, None, :, None])
    return bias.to(F64)[None, :, None, None] + w0[None, :, None, None] * dx + w1[None, :, None, None] * dy


def emb_eval32(flow, weight, bias, gain):
    """torch's fp32 evaluation: the oracle's expression (matcher.py:111-120)."""
    from oracle import roma_oracle as O
    B, _, h, w = flow.shape
    return F.conv2d(float(np.float32(gain)) * (flow - O.pixel_grid(B, h, w)), weight.reshape(-1, 2, 1, 1), bias)


def emb_mutants():
    return {"pixel centre off by half a pixel": lambda f, w, b, g: emb_truth(f, w, b, g, centre_shift=0.5),
            "gain dropped": lambda f, w, b, g: emb_truth(f, w, b, g, drop_gain=True),
            "w0 / w1 swapped": lambda f, w, b, g: emb_truth(f, w, b, g, swap_w=True)}


FMAX = {torch.float32: 3.4028234663852886e38, torch.float16: 65504.0, torch.bfloat16: 3.3895313892515355e38}


def emb_check(out, truth, flow, dtype, slop):
    """Asserts an embedding against its truth, every element:
      ordinary flow  the bound above;
      huge flow      (1e30, -7: one term dominates, so the absolute slop measured at O(1) says nothing) the fp32 evaluation is the
                     difference, the gain and two multiply-adds, each within 2^-24 of a magnitude the result bounds up to the factor the
                     smaller terms add: 8 * 2^-24 * |truth| + r * |truth|; beyond the type's largest number the infinity of that sign;
      infinite flow  the truth's infinity, or NaN where it is NaN (inf - inf);
      NaN flow       NaN - and NaN nowhere else.
    Returns the worst |out - truth| / bound over the ordinary elements."""
    out = out.detach().to(F64).cpu()
    nf, hg = nonfinite_pixels(flow).expand_as(truth), huge_pixels(flow).expand_as(truth)
    ordinary = ~nf & ~hg
    worst = excess(out, truth, dtype, slop, ordinary)
    assert worst <= 1.0, f"embedding is {worst:.2f} x its bound away from the truth"
    over = hg & (truth.abs() > FMAX[dtype])
    big = hg & ~over
    assert bool(((out - truth).abs()[big] <= ((8 * 2.0 ** -24 + HALF_SPACING[dtype]) * truth.abs() + slop + SUBNORMAL[dtype])[big]).all())
    assert torch.equal(out[over], torch.copysign(torch.full_like(truth[over], math.inf), truth[over]))
    assert torch.equal(out.isnan(), truth.isnan()), "NaN where the truth has none, or none where it has"
    nan_flow = flow.isnan().any(dim=1, keepdim=True).expand_as(truth)
    assert bool(out.isnan()[nan_flow].all()) and not bool(out.isnan()[~nf].any()), "NaN flow must give NaN in its pixel, and only there"
    inf_ = nf & ~truth.isnan()
    assert torch.equal(out[inf_], truth[inf_])
    return worst


# ------------------------------------------------------------------------------------------------ resize
def interp_truth(x, size, dtype=F64):
    return F.interpolate(x.to(dtype), size=size, mode="bilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ flow update / refiner head
def update_truth(flow, cert, delta, sx, sy, dtype=F64, swap_s=False):
    """flow + (sx * delta0, sy * delta1), (cert or 0) + delta2 - sampling.hip flow_update_kernel / matcher.py:397-402."""
    sx, sy = float(np.float32(sx)), float(np.float32(sy))
    if swap_s:
        sx, sy = sy, sx
    d = delta.to(dtype)
    f = flow.to(dtype) + torch.stack((sx * d[:, 0], sy * d[:, 1]), dim=1)
    c = d[:, 2:3] if cert is None else cert.to(dtype) + d[:, 2:3]
    return f, c


def head_truth(x, wo, bo, flow, cert, sx, sy, dtype=F64, row_shift=0, swap_s=False):
    """refiner_head.hip's header: d[m] = bo + sum_k x[m][k] * wo[k], then update_truth.  x (B,h,w,pitch) of which wo.shape[0] channels
    count.  Returns (flow, certainty, delta (B,3,h,w)).  row_shift rolls wo's rows (a mutant)."""
    C = wo.shape[0]
    d = (x[..., :C].to(dtype) @ torch.roll(wo, row_shift, 0).to(dtype) + bo.to(dtype)).permute(0, 3, 1, 2)
    f, c = update_truth(flow, cert, d, sx, sy, dtype, swap_s)
    return f, c, d
