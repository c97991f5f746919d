"""The decoder's sampling kernels (sampling.hip) and the refiner head (refiner_head.hip) against fp64 truths, kernel by kernel, at the
widths, layouts and alignments the product uses.  Truths, bounds and mutants: tests/sampling_ref.py.

Every comparison is per element, |out - truth| <= slop + r * |truth|: r the half spacing of the output type, slop 4 x the worst
difference of torch's fp32 CPU evaluation from the fp64 truth on the same inputs.  Each test prints that reference error and the
kernel's own worst error; the CPU tests show that the bound is tight enough to tell every mutant of sampling_ref.py from the truth
by a factor of 10 at least.

The library's rule for samples without a source, pinned here: a sample whose four taps are outside the source is exactly 0 - far
out-of-range, infinite and NaN flow included - whatever the source's border pixels hold (infinity and NaN included); an out-of-range
tap contributes 0, as in F.grid_sample.  The displacement embedding of a NaN flow is NaN, in that pixel only.

Measured on MI355X, worst over the cases of each kind: |fp32 CPU evaluation - truth| of the reference / |kernel - truth| [worst
|out - truth| / bound, 1 being the limit].  fp16 and bf16 results carry their own rounding (the r-term), which is why they come
close to 1: the kernels round once, and a half spacing is what one rounding costs.
    warp, packet kernel           fp32 4.43e-06 / 4.43e-06 [0.25]   fp16 5.77e-06 / 9.74e-04 [0.97]   bf16 5.75e-06 / 7.81e-03 [0.99]
    warp, one thread per pixel                                      fp16 4.35e-06 / 9.76e-04 [0.97]   bf16 4.34e-06 / 7.79e-03 [0.99]
    warp, element-wise            fp32 3.57e-06 / 3.57e-06 [0.25]   fp16 4.93e-06 / 9.76e-04 [0.97]   bf16 4.88e-06 / 7.80e-03 [0.99]
    disp_emb                      fp32 6.67e-06 / 6.67e-06 [0.25]   fp16 6.67e-06 / 1.55e-02 [0.98]   bf16 6.67e-06 / 2.43e-01 [0.99]
    refiner_assemble, warp                                          fp16 9.68e-06 / 1.10e-03 [0.97]   bf16 9.70e-06 / 1.08e-02 [0.99]
    refiner_assemble, embedding                                     fp16 6.67e-06 / 2.57e-02 [0.98]   bf16 6.67e-06 / 2.44e-01 [0.99]
    interp (and the pair form)    fp32 2.27e-06 / 2.27e-06 [0.27]
    flow_update                   flow 6.01e-08 / 5.96e-08 [0.25]   certainty 2.38e-07 / 2.38e-07 [0.25]
    refiner_head (activation fp32 / fp16 / bf16; flow, certainty, delta are fp32)
        flow       7.38e-08 / 5.95e-08 [0.25]   7.28e-08 / 6.12e-08 [0.25]   1.05e-07 / 6.41e-08 [0.26]
        certainty  2.42e-06 / 3.86e-07 [0.25]   3.22e-06 / 4.98e-07 [0.20]   2.78e-06 / 4.16e-07 [0.24]
        delta      3.34e-06 / 4.18e-07 [0.14]   3.22e-06 / 4.98e-07 [0.14]   4.66e-06 / 4.16e-07 [0.24]
    second pass of the grid-stride loops
        warp packet fp16 4.21e-06 / 1.83e-03 [0.98]   per pixel fp16 4.71e-06 / 1.88e-03 [0.98]   element-wise fp32 3.69e-06 / 3.69e-06 [0.25]
        disp_emb fp16 1.54e-06 / 7.11e-03 [1.00]      interp 8.53e-05 / 8.53e-05 [0.25]           flow_update 6.33e-08 / 5.96e-08 [0.24]
        refiner_head fp16, 2 097 153 pixels at C = 8: delta 9.38e-07 / 9.19e-07 [0.25]; 131 073 pixels at C = 512: 4.19e-06 / 5.13e-07 [0.03]
The packet and per-pixel kernels and both refiner_assemble kernels load every tap from a clamped address; they used to mask an
out-of-range tap through its weight alone, 0 * src[clamped pixel], which is NaN where that border pixel is inf or NaN.  They now also
keep only the sign bits of such a tap (sampling.hip tap_mask), which is what the non-finite-source assertions here pin.
"""
import functools
import math

import pytest
import torch

from tests import helpers as H
from tests import sampling_ref as S
from tests.golden import recipes as R
from tests.test_refiner_assemble import LEVELS

gpu = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GUARD = 256                                  # elements in front of and behind every output (a multiple of 8: 16-byte alignment stays)
SENTINEL = -7.25
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, F16, BF16]
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16"}
B, HS, WS, HG, WG = 4, 11, 13, 19, 26        # source 4 x C x 11 x 13, grid 19 x 26: the sizes differ on both axes
SHIFTS = (0, 1, B // 2)
GAIN = 1.875                                 # 40 / 32 * 1.5, exact in fp32


def _ops():
    from roma_amd import ops
    return ops


def flow_for(b=B, h=HG, w=WG, hs=HS, ws=WS):
    return S.planted_flow(f"sk.flow.{h}x{w}", b, h, w, hs, ws)


@functools.lru_cache(maxsize=None)
def source(C, dtype, b=B, hs=HS, ws=WS):
    """The source as the kernel sees it: rounded to its storage type.  Shared: read-only."""
    return H.T(R.normal(f"sk.src.{C}", (b, C, hs, ws))).to(dtype)


@functools.lru_cache(maxsize=None)
def emb_weights(E):
    return H.T(R.normal(f"sk.emb.w.{E}", (E, 2))), H.T(R.normal(f"sk.emb.b.{E}", (E,)))


def nonfinite_ring(src):
    """The source with its border ring set to +inf, -inf and NaN in turn."""
    s = src.clone()
    vals = torch.tensor([math.inf, -math.inf, math.nan]).to(src.dtype)
    _, _, hs, ws = s.shape
    ring = torch.zeros((hs, ws), dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    idx = ring.nonzero()
    for i, (y, x) in enumerate(idx.tolist()):
        s[:, :, y, x] = vals[i % 3]
    return s


def report(what, ref_err, got_err, worst):
    print(f"{what}: reference fp32 error {ref_err:.2e}, kernel error {got_err:.2e} ({worst:.2f} of the bound)")


# ---- buffers with a sentinel everywhere the kernel must not write ------------------------------------------------------------------
class Store:
    """A (b, C, h, w) view for the kernels, over fresh device storage filled with the sentinel: planar, or channels [off, off + C) of
    channels-last pixels of `pitch` channels; GUARD elements in front and behind."""

    def __init__(self, b, C, h, w, dtype, layout, pitch=None, off=0):
        self.C, self.off, self.nhwc = C, off, layout == "nhwc"
        shape = (b, h, w, pitch or C) if self.nhwc else (b, C, h, w)
        self.n = math.prod(shape)
        self.flat = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.body = self.flat[GUARD:GUARD + self.n].view(shape)
        self.view = self.body[..., off:off + C].permute(0, 3, 1, 2) if self.nhwc else self.body

    def fill(self, t):
        self.view.copy_(t.to(DEV))
        return self

    def reset(self):
        self.flat.fill_(SENTINEL)

    def assert_rest_untouched(self):
        assert bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[GUARD + self.n:] == SENTINEL).all()), "guard band written"
        if self.nhwc:
            keep = torch.ones(self.body.shape[-1], dtype=torch.bool, device=DEV)
            keep[self.off:self.off + self.C] = False
            assert bool((self.body[..., keep] == SENTINEL).all()), "channels outside the destination slice written"


def dense(C):
    return ("nhwc", C, 0)


PLANAR = ("planar", None, 0)


def _warp_cases():
    cases = []
    for dt, C in ((F16, 8), (F16, 64), (BF16, 8), (BF16, 64), (F32, 4), (F32, 12)):                 # the packet kernel
        e = 4 if dt == F32 else 8
        cases += [(f"packet-dense-{NAME[dt]}-C{C}", dt, C, dense(C), dense(C)),
                  (f"packet-srcslice-{NAME[dt]}-C{C}", dt, C, ("nhwc", C + 2 * e, e), dense(C)),
                  (f"packet-dstslice-{NAME[dt]}-C{C}", dt, C, dense(C), ("nhwc", C + 3 * e, 2 * e))]
    for dt in (F16, BF16):                                                                         # one thread per pixel: one / two packets
        for C, sp, dp, off in ((1, 8, 8, 2), (1, 8, 8, 3), (3, 8, 8, 4), (3, 8, 8, 5), (9, 16, 24, 9), (9, 16, 24, 10), (12, 16, 32, 14),
                               (12, 16, 32, 15), (16, 16, 40, 17), (16, 16, 40, 18)):
            cases.append((f"pixel-{NAME[dt]}-C{C}-off{off}", dt, C, ("nhwc", sp, 0), ("nhwc", dp, off)))
    for dt in DTYPES:                                                                              # element-wise
        cases += [(f"element-planar-planar-{NAME[dt]}", dt, 5, PLANAR, PLANAR),
                  (f"element-planar-nhwc-{NAME[dt]}", dt, 5, PLANAR, ("nhwc", 8, 1)),
                  (f"element-nhwc-planar-{NAME[dt]}", dt, 5, ("nhwc", 8, 2), PLANAR),
                  (f"element-dense-C9-{NAME[dt]}", dt, 9, dense(9), dense(9))]
    for dt in (F16, BF16):
        cases += [(f"element-C20-{NAME[dt]}", dt, 20, ("nhwc", 24, 0), dense(20)),
                  (f"element-unaligned-src-C8-{NAME[dt]}", dt, 8, ("nhwc", 16, 4), dense(8))]
    return cases


WARP_CASES = _warp_cases()


def expected_kernel(dt, C, src, dst):
    """The line of roma_warp_bilinear's dispatch a case takes (the Store's base is 16-byte aligned)."""
    e = 4 if dt == F32 else 8
    nhwc = src[0] == "nhwc" and dst[0] == "nhwc"
    al = lambda s: (s[2] * (4 if dt == F32 else 2)) % 16 == 0
    if nhwc and C % e == 0 and src[1] % e == 0 and dst[1] % e == 0 and al(src) and al(dst):
        return "packet"
    if nhwc and dt != F32 and C <= 16 and src[1] % 8 == 0 and src[1] >= 8 * ((C + 7) // 8) and dst[1] % 2 == 0 and al(src):
        return "pixel"
    return "element"


def test_every_warp_case_takes_the_dispatch_line_it_is_named_for():
    for name, dt, C, src, dst in WARP_CASES:
        assert expected_kernel(dt, C, src, dst) == name.split("-")[0], name


# ---- CPU: the references themselves --------------------------------------------------------------------------------------------------
def test_flow_has_the_planted_edges_and_the_excluded_share_is_within_its_cap():
    flow = flow_for()
    nf = S.nonfinite_pixels(flow)
    per_map = nf.flatten(1).sum(1)
    assert int(per_map.max()) <= S.MAX_EXCLUDED and int(per_map.min()) >= 4
    for v in (-1.0, 1.0, -7.0, 1e30, math.inf, -math.inf):
        assert bool((flow == v).any()), v
    assert bool(flow.isnan().any())
    outside, ring, inner = S.tap_classes(flow, HS, WS)
    assert int(outside.sum()) >= 10 * B and int(inner.sum()) > 100 and int(ring.sum()) > 100
    # outside the excluded pixels the reference is finite everywhere, and exactly 0 where every tap is outside
    src = source(8, F16)
    for shift in SHIFTS:
        t = S.warp_truth(src, flow, shift)
        assert bool(t.isfinite()[~nf.expand_as(t)].all())
        assert bool((t[(outside & ~nf).expand_as(t)] == 0).all())
    w, b = emb_weights(6)
    e = S.emb_truth(flow, w, b, GAIN)
    assert bool(e.isfinite()[~nf.expand_as(e)].all())


def test_truths_equal_the_oracle_and_torch():
    from oracle import roma_oracle as O
    flow = flow_for()
    ok = ~S.nonfinite_pixels(flow) & ~S.huge_pixels(flow)
    src = source(12, F32)
    t = S.warp_truth(src, flow, 0)
    # the oracle's ConvRefiner.forward line (matcher.py:109), in fp32
    o = torch.nn.functional.grid_sample(src, flow.permute(0, 2, 3, 1), align_corners=False, mode="bilinear")
    # fp32 places the sample within 3 roundings of a position <= 13, ~2.4e-6 pixel, and neighbouring source values differ by up to ~8
    assert float((o.double() - t)[ok.expand_as(t)].abs().max()) < 2e-5
    for shift in SHIFTS:                                         # the tap-by-tap form the mutants are made from
        d = (S.warp_manual(src, flow, shift) - S.warp_truth(src, flow, shift))[ok.expand_as(t)].abs().max()
        assert float(d) < 1e-13
    w, b = emb_weights(16)
    e = S.emb_truth(flow, w, b, GAIN)
    o = torch.nn.functional.conv2d(GAIN * (flow.double() - O.pixel_grid(B, HG, WG).double()), w.double().view(16, 2, 1, 1), b.double())
    assert float((o - e)[ok.expand_as(e)].abs().max()) < 2e-6      # pixel_grid is an fp32 linspace: 1.2e-7 * gain * |w|


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_every_mutant_is_ten_bounds_away(dtype):
    flow = flow_for()
    ok = ~S.nonfinite_pixels(flow)
    src = source(8, dtype)
    for shift in SHIFTS:
        t = S.warp_truth(src, flow, shift)
        slop = S.slop_of(S.warp_truth(src, flow, shift, F32), t, ok)
        for name, f in S.warp_mutants(dtype).items():
            x = S.excess(f(src, flow, shift), t, dtype, slop, ok)
            print(f"warp {NAME[dtype]} shift {shift} {name}: {x:.3g} x the bound")
            assert x >= 10, name
    ordinary = ok & ~S.huge_pixels(flow)
    w, b = emb_weights(16)
    t = S.emb_truth(flow, w, b, GAIN)
    slop = S.slop_of(S.emb_eval32(flow, w, b, GAIN), t, ordinary)
    for name, f in S.emb_mutants().items():
        x = S.excess(f(flow, w, b, GAIN), t, dtype, slop, ordinary)
        print(f"disp_emb {NAME[dtype]} {name}: {x:.3g} x the bound")
        assert x >= 10, name
    x, wo, bo, fl, cert = head_inputs(dtype, 128, 136, 2, 5, 7)
    truth = S.head_truth(x, wo, bo, fl, cert, SX, SY)
    ev = S.head_truth(x, wo, bo, fl, cert, SX, SY, F32)
    for name, kw in (("head weights shifted by one row", dict(row_shift=1)), ("sx / sy swapped", dict(swap_s=True))):
        m = S.head_truth(x, wo, bo, fl, cert, SX, SY, **kw)
        xs = [S.excess(mi, ti, F32, S.slop_of(ei, ti)) for mi, ti, ei in zip(m, truth, ev)]
        print(f"refiner_head {NAME[dtype]} {name}: {max(xs):.3g} x the bound")
        assert max(xs) >= 10, name
    delta = H.T(R.normal("sk.fu.delta", (2, 3, 5, 7)))
    tf, _ = S.update_truth(fl, cert, delta, SX, SY)
    ef, _ = S.update_truth(fl, cert, delta, SX, SY, F32)
    mf, _ = S.update_truth(fl, cert, delta, SX, SY, swap_s=True)
    assert S.excess(mf, tf, F32, S.slop_of(ef, tf)) >= 10


# ---- 1, 2: warp_bilinear -------------------------------------------------------------------------------------------------------------
def run_warp(dt, C, src_spec, dst_spec, flow, src, shifts, what):
    """Every shift: the call against the truth; exact zeros where every tap is outside; nothing else written.  Then the same call on the
    source with a non-finite border ring: zeros again where every tap is outside, the finite run's bits wherever no tap that can carry
    weight is on the ring."""
    ops = _ops()
    b, _, hs, ws = src.shape
    h, w = flow.shape[2:]
    fl = flow.to(DEV)
    nf = S.nonfinite_pixels(flow)
    outside, ring, inner = S.tap_classes(flow, hs, ws)
    assert int(nf.flatten(1).sum(1).max()) <= S.MAX_EXCLUDED
    s_fin = Store(b, C, hs, ws, dt, *src_spec).fill(src)
    s_nan = Store(b, C, hs, ws, dt, *src_spec).fill(nonfinite_ring(src))
    dst = Store(b, C, h, w, dt, *dst_spec)
    for shift in shifts:
        truth = S.warp_truth(src, flow, shift)
        ref_err = S.slop_of(S.warp_truth(src, flow, shift, F32), truth, ~nf) / S.SLACK
        dst.reset()
        out = ops.warp_bilinear(s_fin.view, fl, out=dst.view, batch_shift=shift)
        assert out.data_ptr() == dst.view.data_ptr()
        got = dst.view.cpu()
        dst.assert_rest_untouched()
        worst = S.excess(got, truth, dt, S.SLACK * ref_err, ~nf)
        report(f"warp {what} shift {shift}", ref_err, float((got.double() - truth)[(~nf).expand_as(truth)].abs().max()), worst)
        assert worst <= 1.0
        assert bool((got[outside.expand_as(got)] == 0).all()), "a sample with every tap outside (or a non-finite flow) is not exactly 0"
        dst.reset()
        ops.warp_bilinear(s_nan.view, fl, out=dst.view, batch_shift=shift)
        bad = dst.view.cpu()
        dst.assert_rest_untouched()
        assert bool((bad[outside.expand_as(bad)] == 0).all()), "non-finite border pixels leak into samples with every tap outside"
        m = inner.expand_as(bad)
        assert torch.equal(bad[m].view(torch.int16 if dt != F32 else torch.int32), got[m].view(torch.int16 if dt != F32 else torch.int32)), \
            "samples off the border ring changed with the ring's values"


@gpu
@pytest.mark.parametrize("name,dt,C,src_spec,dst_spec", WARP_CASES, ids=[c[0] for c in WARP_CASES])
def test_warp_bilinear_every_dispatch_line_and_nonfinite_source(name, dt, C, src_spec, dst_spec):
    run_warp(dt, C, src_spec, dst_spec, flow_for(), source(C, dt), SHIFTS, name)


# ---- 3: disp_emb ---------------------------------------------------------------------------------------------------------------------
def _emb_cases():
    cases = []
    for E in (6, 16, 32, 64, 128):
        cases += [(f"E{E}-planar", E, PLANAR), (f"E{E}-dense", E, dense(E))]
    for C, E, D, Dp in LEVELS:
        cases.append((f"E{E}-slice-of-{Dp}", E, ("nhwc", Dp, 2 * C)))
    return cases


EMB_CASES = _emb_cases()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("name,E,dst_spec", EMB_CASES, ids=[c[0] for c in EMB_CASES])
def test_disp_emb(name, E, dst_spec, dtype):
    flow = flow_for()
    w, b = emb_weights(E)
    truth = S.emb_truth(flow, w, b, GAIN)
    ordinary = ~S.nonfinite_pixels(flow) & ~S.huge_pixels(flow)
    ref_err = S.slop_of(S.emb_eval32(flow, w, b, GAIN), truth, ordinary) / S.SLACK
    dst = Store(B, E, HG, WG, dtype, *dst_spec)
    out = _ops().disp_emb(flow.to(DEV), w.to(DEV), b.to(DEV), GAIN, out=dst.view)
    assert out.data_ptr() == dst.view.data_ptr()
    got = dst.view.cpu()
    dst.assert_rest_untouched()
    worst = S.emb_check(got, truth, flow, dtype, S.SLACK * ref_err)
    report(f"disp_emb {name} {NAME[dtype]}", ref_err, float((got.double() - truth)[ordinary.expand_as(truth)].abs().max()), worst)


# ---- 4: refiner_assemble against the truths ------------------------------------------------------------------------------------------
def run_assemble(level, dtype, separate, b, flow, hs, ws, what, nonfinite=False):
    ops = _ops()
    C, E, D, Dp = level
    h, w = flow.shape[2:]
    shift = b // 2
    we, be = emb_weights(E)
    buf = Store(b, Dp, h, w, dtype, "nhwc", Dp, 0)                # the whole pixel is the view: nothing of it is exempt here
    x = H.T(R.normal(f"sk.asm.x.{C}", (b, C, h, w))).to(dtype)
    if separate:
        src = H.T(R.normal(f"sk.asm.y.{C}", (b, C, hs, ws))).to(dtype)
        if nonfinite:
            src = nonfinite_ring(src)
        y = Store(b, C, hs, ws, dtype, "nhwc", 16 if C == 9 else C + 8, 0).fill(src)
        src_view, y_before = y.view, y.flat.clone()
    else:
        src = nonfinite_ring(x) if nonfinite else x
        hs, ws = h, w
    d = buf.body.permute(0, 3, 1, 2)
    d[:, :C] = src.to(DEV) if not separate else x.to(DEV)
    if not separate:
        src_view = d[:, :C]
    before = buf.body.clone()
    ops.refiner_assemble(buf.body, src_view, flow.to(DEV), we.to(DEV), be.to(DEV), GAIN, C, D, batch_shift=shift)
    torch.cuda.synchronize()
    got = buf.body.cpu().permute(0, 3, 1, 2)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(buf.body[..., :C]), bits(before[..., :C])), "x channels were written"
    keep = D // 8 * 8 if Dp > D else D
    assert torch.equal(bits(buf.body[..., 2 * C + E:keep]), bits(before[..., 2 * C + E:keep])), "correlation slice written outside the last packet"
    assert bool((buf.flat[:GUARD] == SENTINEL).all()) and bool((buf.flat[GUARD + buf.n:] == SENTINEL).all()), "guard band written"
    if Dp > D:
        assert bool((bits(buf.body[..., D:]) == 0).all()), "padding is not zero"
    if separate:
        assert torch.equal(bits(y.flat), bits(y_before)), "source written"
    outside, ring, inner = S.tap_classes(flow, hs, ws)
    warp = got[:, C:2 * C]
    assert bool((warp[outside.expand_as(warp)] == 0).all()), "a sample with every tap outside is not exactly 0"
    if nonfinite:
        return warp, inner
    nf = S.nonfinite_pixels(flow)
    truth = S.warp_truth(src, flow, shift)
    ref_err = S.slop_of(S.warp_truth(src, flow, shift, F32), truth, ~nf) / S.SLACK
    worst = S.excess(warp, truth, dtype, S.SLACK * ref_err, ~nf)
    report(f"assemble warp {what}", ref_err, float((warp.double() - truth)[(~nf).expand_as(truth)].abs().max()), worst)
    assert worst <= 1.0
    et = S.emb_truth(flow, we, be, GAIN)
    ordinary = ~nf & ~S.huge_pixels(flow)
    eref = S.slop_of(S.emb_eval32(flow, we, be, GAIN), et, ordinary) / S.SLACK
    emb = got[:, 2 * C:2 * C + E]
    worst = S.emb_check(emb, et, flow, dtype, S.SLACK * eref)
    report(f"assemble embedding {what}", eref, float((emb.double() - et)[ordinary.expand_as(et)].abs().max()), worst)
    return warp, inner


@gpu
@pytest.mark.parametrize("separate", [False, True], ids=["in_buffer", "separate"])
@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=NAME.get)
@pytest.mark.parametrize("level", LEVELS, ids=[f"C{lv[0]}-E{lv[1]}" for lv in LEVELS])
def test_refiner_assemble_against_the_truths(level, dtype, b, separate):
    flow = flow_for(b, HG, WG, HS, WS) if separate else S.planted_flow(f"sk.flow.self.{b}", b, HG, WG, HG, WG)
    run_assemble(level, dtype, separate, b, flow, HS, WS, f"C{level[0]} {NAME[dtype]} B{b} {'separate' if separate else 'in buffer'}")


@gpu
@pytest.mark.parametrize("separate", [False, True], ids=["in_buffer", "separate"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=NAME.get)
@pytest.mark.parametrize("level", LEVELS[:3], ids=[f"C{lv[0]}-E{lv[1]}" for lv in LEVELS[:3]])
def test_refiner_assemble_nonfinite_source(level, dtype, separate):
    flow = flow_for() if separate else S.planted_flow(f"sk.flow.self.{B}", B, HG, WG, HG, WG)
    fin, inner = run_assemble(level, dtype, separate, B, flow, HS, WS, "finite")
    bad, _ = run_assemble(level, dtype, separate, B, flow, HS, WS, "ring", nonfinite=True)
    m = inner.expand_as(fin)
    assert int(inner.sum()) > 100
    assert torch.equal(bad[m].view(torch.int16), fin[m].view(torch.int16)), "samples off the border ring changed with the ring's values"


# ---- 5: interp -----------------------------------------------------------------------------------------------------------------------
INTERP = [((1, 7), (5, 9)), ((7, 1), (9, 4)), ((1, 1), (3, 4)), ((5, 6), (13, 17)), ((23, 19), (7, 5)), ((9, 14), (20, 6)), ((7, 9), (7, 9))]


def check_interp(got, x, size, what):
    truth = S.interp_truth(x, size)
    ref_err = S.slop_of(S.interp_truth(x, size, F32), truth) / S.SLACK
    got = got.cpu()
    err = float((got.double() - truth).abs().max())
    report(f"interp {what}", ref_err, err, S.excess(got, truth, F32, S.SLACK * ref_err) if ref_err > 0 else 0.0)
    assert bool(((got.double() - truth).abs() <= S.bound(truth, F32, S.SLACK * ref_err)).all())


@gpu
@pytest.mark.parametrize("sizes", INTERP, ids=[f"{a[0]}x{a[1]}-{b_[0]}x{b_[1]}" for a, b_ in INTERP])
def test_interp_bilinear_and_pair(sizes):
    ops = _ops()
    (hi, wi), size = sizes
    x = H.T(R.normal(f"sk.interp.{sizes}", (2, 2, hi, wi)))
    c = H.T(R.normal(f"sk.interp.c.{sizes}", (2, 1, hi, wi)))
    gx, gc = ops.interp_bilinear(x.to(DEV), size), ops.interp_bilinear(c.to(DEV), size)
    check_interp(gx, x, size, f"{sizes} 2 channels")
    check_interp(gc, c, size, f"{sizes} 1 channel")
    if (hi, wi) == tuple(size):
        assert torch.equal(gx.cpu(), x) and torch.equal(gc.cpu(), c), "equal sizes must copy"
    px, pc = ops.interp_bilinear_pair(x.to(DEV), c.to(DEV), size)
    assert torch.equal(px, gx) and torch.equal(pc, gc), "the pair form differs from two single calls"
    pc2, px2 = ops.interp_bilinear_pair(c.to(DEV), x.to(DEV), size)  # 1 + 2 channels
    assert torch.equal(px2, gx) and torch.equal(pc2, gc)


# ---- 6: flow_update and refiner_head --------------------------------------------------------------------------------------------------
SX, SY = 3 / 128, 5 / 256                    # exact in fp32, and different


@functools.lru_cache(maxsize=None)
def head_inputs(dtype, C, pitch, b, h, w):
    x = H.T(R.normal(f"sk.head.x.{C}.{h}x{w}", (b, h, w, pitch))).to(dtype)
    wo = H.T(R.normal(f"sk.head.wo.{C}", (C, 3), scale=C ** -0.5))
    bo = H.T(R.normal(f"sk.head.bo.{C}", (3,)))
    flow = H.T(R.coherent_flow(f"sk.head.flow.{h}x{w}", b, h, w))
    cert = H.T(R.normal(f"sk.head.cert.{h}x{w}", (b, 1, h, w)))
    return x, wo, bo, flow, cert


def flow_store(flow):
    b, _, h, w = flow.shape
    return Store(b, 2, h, w, F32, "planar").fill(flow)


def check_three(got, truth, ev, what):
    for name, g, t, e in zip(("flow", "certainty", "delta"), got, truth, ev):
        ref_err = S.slop_of(e, t) / S.SLACK
        g = g.cpu()
        worst = S.excess(g, t, F32, S.SLACK * ref_err)
        report(f"{what} {name}", ref_err, float((g.double() - t).abs().max()), worst)
        assert worst <= 1.0, f"{what} {name}"


def run_head(dtype, C, pitch, b, h, w, what, variants=((True, True), (True, False), (False, True), (False, False))):
    ops = _ops()
    x, wo, bo, flow, cert = head_inputs(dtype, C, pitch, b, h, w)
    xd, wd, bd = x.to(DEV), wo.to(DEV), bo.to(DEV)
    for with_cert, want_delta in variants:
        c = cert if with_cert else None
        truth = S.head_truth(x, wo, bo, flow, c, SX, SY)
        ev = S.head_truth(x, wo, bo, flow, c, SX, SY, F32)
        fs = flow_store(flow)
        res = ops.refiner_head(xd, wd, bd, fs.view, None if c is None else c.to(DEV), SX, SY, want_delta=want_delta)
        assert len(res) == (3 if want_delta else 2) and res[0].data_ptr() == fs.view.data_ptr(), "flow is updated in place"
        fs.assert_rest_untouched()                               # flow has channels 0 and 1 and nothing is written beside them
        assert res[1].shape == (b, 1, h, w)
        check_three((fs.view,) + tuple(res[1:]), truth, ev, f"refiner_head {what} cert={with_cert}")
    assert torch.equal(xd.cpu().view(-1).view(torch.int16 if dtype != F32 else torch.int32),
                       x.view(-1).view(torch.int16 if dtype != F32 else torch.int32)), "activation written"


def _head_cases():
    cases = [(dt, D, D) for dt in DTYPES for D in (24, 144, 576, 1152, 1408)]                       # the shipped (D, pitch)
    cases += [(dt, C, C + 8) for dt in (F16, BF16) for C in (120, 128, 504, 512)]                  # packets per pixel 15 / 16, 63 / 64
    cases += [(F32, C, C + 8) for C in (60, 64, 252, 256)]
    return cases


@gpu
@pytest.mark.parametrize("dtype,C,pitch", _head_cases(), ids=lambda v: NAME.get(v, str(v)))
def test_refiner_head(dtype, C, pitch):
    run_head(dtype, C, pitch, 2, 5, 7, f"{NAME[dtype]} C{C}")


@gpu
@pytest.mark.parametrize("with_cert", [True, False])
def test_flow_update(with_cert):
    b, h, w = 2, 5, 7
    _, _, _, flow, cert = head_inputs(F32, 24, 24, b, h, w)
    delta = H.T(R.normal("sk.fu.delta", (b, 3, h, w)))
    c = cert if with_cert else None
    fs = flow_store(flow)
    f, cn = _ops().flow_update(fs.view, None if c is None else c.to(DEV), delta.to(DEV), SX, SY)
    assert f.data_ptr() == fs.view.data_ptr()
    fs.assert_rest_untouched()
    check_three((fs.view, cn), S.update_truth(flow, c, delta, SX, SY), S.update_truth(flow, c, delta, SX, SY, F32), f"flow_update cert={with_cert}")


# ---- 7: the second pass of every grid-stride loop (launches are capped at 8192 x 256 threads; refiner_head at 32768 blocks) ----------
CAP = 8192 * 256


BIG_WARPS = [("packet-fp16-C64", F16, 64, dense(64), dense(64), 2, 363, 363),
             ("pixel-fp16-C9", F16, 9, ("nhwc", 16, 0), ("nhwc", 24, 9), 2, 1024, 1025),
             ("element-fp32-C3", F32, 3, PLANAR, PLANAR, 2, 600, 600)]


@gpu
@pytest.mark.parametrize("name,dt,C,src_spec,dst_spec,b,h,w", BIG_WARPS, ids=[c[0] for c in BIG_WARPS])
def test_warp_second_pass_of_the_grid_stride_loop(name, dt, C, src_spec, dst_spec, b, h, w):
    kind = expected_kernel(dt, C, src_spec, dst_spec)
    assert kind == name.split("-")[0]
    items = b * h * w * {"packet": C // 8, "pixel": 1, "element": C}[kind]
    assert CAP < items < CAP * 1.04
    run_warp(dt, C, src_spec, dst_spec, S.planted_flow(f"sk.big.{h}", b, h, w, 16, 16), source(C, dt, b, 16, 16), (1,), name)


@gpu
def test_disp_emb_second_pass_of_the_grid_stride_loop():
    E, b, h, w = 6, 2, 420, 420
    assert CAP < b * E * h * w < CAP * 1.04
    flow = S.planted_flow("sk.big.emb", b, h, w, h, w)
    wgt, bias = emb_weights(E)
    truth = S.emb_truth(flow, wgt, bias, GAIN)
    ordinary = ~S.nonfinite_pixels(flow) & ~S.huge_pixels(flow)
    ref_err = S.slop_of(S.emb_eval32(flow, wgt, bias, GAIN), truth, ordinary) / S.SLACK
    dst = Store(b, E, h, w, F16, "nhwc", 24, 18)
    _ops().disp_emb(flow.to(DEV), wgt.to(DEV), bias.to(DEV), GAIN, out=dst.view)
    got = dst.view.cpu()
    dst.assert_rest_untouched()
    worst = S.emb_check(got, truth, flow, F16, S.SLACK * ref_err)
    report("disp_emb 2 x 6 x 420 x 420 fp16", ref_err, float((got.double() - truth)[ordinary.expand_as(truth)].abs().max()), worst)


@gpu
def test_interp_second_pass_of_the_grid_stride_loop():
    ops = _ops()
    size = (600, 600)
    x = H.T(R.normal("sk.big.interp", (1, 6, 211, 197)))
    assert CAP < 6 * 600 * 600 < CAP * 1.04
    g = ops.interp_bilinear(x.to(DEV), size)
    check_interp(g, x, size, "6 planes to 600 x 600")
    pa, pb = ops.interp_bilinear_pair(x[:, :4].to(DEV), x[:, 4:].to(DEV), size)
    assert torch.equal(pa, g[:, :4]) and torch.equal(pb, g[:, 4:]), "the pair form differs from the single call"


@gpu
def test_flow_update_second_pass_of_the_grid_stride_loop():
    b, h, w = 2, 1024, 1025
    assert CAP < b * h * w < CAP * 1.04
    flow = H.T(R.coherent_flow("sk.big.fu", b, h, w))
    cert = H.T(R.normal("sk.big.fu.cert", (b, 1, h, w)))
    delta = H.T(R.normal("sk.big.fu.delta", (b, 3, h, w)))
    fs = flow_store(flow)
    f, cn = _ops().flow_update(fs.view, cert.to(DEV), delta.to(DEV), SX, SY)
    fs.assert_rest_untouched()
    check_three((fs.view, cn), S.update_truth(flow, cert, delta, SX, SY), S.update_truth(flow, cert, delta, SX, SY, F32), "flow_update 2 x 1024 x 1025")


@gpu
@pytest.mark.parametrize("C,h,w,lanes", [(8, 3, 699051, 4), (512, 3, 43691, 64)])
def test_refiner_head_past_its_block_cap(C, h, w, lanes):
    assert h * w * lanes > 32768 * 256 and h * w * lanes - 32768 * 256 <= lanes       # one pixel past the cap
    run_head(F16, C, C, 1, h, w, f"fp16 C{C} {h * w} pixels", variants=((True, True),))
