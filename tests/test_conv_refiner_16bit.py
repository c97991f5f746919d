"""The 16-bit ConvRefiner MODULE (roma_amd.matcher.ConvRefiner: assembly, every block path, the ping-pong buffers, out_conv /
refiner_head) at the five shipped widths of model_zoo.REFINER_SPEC, D = 1377, 1137, 569, 144 and 24, against two references written in
plain torch ops:

    truth      everything in fp64 from the dtype-rounded x, y and block weights (disp_emb and out_conv weights keep their fp32 values, as
               in the product): F.grid_sample, local_correlation restated in its arguments' dtype (the oracle's computes in fp32
               whatever it is given; `local_corr_ref` is pinned to it and to the reference's literal grid_sample form below), the
               oracle module's blocks in .double(), no rounding in between.
    yardstick  what the reference computes under autocast: fp32 positions, grid_sample / local_correlation / embedding in fp32 on the
               rounded features and rounded to the dtype once, the oracle module's blocks .to(dtype) through the library, out_conv in
               fp32.

For every compared tensor e_lib = max |yardstick - truth| and e_hip = max |product - truth| on the same inputs, and the test asserts
e_hip <= 2 e_lib (the rule of test_vgg_conv_fused.py: both sum in fp32, the product rounds in fewer places because BatchNorm is folded
in fp32, so the factor 2 is room for the order of summation).  Weights are variance-preserving (`make_state`), because after nine
blocks of PyTorch's default initialisation only the biases are left and no mistake in the assembly can be seen.

The CPU test shows that the bound can fail: six mutants of truth (embedding slice rolled by a channel, warp without the batch shift,
correlation slice rolled by a channel, a block skipped, block 1's weights used for block 0 too, one depthwise tap zeroed) are each at
least 4 x (2 e_lib) away from truth.

Measured on the CPU (test_mutants_of_truth_are_far_outside_the_bound; the smallest mutant / (2 e_lib) over D = 24, 144, 569 and 0, 2, 8
hidden blocks, fp16 / bf16; 4 is asserted):
    embedding rolled 37.8 / 4.8    warp without batch shift 123.9 / 12.3    correlation rolled 65.4 / 8.3    block skipped 352 / 34.8
    block weights reused 192 / 19.1    tap zeroed (no hidden block) 86.6 / 9.5
    e_lib there: fp16 1.8e-3 to 7.7e-3, bf16 1.6e-2 to 7.8e-2; max |activation| 3.7 to 6.7.

Measured on MI355X (worst e_lib / e_hip over both maps, the depths 0, 2, 8, every implementation and entry; "act" the last block's
activation, "out" the worst of out_conv's outputs, the updated flow in out_conv's units and the certainty):
    D       fp16 act             fp16 out             bf16 act             bf16 out
    24      1.72e-2 / 4.58e-3    1.44e-2 / 5.41e-3    1.86e-1 / 3.65e-2    1.58e-1 / 4.22e-2
    144     1.82e-2 / 5.01e-3    1.04e-2 / 3.85e-3    1.23e-1 / 4.33e-2    6.68e-2 / 3.06e-2
    569     2.08e-2 / 5.63e-3    1.59e-2 / 4.35e-3    1.58e-1 / 4.96e-2    1.16e-1 / 3.54e-2
    1137    2.45e-2 / 5.90e-3    1.13e-2 / 4.18e-3    1.72e-1 / 5.20e-2    8.95e-2 / 4.00e-2
    1377    2.07e-2 / 6.46e-3    1.15e-2 / 4.26e-3    1.45e-1 / 4.06e-2    8.86e-2 / 2.79e-2
The largest e_hip / e_lib of any single compared tensor is 0.75 (2 is asserted); the two D = 144 paths and the two fp16 D = 569 paths
give the same figures.  fp32 control: at most 8.0e-6 against bounds of 6.8e-5 to 2.7e-4.
The poisoned runs also show that the module's result does not depend on what the padding channels [D, Dp) of a fresh buffer hold: the
depthwise kernels' ReLU is a max that drops a NaN, and the padded taps, scale and shift are zero.
"""
import contextlib
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import roma_oracle as oracle
from roma_amd import matcher
from roma_amd.model_zoo import REFINER_SPEC

torch.set_grad_enabled(False)
DEV = "cuda"
HALF = [torch.float16, torch.bfloat16]
SF2 = 864 / 560                                  # the upsample pass's scale_factor (sqrt of the area ratio)
MAPS = [(2, 19, 23), (4, 9, 40)]                 # partial 8 x 16, 16 x 16 and 8-pixel-strip tiles; r = 7 reaches past every border
MAP_SF = {MAPS[0]: 1.0, MAPS[1]: SF2}
MUTANT_FACTOR = 4


def width(level):
    feat, emb, r = REFINER_SPEC[level]
    return 2 * feat + emb + ((2 * r + 1) ** 2 if r else 0)


BY_WIDTH = {width(s): s for s in REFINER_SPEC}
assert sorted(BY_WIDTH) == [24, 144, 569, 1137, 1377]
# (level, dtype, block implementation, mid implementation): everything prepare() builds for the level and dtype
IMPLS = []
for _D, _impls in ((24, ["fused"]), (144, ["split_mfma/one", "split_mfma/two"]), (569, ["split_gemm", "wide"]), (1137, ["split_gemm"]),
                   (1377, ["split_gemm"])):
    for _dt in HALF:
        for _i in _impls:
            if _i != "wide" or _dt == torch.float16:
                IMPLS.append((BY_WIDTH[_D], _dt, _i))


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return str(v).replace("/", "_")


# ------------------------------------------------------------------------------------------------
# weights and inputs
# ------------------------------------------------------------------------------------------------
def make_state(level, hidden_blocks, dtype, seed=0):
    """A state dict for both ConvRefiner classes with activations that stay at a maximum of 4 to 8 through nine blocks.  The tensors of
    the blocks are rounded to `dtype` (what .to(dtype) of the yardstick would do), so that truth, yardstick and product start from the
    same numbers; disp_emb and out_conv stay fp32."""
    feat, emb, r = REFINER_SPEC[level]
    D = width(level)
    ref = oracle.ConvRefiner(D, D, 3, hidden_blocks, emb, r)
    g = torch.Generator().manual_seed(1000 * D + 10 * hidden_blocks + seed)
    state = {}
    for key, t in ref.state_dict().items():
        def normal(std):
            return torch.randn(t.shape, generator=g) * std

        def uniform(lo, hi):
            return torch.rand(t.shape, generator=g) * (hi - lo) + lo

        in_block = key.startswith(("block1.", "hidden_blocks."))
        if key.endswith("num_batches_tracked"):
            v = t.clone()
        elif key == "disp_emb.weight":
            v = normal(4.0)
        elif key == "out_conv.weight":
            v = normal(D ** -0.5)
        elif key.endswith(".0.weight"):
            v = normal(0.2)
        elif key.endswith(".3.weight"):
            v = normal((2.0 / D) ** 0.5)
        elif key.endswith(".1.weight"):
            v = uniform(0.8, 1.2)
        elif key.endswith("running_var"):
            v = uniform(0.5, 1.5)
        else:
            assert key.endswith(("bias", "running_mean")), key
            v = normal(0.1)
        if in_block and v.is_floating_point():
            v = v.to(dtype).float()
        state[key] = v
    ref.load_state_dict(state)
    return ref.eval()


class Inputs:
    def __init__(self, level, shape, dtype, seed=0):
        feat, emb, r = REFINER_SPEC[level]
        B, h, w = shape
        g = torch.Generator().manual_seed(7 * width(level) + h + seed)
        self.x = torch.randn((B, feat, h, w), generator=g).to(dtype)
        self.y = torch.randn((B, feat, h, w), generator=g).to(dtype)
        self.flow = (oracle.pixel_grid(B, h, w) + 0.05 * torch.randn((B, 2, h, w), generator=g)).contiguous()
        self.certainty = torch.randn((B, 1, h, w), generator=g)
        self.sx, self.sy = 1 / (4 * w), 1 / (4 * h)          # Decoder.forward: ins / (refine_init * W) on a map of W / ins columns

    def to(self, device):
        out = copy.copy(self)
        for k in ("x", "y", "flow", "certainty"):
            setattr(out, k, getattr(self, k).to(device))
        return out


# ------------------------------------------------------------------------------------------------
# the two references
# ------------------------------------------------------------------------------------------------
def local_corr_ref(f0, f1, r, flow):
    """oracle.local_correlation (the shared-fraction form: a 4-tap blend of integer-grid dot products on the (2r+2)^2 patch) in the
    dtype of its arguments."""
    B, C, h, w = f0.shape
    n = 2 * r + 1
    f1 = f1.reshape(B, C, h * w)
    px = ((flow[:, 0] + 1) * w - 1) / 2
    py = ((flow[:, 1] + 1) * h - 1) / 2
    x0, y0 = torch.floor(px), torch.floor(py)
    ax, ay = (px - x0)[:, None, None], (py - y0)[:, None, None]
    x0, y0 = x0.long(), y0.long()
    dots = f0.new_zeros(B, n + 1, n + 1, h, w)
    for j in range(n + 1):
        yy = y0 - r + j
        for i in range(n + 1):
            xx = x0 - r + i
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(B, 1, h * w).expand(B, C, h * w)
            dots[:, j, i] = (f0 * torch.gather(f1, 2, idx).reshape(B, C, h, w)).sum(dim=1) * ok
    dots = dots / math.sqrt(C)
    corr = (1 - ay) * ((1 - ax) * dots[:, :n, :n] + ax * dots[:, :n, 1:]) + ay * ((1 - ax) * dots[:, 1:, :n] + ax * dots[:, 1:, 1:])
    return corr.reshape(B, n * n, h, w)


def _blocks(ref):
    return [ref.block1] + list(ref.hidden_blocks)


def truth(ref, inp, sf, shift=0, mutant=None):
    """fp64 throughout.  ref: the oracle module holding make_state's weights (fp32 storage of dtype-rounded numbers: .double() is exact).
    Returns the last block's activation (B,D,h,w) and out_conv's two outputs.  `mutant` applies one of the mistakes of MUTANTS."""
    r = ref.local_corr_radius
    x, flow = inp.x.double(), inp.flow.double()
    y = inp.y.double().roll(-shift, 0)                                            # y_ref[b] = y[(b + shift) % B]
    B, C, h, w = x.shape
    y_warp = inp.y.double() if mutant == "warp_without_batch_shift" else y
    parts = [x, F.grid_sample(y_warp, flow.permute(0, 2, 3, 1), align_corners=False, mode="bilinear")]
    ys = torch.linspace(-1 + 1 / h, 1 - 1 / h, h, dtype=torch.float64, device=x.device)
    xs = torch.linspace(-1 + 1 / w, 1 - 1 / w, w, dtype=torch.float64, device=x.device)
    grid = torch.stack((xs[None, :].expand(h, w), ys[:, None].expand(h, w)), dim=0)[None]
    emb = F.conv2d(40 / 32 * sf * (flow - grid), ref.disp_emb.weight.double(), ref.disp_emb.bias.double())
    parts.append(emb.roll(1, 1) if mutant == "embedding_rolled" else emb)
    if r:
        corr = local_corr_ref(x, y, r, flow)
        parts.append(corr.roll(1, 1) if mutant == "correlation_rolled" else corr)
    blocks = [copy.deepcopy(b).double() for b in _blocks(ref)]
    if mutant == "block_skipped":
        blocks = blocks[:-1]
    elif mutant == "block_weights_reused":
        blocks[0] = blocks[1]
    elif mutant == "tap_zeroed":                                                  # the largest tap of channel 0: a choice from the weights alone
        wt = blocks[0][0].weight
        wt[0].view(-1)[wt[0].abs().argmax()] = 0.0
    d = torch.cat(parts, dim=1)
    for blk in blocks:
        d = blk(d)
    out = F.conv2d(d, ref.out_conv.weight.double(), ref.out_conv.bias.double())
    return {"act": d, "dflow": out[:, :-1], "dcert": out[:, -1:]}


MUTANTS = ["embedding_rolled", "warp_without_batch_shift", "correlation_rolled", "block_skipped", "block_weights_reused", "tap_zeroed"]


def yardstick(ref, inp, sf, dtype, shift=0):
    """The reference under autocast: see the module docstring.  Runs where inp lives; channels-last on the device."""
    r = ref.local_corr_radius
    x, flow = inp.x, inp.flow
    y = inp.y.roll(-shift, 0)
    B, C, h, w = x.shape
    parts = [x, F.grid_sample(y.float(), flow.permute(0, 2, 3, 1), align_corners=False, mode="bilinear").to(dtype)]
    grid = oracle.pixel_grid(B, h, w, x.device)
    parts.append(F.conv2d(40 / 32 * sf * (flow - grid), ref.disp_emb.weight, ref.disp_emb.bias).to(dtype))
    if r:
        parts.append(oracle.local_correlation(x, y, r, flow=flow))                # fp32 inside, rounded to x's dtype once
    d = torch.cat(parts, dim=1)
    assert d.dtype == dtype
    if x.is_cuda:
        d = d.contiguous(memory_format=torch.channels_last)
    for blk in _blocks(ref):
        d = copy.deepcopy(blk).to(dtype)(d)
    assert d.dtype == dtype
    out = F.conv2d(d.float(), ref.out_conv.weight, ref.out_conv.bias)
    return {"act": d, "dflow": out[:, :-1], "dcert": out[:, -1:]}


def updated(inp, res, certainty):
    """What Decoder.forward makes of out_conv's outputs (flow + (sx dx, sy dy), certainty + dcert), in res's precision."""
    flow = inp.flow.to(res["dflow"].dtype)
    s = torch.tensor([inp.sx, inp.sy], dtype=flow.dtype, device=flow.device).view(1, 2, 1, 1)
    return {"flow": flow + s * res["dflow"], "cert": res["dcert"] if certainty is None else certainty.to(flow.dtype) + res["dcert"]}


def maxdiff(a, b, inp=None):
    """max |a - b|; for an updated flow divided by (sx, sy): the units of out_conv."""
    d = (a.double() - b.double()).abs()
    if inp is not None:
        d = d / torch.tensor([inp.sx, inp.sy], dtype=torch.float64, device=d.device).view(1, 2, 1, 1)
    return float(d.max())


# ------------------------------------------------------------------------------------------------
# CPU: the references agree with the oracle, and the bound can fail
# ------------------------------------------------------------------------------------------------
def test_local_corr_ref_is_the_oracles_and_the_literal_form():
    g = torch.Generator().manual_seed(11)
    B, C, h, w, r = 2, 24, 9, 13, 2
    f0, f1 = torch.randn((B, C, h, w), generator=g), torch.randn((B, C, h, w), generator=g)
    flow = oracle.pixel_grid(B, h, w) + 0.3 * torch.randn((B, 2, h, w), generator=g)           # windows past every border
    got = local_corr_ref(f0.double(), f1.double(), r, flow.double())
    assert got.dtype == torch.float64
    assert maxdiff(got, oracle.local_correlation(f0, f1, r, flow=flow)) < 1e-5
    # romatch/utils/local_correlation.py: one grid_sample per window offset ((ix - r) 2 / w, (iy - r) 2 / h), k = iy (2r + 1) + ix
    lit = []
    for iy in range(-r, r + 1):
        for ix in range(-r, r + 1):
            off = torch.tensor([ix * 2 / w, iy * 2 / h], dtype=torch.float64).view(1, 2, 1, 1)
            s = F.grid_sample(f1.double(), (flow.double() + off).permute(0, 2, 3, 1), align_corners=False, mode="bilinear")
            lit.append((f0.double() * s).sum(dim=1) / math.sqrt(C))
    assert maxdiff(got, torch.stack(lit, dim=1)) < 1e-9


def test_product_module_takes_the_state_dict():
    for level in REFINER_SPEC:
        feat, emb, r = REFINER_SPEC[level]
        D = width(level)
        ref = make_state(level, 1, torch.float16)
        m = matcher.ConvRefiner(D, D, 3, hidden_blocks=1, displacement_emb_dim=emb, local_corr_radius=r)
        m.load_state_dict(ref.state_dict())                                         # strict: the same key layout
        assert matcher.padded_width(D) == {24: 24, 144: 144, 569: 576, 1137: 1152, 1377: 1408}[D]


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("hidden_blocks", [0, 2, 8])
@pytest.mark.parametrize("D", [24, 144, 569])
def test_mutants_of_truth_are_far_outside_the_bound(D, hidden_blocks, dtype):
    """On the CPU, the symmetric form (y = x, batch_shift = B/2) on a (2, 19, 23) map: every mutant that exists for the case is at least
    MUTANT_FACTOR x (2 e_lib) from truth in the last block's activation — the tap mutant at hidden_blocks = 0 only (deeper, one tap of
    one channel is printed, not asserted)."""
    level = BY_WIDTH[D]
    sf = SF2 if hidden_blocks == 2 else 1.0
    ref = make_state(level, hidden_blocks, dtype)
    inp = Inputs(level, MAPS[0], dtype)
    inp.y = inp.x
    shift = MAPS[0][0] // 2
    t = truth(ref, inp, sf, shift)["act"]
    e_lib = maxdiff(yardstick(ref, inp, sf, dtype, shift)["act"], t)
    bound = 2 * e_lib
    print(f"D={D} blocks={hidden_blocks} {_name(dtype)}: max|act| {float(t.abs().max()):.2f}  e_lib {e_lib:.3e}")
    assert 2.0 < float(t.abs().max()) < 16.0                                        # the signal neither died nor blew up
    for mutant in MUTANTS:
        if (mutant == "correlation_rolled" and not ref.local_corr_radius) or (mutant == "block_weights_reused" and hidden_blocks == 0):
            continue
        e = maxdiff(truth(ref, inp, sf, shift, mutant)["act"], t)
        print(f"    {mutant:26s} {e:.3e} = {e / bound:7.1f} x the bound")
        if mutant != "tap_zeroed" or hidden_blocks == 0:
            assert e >= MUTANT_FACTOR * bound, (mutant, e, bound)


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def poisoned_empty(monkeypatch):
    """A context manager under which torch.empty / torch.empty_like return floating-point tensors full of NaN: whatever the product
    reads without having written it shows."""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t

    @contextlib.contextmanager
    def ctx():
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
            m.setattr(torch, "empty_like", lambda *a, **k: fill(real_empty_like(*a, **k)))
            yield
    return ctx


@pytest.fixture
def assemble_calls(monkeypatch):
    """Counts the calls of ops.refiner_assemble (the fused assembly)."""
    calls = []
    real = matcher.ops.refiner_assemble

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(matcher.ops, "refiner_assemble", spy)
    return calls


# the op that runs the 1x1 of a block (or the whole block) per forced implementation; split_gemm's is torch.addmm
BLOCK_OP = {"fused": "refiner_block", "split_mfma/one": "refiner_block_mid", "split_mfma/two": "pointwise_mfma", "wide": "refiner_block_wide"}


@pytest.fixture
def block_calls(monkeypatch):
    """Counts the calls of the ops of BLOCK_OP by name."""
    calls = {}
    for op in BLOCK_OP.values():
        def spy(*a, _op=op, _real=getattr(matcher.ops, op), **k):
            calls[_op] = calls.get(_op, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(matcher.ops, op, spy)
    return calls


@functools.lru_cache(maxsize=2)
def references(level, shape, hidden_blocks, dtype):
    """Module, inputs, truth and yardstick of one case on the device, both forms: "sep" (a separate y) and "sym" (y = x, batch_shift =
    B/2).  Shared by the implementations of a level; nothing here is modified by a test."""
    sf = MAP_SF[shape]
    ref = make_state(level, hidden_blocks, dtype).to(DEV)
    inp = Inputs(level, shape, dtype).to(DEV)
    sym = copy.copy(inp)
    sym.y = sym.x
    shift = shape[0] // 2
    out = {"ref": ref, "sf": sf, "shift": shift, "sep": (inp, truth(ref, inp, sf), None), "sym": (sym, truth(ref, sym, sf, shift), None)}
    if dtype != torch.float32:
        out["sep"] = (inp, out["sep"][1], yardstick(ref, inp, sf, dtype))
        out["sym"] = (sym, out["sym"][1], yardstick(ref, sym, sf, dtype, shift))
    return out


def product_module(level, ref, hidden_blocks, dtype):
    feat, emb, r = REFINER_SPEC[level]
    D = width(level)
    m = matcher.ConvRefiner(D, D, 3, hidden_blocks=hidden_blocks, displacement_emb_dim=emb, local_corr_radius=r, amp_dtype=dtype)
    m.load_state_dict(ref.state_dict())
    return m.to(DEV).eval()


def pitched_channels_last(t):
    """t (B,C,h,w) as channels [0, C) of a channels-last buffer whose pitch is C rounded up to 16 — what Decoder.project hands over."""
    B, C, h, w = t.shape
    buf = torch.zeros((B, h, w, (C + 15) // 16 * 16), dtype=t.dtype, device=t.device)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return buf[..., :C].permute(0, 3, 1, 2)


def run_entry(m, entry, inp, sf, shift, dtype, poison=False):
    """One call of the product the way `entry` describes; returns {name: tensor}."""
    if entry in ("a", "b"):
        y = inp.y.contiguous() if entry == "a" else pitched_channels_last(inp.y)
        flow = inp.flow.clone()
        out = {}
        if entry == "a":
            cur, P = m._body(inp.x, y, flow, sf, dtype)
            assert cur.shape[-1] == P.Dp and cur.dtype == dtype
            out["act"] = cur[..., :P.D].permute(0, 3, 1, 2).clone()
        out["dflow"], out["dcert"] = m.forward(inp.x, y, flow, scale_factor=sf, dtype=dtype)
        assert torch.equal(flow, inp.flow)
        return out
    B, C, h, w = inp.x.shape
    buf = m.new_buffer(B, h, w, dtype, inp.x.device)
    if poison:
        buf.fill_(float("nan"))
    buf[..., :C] = inp.x.permute(0, 2, 3, 1)
    x = buf[..., :C].permute(0, 3, 1, 2)
    flow = inp.flow.clone()
    certainty = inp.certainty.clone() if entry == "c" else None
    got_flow, cert = m.forward_update(x, x, flow, certainty, sf, inp.sx, inp.sy, dtype=dtype, buf=buf, batch_shift=shift)
    assert got_flow.data_ptr() == flow.data_ptr()                                   # updated in place
    return {"flow": got_flow, "cert": cert}


def expected(entry, inp, res):
    if entry in ("a", "b"):
        return res
    return updated(inp, res, inp.certainty if entry == "c" else None)


def force(monkeypatch, impl):
    block, _, mid = impl.partition("/")
    monkeypatch.setattr(matcher, "block_impl", lambda *a: block)
    if mid:
        monkeypatch.setattr(matcher, "mid_block_impl", lambda *a: mid)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("level,dtype,impl", IMPLS, ids=_name)                     # the inner loop: the implementations of a level share a reference
@pytest.mark.parametrize("shape,hidden_blocks", [(MAPS[0], 0), (MAPS[0], 2), (MAPS[0], 8), (MAPS[1], 0), (MAPS[1], 2)], ids=_name)
def test_module_within_twice_the_library_error(shape, hidden_blocks, level, dtype, impl, monkeypatch, poisoned_empty, assemble_calls,
                                               block_calls):
    R = references(level, shape, hidden_blocks, dtype)
    m = product_module(level, R["ref"], hidden_blocks, dtype)
    P = m.prepare(dtype)                                                            # with the real block_impl
    assert impl.split("/")[0] in P.blocks, (impl, list(P.blocks))
    force(monkeypatch, impl)
    tag = f"REFINER16 D={P.D} {_name(dtype)} {impl} {_name(shape)} blocks={hidden_blocks}"
    failures = []
    for entry in "abcd":
        inp, t, lib = R["sep" if entry in "ab" else "sym"]
        shift = 0 if entry in "ab" else R["shift"]
        del assemble_calls[:]
        got = run_entry(m, entry, inp, R["sf"], shift, dtype)
        assert len(assemble_calls) == (0 if entry == "a" else 1), (entry, len(assemble_calls))   # (a) split assembly, (b)-(d) fused
        with poisoned_empty():
            again = run_entry(m, entry, inp, R["sf"], shift, dtype, poison=True)
        torch.cuda.synchronize()
        want_t, want_lib = expected(entry, inp, t), expected(entry, inp, lib)
        for name, g in got.items():
            assert torch.isfinite(g).all() and torch.isfinite(again[name]).all(), (entry, name, "not finite")
            assert torch.equal(_bits(g), _bits(again[name])), (entry, name, "the result depends on memory the module never wrote")
            scaled = inp if name == "flow" else None
            e_lib, e_hip = maxdiff(want_lib[name], want_t[name], scaled), maxdiff(g, want_t[name], scaled)
            print(f"{tag} entry={entry} {name}: e_lib {e_lib:.3e} e_hip {e_hip:.3e} max|truth| {float(want_t[name].abs().max()):.2f}")
            if not e_hip <= 2 * e_lib:
                failures.append((entry, name, e_hip, e_lib))
    # the forced implementation is what ran: ten passes through _body ((a) makes two, and every entry runs again poisoned)
    assert block_calls == ({BLOCK_OP[impl]: 10 * (hidden_blocks + 1)} if impl in BLOCK_OP else {}), block_calls
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("level", list(REFINER_SPEC))
def test_module_fp32_control(level, poisoned_empty):
    """The same harness in fp32 against truth, at the golden test's bar scaled to these activations: the harness and the mapping of the
    weights agree with the product at the shipped widths before any 16-bit judgement."""
    dtype, shape, hidden_blocks = torch.float32, MAPS[0], 8
    R = references(level, shape, hidden_blocks, dtype)
    m = product_module(level, R["ref"], hidden_blocks, dtype)
    for entry in "abcd":
        inp, t, _ = R["sep" if entry in "ab" else "sym"]
        shift = 0 if entry in "ab" else R["shift"]
        got = run_entry(m, entry, inp, R["sf"], shift, dtype)
        with poisoned_empty():
            again = run_entry(m, entry, inp, R["sf"], shift, dtype, poison=True)
        torch.cuda.synchronize()
        want = expected(entry, inp, t)
        for name, g in got.items():
            assert torch.isfinite(g).all() and torch.equal(_bits(g), _bits(again[name])), (entry, name)
            unit = t["dflow"] if name == "flow" else want[name]                     # the flow is compared in out_conv's units
            bound = 5e-5 * max(1.0, float(unit.abs().max()))
            e = maxdiff(g, want[name], inp if name == "flow" else None)
            print(f"REFINER32 D={width(level)} entry={entry} {name}: e_hip {e:.3e} bound {bound:.3e}")
            assert e <= bound, (entry, name, e, bound)
