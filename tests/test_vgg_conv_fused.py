"""ops.conv3x3_bias_relu (a VGG19-BN layer in one kernel), ops.maxpool2_nhwc and the fused path through VGG19.forward.

The yardstick is the fp32 convolution of the same fp16 operands followed by the layer's two roundings, relu(fp16(conv) + bias) -> fp16.
The tolerance is measured inside each test: the path the fused kernel replaces (F.conv2d in fp16 + ops.bias_relu_) is compared with the
same yardstick on the same inputs, and the fused kernel may be at most twice as far away (both sum in fp32; only the order differs).

Measured on MI355X (max |difference| to the yardstick over the three map sizes, library / worst of the ten instances; the fp16 spacing
of the results is 9.8e-4):
    (64,64) 1.95e-3 / 1.95e-3    (64,128) 1.95e-3 / 1.95e-3    (128,128) 1.95e-3 / 1.95e-3    (128,256) 1.95e-3 / 1.95e-3
    (256,256) 3.91e-3 / 1.95e-3    (256,512) 2.93e-3 / 1.95e-3    (512,512) 3.91e-3 / 1.95e-3
pyramid at 64 x 96 (library / fused against the fp32 pyramid): scale 1 1.46e-3 / 1.46e-3, 2 4.8e-4 / 4.8e-4, 4 4.0e-4 / 3.0e-4,
8 4.6e-4 / 2.9e-4.
"""
import pytest
import torch
import torch.nn.functional as F

from roma_amd import encoders, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHANNELS = [(64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]
MAPS = [(5, 7), (16, 24), (33, 20)]          # B = 2: 70, 768 and 1320 pixels — 1320 is no multiple of 256, 128 or 64 (MPerBlock)


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def operands(cin, cout, H, W, seed=0):
    """Zero-mean operands: the edge-property tests."""
    g = torch.Generator().manual_seed(1000 * cin + cout + H + seed)
    x = torch.randn(2, cin, H, W, generator=g).half()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).half()
    b = (torch.randn(cout, generator=g) * 0.25).half()
    return nhwc(x.to(DEV)), nhwc(w.to(DEV)), b.to(DEV)


def one_binade_operands(cin, cout, H, W):
    """Operands for a max-|difference| comparison that measures the summation and not the luck of WHICH element differs.  Sums of
    the same products in another order differ by far less than an fp16 spacing, so after the rounding to fp16 a path differs from
    the yardstick by whole spacings, in some elements only — and the spacing is 4.9e-4 below 1, 9.8e-4 in [1, 2), 2.0e-3 in [2, 4).
    With zero-mean data the largest difference is the spacing at whichever element happened to differ, a factor of 4 apart between
    two equally good kernels (measured: 4.9e-4 for the library against 2.0e-3 for a fused instance at (128,256), 5 x 7).  Here x in [0.5, 1.5) and w in [0.25, 1.75) * 1.5 / (9 Cin) put every interior convolution
    sum at 1.5 +- 0.15 and the border sums (6 or 4 taps of 9) below that; |bias| <= 0.3 keeps the result below 2.  Every 16th
    channel gets bias -1.5 instead, so that its results straddle the ReLU's zero.  All operands are normal fp16 numbers."""
    g = torch.Generator().manual_seed(1000 * cin + cout + H)
    x = (torch.rand(2, cin, H, W, generator=g) + 0.5).half()
    w = ((torch.rand(cout, cin, 3, 3, generator=g) * 1.5 + 0.25) * (1.5 / (9 * cin))).half()
    b = (torch.rand(cout, generator=g) * 0.6 - 0.3)
    b[::16] = -1.5
    return nhwc(x.to(DEV)), nhwc(w.to(DEV)), b.half().to(DEV)


def yardstick(x, w, b):
    """On the CPU: the device's fp32 convolution is itself one to two fp16 spacings away from this one on these operands."""
    acc = F.conv2d(x.float().cpu(), w.float().cpu(), None, padding=1).to(x.device)
    return torch.relu(acc.half().float() + b.float()[None, :, None, None]).half()


def library(x, w, b):
    return ops.bias_relu_(F.conv2d(x, w, None, padding=1), b)


def instances_under_test():
    used = {inst for rows in encoders.VGG_CONV_TABLE.values() for _, _, inst in rows}
    return sorted(used | set(range(len(ops.conv3x3_instances()))))       # what the table uses, and what the tuning tool may put there


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_conv_matches_fp32_reference_within_twice_the_library_error(cin, cout, miopen_find):
    worst_lib = worst_fused = 0.0
    for H, W in MAPS:
        x, w, b = one_binade_operands(cin, cout, H, W)
        ref = yardstick(x, w, b).float()
        dev32 = torch.relu(F.conv2d(x.float(), w.float(), None, padding=1).half().float() + b.float()[None, :, None, None]).half()
        print(f"({cin},{cout}) {H}x{W} device fp32 convolution against the CPU's: {float((dev32.float() - ref).abs().max()):.3e}")
        e_lib = float((library(x, w, b).float() - ref).abs().max())
        worst_lib = max(worst_lib, e_lib)
        for inst in instances_under_test():
            y = ops.conv3x3_bias_relu(x, w, b, inst)
            assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
            e = float((y.float() - ref).abs().max())
            worst_fused = max(worst_fused, e)
            clipped = float((ref == 0).float().mean())
            assert 0.005 < clipped < 0.06 and float(ref.max()) < 2.0, (clipped, float(ref.max()))    # the ReLU is exercised, one binade
            print(f"({cin},{cout}) {H}x{W} instance {inst}: fused {e:.3e}  library {e_lib:.3e}")
            assert e <= 2 * e_lib, (cin, cout, H, W, inst, e, e_lib)
    print(f"({cin},{cout}) worst: library {worst_lib:.3e}  fused {worst_fused:.3e}")


@pytest.mark.parametrize("inst", range(len(ops.conv3x3_instances())))
def test_edge_properties(inst):
    x, w, b = operands(64, 64, 9, 11, seed=inst)
    # a bias far below anything the convolution can reach: all zeros
    y = ops.conv3x3_bias_relu(x, w, torch.full_like(b, -1000.0), inst)
    assert int(torch.count_nonzero(y)) == 0
    # channels with zero weights: exactly relu(bias) everywhere, the padded border included
    w0 = w.clone()
    w0[3] = 0
    w0[5] = 0
    b0 = b.clone()
    b0[3], b0[5] = 0.3701, -0.25
    y = ops.conv3x3_bias_relu(x, nhwc(w0), b0, inst)
    assert bool((y[:, 3] == b0[3]).all()) and bool((y[:, 5] == 0).all())
    assert torch.equal(y[:, :3], ops.conv3x3_bias_relu(x, w, b, inst)[:, :3])
    # a write into the first 64 channels of an 80-channel map leaves the other 16 alone
    wide = torch.full((2, 9, 11, 80), 7.0, dtype=torch.float16, device=DEV).permute(0, 3, 1, 2)
    out = ops.conv3x3_bias_relu(x, w, b, inst, out=wide[:, :64])
    assert out.data_ptr() == wide.data_ptr() and bool((wide[:, 64:] == 7.0).all())
    assert torch.equal(wide[:, :64], ops.conv3x3_bias_relu(x, w, b, inst))
    # and a read from a channel slice of a wider map
    xin = torch.randn(2, 9, 11, 80, device=DEV).half().permute(0, 3, 1, 2)
    assert torch.equal(ops.conv3x3_bias_relu(xin[:, :64], w, b, inst), ops.conv3x3_bias_relu(nhwc(xin[:, :64]), w, b, inst))


@pytest.mark.parametrize("shape", [(2, 64, 6, 10), (2, 512, 4, 6), (1, 128, 34, 18)])
def test_maxpool_has_the_bits_of_the_fused_epilogue_pool(shape):
    g = torch.Generator().manual_seed(shape[1])
    x = nhwc(torch.randn(*shape, generator=g).half().to(DEV))
    b = (torch.randn(shape[1], generator=g) * 0.5).half().to(DEV)
    pooled = ops.bias_relu_pool2_(x, b)                          # x now holds relu(x + b)
    got = ops.maxpool2_nhwc(x)
    assert got.shape == pooled.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, pooled)
    assert torch.equal(got, F.max_pool2d(x, 2, 2))
    xb = nhwc(torch.randn(*shape, generator=g).to(DEV).bfloat16())
    assert torch.equal(ops.maxpool2_nhwc(xb), F.max_pool2d(xb, 2, 2))
    xf = nhwc(torch.randn(*shape, generator=g).to(DEV))
    assert torch.equal(ops.maxpool2_nhwc(xf), F.max_pool2d(xf, 2, 2))


def test_pyramid_fused_everywhere_against_library_everywhere(miopen_find):
    torch.manual_seed(3)
    net = encoders.VGG19().to(DEV).eval()
    for m in net.layers:                                         # BatchNorm statistics that do something
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.8, 1.2)
            m.bias.data.normal_(0, 0.1)
    x = torch.randn(2, 3, 64, 96, device=DEV)
    ref = net(x, torch.float32)
    net.conv_impl = lambda *a: "library"
    lib = net(x, torch.float16)
    calls = []

    def everywhere(dtype, channels_last, cin, cout, B, H, W):
        fused = dtype == torch.float16 and channels_last and cin % 8 == 0
        calls.append(fused)
        return 2 if fused else "library"                         # 128 x 128 tile: supports every VGG19 shape (padded GEMM)
    net.conv_impl = everywhere
    fus = net(x, torch.float16)
    assert calls.count(True) == 11 and calls.count(False) == 1   # every layer but the stem
    assert sorted(fus) == sorted(lib) == sorted(ref) == [1, 2, 4, 8]
    for s in (1, 2, 4, 8):
        assert fus[s].shape == lib[s].shape and fus[s].dtype == torch.float16
        e_lib = float((lib[s].float() - ref[s]).abs().max())
        e_fus = float((fus[s].float() - ref[s]).abs().max())
        print(f"scale {s}: library {e_lib:.3e}  fused {e_fus:.3e}  fused vs library {float((fus[s].float() - lib[s].float()).abs().max()):.3e}")
        assert e_fus <= 2 * e_lib, (s, e_fus, e_lib)
