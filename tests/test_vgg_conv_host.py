"""The fused VGG19 layer's host side: the static per-layer choice and the argument checks of the two new entry points (no GPU)."""
import ctypes

import torch

from roma_amd import _lib, encoders, ops


def test_choice_is_library_for_everything_unmeasured():
    f = encoders.vgg_conv_impl
    assert f(torch.float32, True, 64, 64, 2, 560, 560) == "library"
    assert f(torch.bfloat16, True, 64, 64, 2, 560, 560) == "library"
    assert f(torch.float16, False, 64, 64, 2, 560, 560) == "library"           # planar maps
    assert f(torch.float16, True, 3, 64, 2, 560, 560) == "library"             # the stem
    assert f(torch.float16, True, 3, 64, 2, 864, 864) == "library"
    for cin, cout in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)):
        assert f(torch.float16, True, cin, cout, 1, 8, 8) == "library"         # far below every measured size
        assert f(torch.float16, True, cin, cout, 64, 1024, 1024) == "library"  # far above
    assert f(torch.float16, True, 96, 96, 2, 560, 560) == "library"            # not a VGG19 layer


def test_table_rows_are_ranges_of_existing_instances():
    n = len(ops.conv3x3_instances())
    assert n == _lib.load().roma_conv3x3_bias_relu_instances(0, None, 0) and 0 < n <= 12
    assert len(set(ops.conv3x3_instances())) == n                               # every instance is a distinct configuration
    for (cin, cout), rows in encoders.VGG_CONV_TABLE.items():
        assert cin % 8 == 0 and cout % 8 == 0 and cin > 3
        for lo, hi, inst in rows:
            assert 0 < lo <= hi and 0 <= inst < n
            H = W = int(round((lo / 2) ** 0.5))
            if 2 * H * W == lo:
                assert encoders.vgg_conv_impl(torch.float16, True, cin, cout, 2, H, W) == inst


def test_conv_entry_point_validates_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_uint16 * 4096)()
    base = ctypes.addressof(buf)
    a = (base + 15) // 16 * 16
    conv = lib.roma_conv3x3_bias_relu
    assert conv(None, a, a, a, 1, 8, 8, 4, 4, _lib.ROMA_F16, 8, 8, 0, None) == _lib.ROMA_E_ARG and b"null pointer" in lib.roma_last_error()
    assert conv(a, a, a, None, 1, 8, 8, 4, 4, _lib.ROMA_F16, 8, 8, 0, None) == _lib.ROMA_E_ARG
    assert conv(a, a, a, a, 1, 8, 8, 4, 4, _lib.ROMA_F32, 8, 8, 0, None) == _lib.ROMA_E_UNSUPPORTED
    assert conv(a, a, a, a, 1, 8, 8, 4, 4, 7, 8, 8, 0, None) == _lib.ROMA_E_DTYPE
    assert conv(a, a, a, a, 1, 8, 8, 0, 4, _lib.ROMA_F16, 8, 8, 0, None) == _lib.ROMA_E_SHAPE
    assert conv(a, a, a, a, 1, 16, 8, 4, 4, _lib.ROMA_F16, 8, 8, 0, None) == _lib.ROMA_E_SHAPE              # x_pitch < Cin
    assert conv(a, a, a, a, 2, 64, 64, 40000, 40000, _lib.ROMA_F16, 64, 64, 0, None) == _lib.ROMA_E_SHAPE   # past 2^31 elements
    assert conv(a, a, a, a, 1, 12, 8, 4, 4, _lib.ROMA_F16, 16, 8, 0, None) == _lib.ROMA_E_ALIGN and b"multiples of 8" in lib.roma_last_error()
    assert conv(a, a, a, a, 1, 8, 12, 4, 4, _lib.ROMA_F16, 8, 16, 0, None) == _lib.ROMA_E_ALIGN
    assert conv(a, a, a, a, 1, 8, 8, 4, 4, _lib.ROMA_F16, 12, 8, 0, None) == _lib.ROMA_E_ALIGN              # pitch
    for k in range(4):                                                                                       # each buffer misaligned
        ptrs = [a, a, a, a]
        ptrs[k] = a + 2
        assert conv(*ptrs, 1, 8, 8, 4, 4, _lib.ROMA_F16, 8, 8, 0, None) == _lib.ROMA_E_ALIGN
    n = lib.roma_conv3x3_bias_relu_instances(0, None, 0)
    assert conv(a, a, a, a, 1, 8, 8, 4, 4, _lib.ROMA_F16, 8, 8, n, None) == _lib.ROMA_E_ARG and b"instance" in lib.roma_last_error()
    assert conv(a, a, a, a, 1, 8, 8, 4, 4, _lib.ROMA_F16, 8, 8, -1, None) == _lib.ROMA_E_ARG
    name = ctypes.create_string_buffer(8)
    assert lib.roma_conv3x3_bias_relu_instances(n, name, 8) == _lib.ROMA_E_ARG
    assert lib.roma_conv3x3_bias_relu_instances(0, name, 8) == n and len(name.value) == 7                    # truncated, terminated


def test_maxpool_entry_point_validates_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_uint16 * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    pool = lib.roma_maxpool2_nhwc
    assert pool(None, a, 1, 8, 2, 2, _lib.ROMA_F16, None) == _lib.ROMA_E_ARG and b"null pointer" in lib.roma_last_error()
    assert pool(a, None, 1, 8, 2, 2, _lib.ROMA_F16, None) == _lib.ROMA_E_ARG
    assert pool(a, a, 1, 8, 2, 2, 9, None) == _lib.ROMA_E_DTYPE
    assert pool(a, a, 1, 8, 3, 2, _lib.ROMA_F16, None) == _lib.ROMA_E_SHAPE
    assert pool(a, a, 1, 8, 2, 5, _lib.ROMA_F16, None) == _lib.ROMA_E_SHAPE
    assert pool(a, a, 1, 12, 2, 2, _lib.ROMA_F16, None) == _lib.ROMA_E_ALIGN
    assert pool(a, a, 1, 6, 2, 2, _lib.ROMA_F32, None) == _lib.ROMA_E_ALIGN
    assert pool(a + 2, a, 1, 8, 2, 2, _lib.ROMA_F16, None) == _lib.ROMA_E_ALIGN


def test_new_ops_refuse_cpu_tensors():
    import pytest
    x = torch.zeros(1, 8, 4, 4, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(8, 8, 3, 3, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv3x3_bias_relu(x, w, torch.zeros(8, dtype=torch.float16), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.maxpool2_nhwc(x)
