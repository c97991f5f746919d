"""JPEG decoding for match() on file paths (matcher.py:606-637, 667-676: `Image.open(path).convert("RGB")`).
Host part (roma_jpeg_info / roma_jpeg_entropy_decode, no GPU) + the numpy restatement of libjpeg's reconstruction
(oracle/jpeg_oracle.py) against PIL itself: bit-identical — that pins the restatement; the GPU test then holds roma_jpeg_reconstruct
to the same images.  The host part reads bytes from outside, so malformed streams (crafted ones and a seeded mutation sweep) are held
to a known return code and to the blocks roma_jpeg_info announced, with a guard band behind the coefficient array."""
import glob
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from roma_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "assets", "*.jpg")))


GUARD, SENTINEL = 1024, 0x5A5A                                  # blocks behind the coefficient array that no call may touch, and what they hold
OK_CODES = (0, _lib.ROMA_E_ARG, _lib.ROMA_E_UNSUPPORTED)


def _host_decode(data, guard=0):
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(8, np.int32)
    rc = lib.roma_jpeg_info(buf.ctypes.data, len(data), info.ctypes.data)
    if rc != 0:
        return rc, None, None, None
    nb = int(info[4]) * int(info[5]) + 2 * int(info[6]) * int(info[7])
    room = np.full((nb + guard, 64), SENTINEL, np.int16)
    coef = room[:nb]
    coef[:] = 0
    qt = np.zeros((3, 64), np.uint16)
    rc = lib.roma_jpeg_entropy_decode(buf.ctypes.data, len(data), coef.ctypes.data, qt.ctypes.data)
    assert (room[nb:] == SENTINEL).all(), "roma_jpeg_entropy_decode wrote behind the blocks roma_jpeg_info announced"
    return rc, info, coef, qt


def _synthetic_jpegs():
    """Streams the bundled photographs do not cover: 4:4:4, 4:2:2, grey, odd sizes, restart intervals, optimised Huffman tables, and
    PROGRESSIVE streams (spectral selection + successive approximation; a bundled photograph re-encoded that way)."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:97, 0:131]
    base = np.stack([127 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 127 + 90 * np.cos(xx / 5.0 + yy / 11.0), 40 + 1.5 * xx], axis=2)
    img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
    out = {}
    for name, im, kw in [("444", Image.fromarray(img), dict(subsampling=0, quality=90)),
                         ("420_odd", Image.fromarray(img[:95, :129]), dict(subsampling=2, quality=75)),
                         ("grey", Image.fromarray(img[..., 0]), dict(quality=85)),
                         ("420_opt", Image.fromarray(img), dict(subsampling=2, quality=60, optimize=True)),
                         ("420_rst", Image.fromarray(img), dict(subsampling=2, quality=80, restart_marker_blocks=3)),
                         ("tiny", Image.fromarray(img[:5, :3]), dict(subsampling=2, quality=95)),
                         ("422", Image.fromarray(img), dict(subsampling=1, quality=85)),
                         ("422_odd", Image.fromarray(img[:33, :61]), dict(subsampling=1, quality=70)),
                         ("422_tiny", Image.fromarray(img[:9, :4]), dict(subsampling=1, quality=90)),
                         ("prog_420", Image.fromarray(img), dict(progressive=True, quality=80)),
                         ("prog_444", Image.fromarray(img), dict(progressive=True, subsampling=0, quality=92)),
                         ("prog_422_odd", Image.fromarray(img[:95, :129]), dict(progressive=True, subsampling=1, quality=60)),
                         ("prog_grey", Image.fromarray(img[..., 0]), dict(progressive=True, quality=85)),
                         ("prog_rst", Image.fromarray(img), dict(progressive=True, quality=75, restart_marker_blocks=4)),
                         ("prog_photo", Image.open(ASSETS[1]).convert("RGB"), dict(progressive=True, quality=88, optimize=True))]:
        bio = io.BytesIO()
        try:
            im.save(bio, "JPEG", **kw)
        except TypeError:                                       # an older Pillow without restart_marker_blocks
            continue
        out[name] = bio.getvalue()
    return out


def test_host_entropy_decoder_and_restatement_are_bit_identical_to_pil():
    from oracle import jpeg_oracle
    streams = {os.path.basename(f): open(f, "rb").read() for f in ASSETS}
    streams.update(_synthetic_jpegs())
    assert len(streams) >= 16
    for name, data in streams.items():
        rc, info, coef, qt = _host_decode(data)
        assert rc == 0, (name, rc, _lib.load().roma_last_error())
        ref = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
        mine = jpeg_oracle.reconstruct(coef, qt, info)
        assert mine.shape == ref.shape and np.array_equal(mine, ref), name


def test_streams_outside_the_supported_subset_are_refused_not_misdecoded():
    img = Image.fromarray((np.arange(64 * 64 * 3) % 251).astype(np.uint8).reshape(64, 64, 3))
    bio = io.BytesIO()
    img.convert("CMYK").save(bio, "JPEG")                       # four components
    rc, *_ = _host_decode(bio.getvalue())
    assert rc == _lib.ROMA_E_UNSUPPORTED
    bio = io.BytesIO()
    try:
        img.save(bio, "JPEG", keep_rgb=True)                    # three components stored as RGB (Adobe marker, no YCbCr transform)
        rc, *_ = _host_decode(bio.getvalue())
        assert rc == _lib.ROMA_E_UNSUPPORTED
    except TypeError:                                           # an older Pillow without keep_rgb
        pass
    rc, *_ = _host_decode(b"\x89PNG\r\n\x1a\n" + b"\0" * 64)
    assert rc == _lib.ROMA_E_ARG
    data = open(ASSETS[0], "rb").read()
    rc, *_ = _host_decode(data[:600])                           # truncated inside the tables
    assert rc < 0


def _segments(data):
    """(marker, offset of its 0xFF, offset behind the segment) of every marker segment up to EOI, stepping over the entropy-coded data"""
    out, i = [], 2
    while i + 4 <= len(data) and data[i:i + 2] != b"\xff\xd9":
        m = data[i + 1]
        if data[i] != 0xFF or m in (0x00, 0xFF) or 0xD0 <= m <= 0xD7:
            i += 1
            continue
        end = i + 2 + int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, i, end))
        i = end
    return out


def _encode(arr, **kw):
    bio = io.BytesIO()
    Image.fromarray(arr).save(bio, "JPEG", **kw)
    return bio.getvalue()


def _pattern(h, w):
    return ((np.arange(h * w * 3) * 37) % 251).astype(np.uint8).reshape(h, w, 3)


def _small_streams():
    """The streams the mutation sweep starts from: few blocks, so that a case is two short calls; interleaved 4:2:0 and 4:2:2 baseline
    scans and the progressive scan types with restart markers in them."""
    syn = _synthetic_jpegs()
    return {"tiny": syn["tiny"], "422_tiny": syn["422_tiny"],
            "prog_rst_16": _encode(_pattern(16, 16), progressive=True, subsampling=0, quality=90, restart_marker_blocks=2)}


def _crafted_streams():
    """name -> (stream, the call that must return ROMA_E_ARG): the malformed streams that wrote out of bounds before the host stage
    rejected them.  Each differs from a stream that decodes in the one respect its name gives."""
    base = _encode(_pattern(24, 40), subsampling=2, quality=85)
    prog = _encode(_pattern(32, 32), progressive=True, quality=85)
    out = {"dht_oversubscribed": (b"\xff\xd8\xff\xc4" + (2 + 17 + 255).to_bytes(2, "big") + bytes([0, 255] + [0] * 15) + bytes(range(255)), "info")}
    _, o, end = next(s for s in _segments(base) if s[0] == 0xC4)   # the first DHT segment, one value longer than its counts announce
    out["dht_counts_one_short"] = (base[:o + 2] + (end - o - 2 + 1).to_bytes(2, "big") + base[o + 4:end] + b"\0" + base[end:], "info")
    _, o, end = next(s for s in _segments(prog) if s[0] == 0xC2)
    sof = bytearray(prog[o:end])
    sof[5:9] = (1024).to_bytes(2, "big") * 2                      # height, width
    ac = next(s[1] for s in _segments(prog) if s[0] == 0xDA and prog[s[2] - 3] > 0)   # the first scan with Ss > 0
    out["second_sof"] = (prog[:ac] + bytes(sof) + prog[ac:], "entropy")
    _, o, end = next(s for s in _segments(base) if s[0] == 0xDA)
    for name, sel in (("dc_selector_7", 0x70), ("ac_selector_7", 0x07)):
        out[name] = (base[:o + 6] + bytes([sel]) + base[o + 7:], "info")   # FF DA, length, Ns, component id, selectors
    return out


def test_crafted_streams_are_rejected_inside_the_buffer():
    lib = _lib.load()
    streams = _crafted_streams()
    assert sorted(streams) == ["ac_selector_7", "dc_selector_7", "dht_counts_one_short", "dht_oversubscribed", "second_sof"]
    for name, (data, call) in streams.items():
        rc, info, _, _ = _host_decode(data, guard=GUARD)         # asserts the guard band itself
        assert rc == _lib.ROMA_E_ARG, (name, rc, lib.roma_last_error())
        assert (info is None) == (call == "info"), name          # the call that rejects it
    assert tuple(_host_decode(streams["second_sof"][0])[1][:2]) == (32, 32)


def test_mutated_streams_return_a_known_code_inside_the_buffer():
    """2 000 seeded cases per small stream, 1-3 bytes behind the first SOF segment overwritten with random values (the frame, and so the
    buffer sized from the intact stream, stays what it was): both host calls return 0, ROMA_E_ARG or ROMA_E_UNSUPPORTED, and the
    guard band behind the coefficient array comes back intact."""
    lib = _lib.load()
    for seed, (name, data) in enumerate(_small_streams().items()):
        rc, _, coef, _ = _host_decode(data)
        assert rc == 0, name
        nb, first = coef.shape[0], next(s[2] for s in _segments(data) if s[0] in (0xC0, 0xC1, 0xC2))
        rng = np.random.default_rng(seed)
        room, qt, info = np.empty((nb + GUARD, 64), np.int16), np.zeros((3, 64), np.uint16), np.zeros(8, np.int32)
        for case in range(2000):
            buf = np.frombuffer(data, dtype=np.uint8).copy()
            k = int(rng.integers(1, 4))
            buf[rng.integers(first, len(buf), size=k)] = rng.integers(0, 256, size=k)
            room[:] = SENTINEL
            rc_info = lib.roma_jpeg_info(buf.ctypes.data, len(buf), info.ctypes.data)
            rc_dec = lib.roma_jpeg_entropy_decode(buf.ctypes.data, len(buf), room.ctypes.data, qt.ctypes.data)
            assert rc_info in OK_CODES and rc_dec in OK_CODES, (name, case, rc_info, rc_dec)
            assert (room[nb:] == SENTINEL).all(), (name, case)


@pytest.mark.gpu
def test_device_reconstruction_is_bit_identical_to_pil():
    from roma_amd.preproc import decode_jpeg_device
    streams = {os.path.basename(f): open(f, "rb").read() for f in ASSETS}
    streams.update(_synthetic_jpegs())
    for name, data in streams.items():
        rgb = decode_jpeg_device(data, "cuda")
        assert rgb is not None and rgb.dtype == torch.uint8, name
        ref = torch.from_numpy(np.array(Image.open(io.BytesIO(data)).convert("RGB")))
        assert rgb.shape == ref.shape and torch.equal(rgb.cpu(), ref), name
    bio = io.BytesIO()
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).convert("CMYK").save(bio, "JPEG")
    assert decode_jpeg_device(bio.getvalue(), "cuda") is None  # the caller decodes such a stream with PIL
    assert torch.equal(decode_jpeg_device(ASSETS[1], "cuda").cpu(), torch.from_numpy(np.array(Image.open(ASSETS[1]).convert("RGB"))))   # a path


@pytest.mark.gpu
def test_match_on_jpeg_paths_feeds_the_same_bits_as_pil():
    """What match(path_A, path_B) feeds the network with the JPEGs decoded on the device — both resolutions, resized and normalised on
    the device — is BIT-identical to what it feeds with PIL decoding on the host; and match() runs on paths either way (two runs of
    the same inputs differ at the 1e-4 level through the library GEMMs' atomics, so outputs are compared with a tolerance; the e2e
    fixtures of test_gpu_model.py, generated from PIL-decoded inputs, go through the device decoder as well)."""
    from roma_amd.model_zoo import build_roma
    from roma_amd.preproc import decode_jpeg_device, preprocess_device
    for f in ASSETS[:2]:
        dev = decode_jpeg_device(f, "cuda")
        host = Image.open(f).convert("RGB")
        for size in ((112, 112), (560, 560), (864, 864)):
            assert torch.equal(preprocess_device(dev, size, "cuda"), preprocess_device(host, size, "cuda")), (f, size)
    torch.manual_seed(0)
    model = build_roma((112, 112), upsample_preds=True, amp_dtype=torch.float32)
    model.upsample_res = (168, 168)
    model = model.to("cuda").eval()
    assert model.device_jpeg
    w1, c1 = model.match(ASSETS[0], ASSETS[1], device="cuda")
    model.device_jpeg = False
    w2, c2 = model.match(ASSETS[0], ASSETS[1], device="cuda")
    assert torch.isfinite(w1).all() and torch.isfinite(c1).all()
    assert float((w1 - w2).abs().median()) < 1e-4 and float((c1 - c2).abs().median()) < 1e-4
