"""Shared plumbing for the parity tests: golden-fixture loading, recipe weights, reduced-model builders.

The builders take a namespace `ns` (the oracle module, or the product package) exposing ConvRefiner, GP, Block,
TransformerDecoder, Decoder with the constructor signatures of oracle/roma_oracle.py, so the same reduced model
can be instantiated on either side and loaded with the same recipe weights (reference state-dict key layout).
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import torch
import torch.nn as nn

from tests.golden import cases, recipes as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def T(a, device=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if device is None else t.to(device)


def load_recipe_weights(module: nn.Module, prefix: str, seed=0, gains=None, strict=True):
    sd = module.state_dict()
    new = {k: T(R.fill_tensor(prefix + k, v.shape, seed, gains)).to(v.dtype) for k, v in sd.items()}
    module.load_state_dict(new, strict=strict)
    return module


def build_refiner(ns, name):
    fd, ed, r, *_ = cases.REFINER_CASES[name]
    D = 2 * fd + ed + ((2 * r + 1) ** 2 if r else 0)
    return ns.ConvRefiner(D, D, 3, hidden_blocks=2, displacement_emb_dim=ed, local_corr_radius=r).eval()


def build_reduced_decoder(ns):
    RED = cases.RED
    dd = RED["gp"] + RED["feat16"]
    td = ns.TransformerDecoder(nn.Sequential(*[ns.Block(dd, RED["heads"]) for _ in range(RED["nblk"])]), dd, RED["cls_res"] ** 2 + 1)
    feat = dict(RED["feat"])
    feat[16] = RED["feat16"]
    refiners = nn.ModuleDict()
    for s in (16, 8, 4, 2, 1):
        r = RED["rad"][s]
        D = 2 * feat[s] + RED["emb"][s] + ((2 * r + 1) ** 2 if r else 0)
        refiners[str(s)] = ns.ConvRefiner(D, D, 3, hidden_blocks=2, displacement_emb_dim=RED["emb"][s], local_corr_radius=r)
    gps = nn.ModuleDict({"16": ns.GP(RED["gp"])})
    vgg = RED["vgg"]
    dims = {"16": (RED["dino"], feat[16]), "8": (vgg[8], feat[8]), "4": (vgg[4], feat[4]), "2": (vgg[2], feat[2]), "1": (vgg[1], feat[1])}
    proj = nn.ModuleDict({s: nn.Sequential(nn.Conv2d(i, o, 1, 1), nn.BatchNorm2d(o)) for s, (i, o) in dims.items()})
    return ns.Decoder(td, gps, proj, refiners).eval()


def full_model_weights(model_state_shapes, vit_state_shapes, seed=0):
    """Recipe weights of the shipped architecture, keyed like the reference's two state dicts."""
    w = R.fill_state_dict(model_state_shapes, seed, cases.E2E_GAINS)
    v = R.fill_state_dict({"dinov2." + k: s for k, s in vit_state_shapes.items()}, seed)
    return w, {k[len("dinov2."):]: a for k, a in v.items()}


def asset(name):
    return os.path.join(GOLDEN, "assets", name)


# ------------------------------------------------------------------------------------------ plumbing of the geometry tests
def dev(a, device="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def to_np(*tensors):
    return [t.cpu().numpy() for t in tensors]


@functools.lru_cache(maxsize=None)
def kernel_resources(hip_file, *extra_flags):
    """The compiler's resource report of roma_amd/csrc/<hip_file> for gfx950 (what tools/kres.sh wraps): {kernel: {field: int}}.
    Compiled once per (file, flags) and process; callers read the result and leave it as it is."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), f"{hipcc} is missing: the resource report needs the compiler"
    src = os.path.join(ROOT, "roma_amd", "csrc", hip_file)
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", *extra_flags], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def check_refine_entry_point_validates_arguments(entry, bind, least, null, misaligned):
    """The assertions the three test_refine_*_entry_point_validates_arguments_without_a_gpu share.  bind(lib, a) returns the test's own
    call(**kw) of the C entry point `entry`, every pointer defaulting to the 16-byte aligned host buffer a, with keywords for the
    pointers named in `null` and `misaligned` and for P, N, thr, iters.  The entry must refuse, by code and message: a null pointer in
    each argument of `null`, P = 0, N = least - 1, a threshold that is not positive, a negative iters, and a pointer that is not
    16-byte aligned in each argument of `misaligned`."""
    from roma_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 32)()
    call = bind(lib, ctypes.cast(buf, ctypes.c_void_p))
    for kw in null:
        assert call(**{kw: None}) == _lib.ROMA_E_ARG and (entry + ": null pointer").encode() in lib.roma_last_error()
    assert call(P=0) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    assert call(N=least - 1) == _lib.ROMA_E_SHAPE and f"need at least {least}".encode() in lib.roma_last_error()
    for thr in (0.0, -1.0, float("nan")):
        assert call(thr=thr) == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    assert call(iters=-1) == _lib.ROMA_E_ARG and b"iters" in lib.roma_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 8)
    for kw in misaligned:
        assert call(**{kw: odd}) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()
