"""roma_amd.geometry.warp_kpts / get_gt_warp / dense_match_metrics / geometric_dist (csrc/depth_warp.hip) against the numpy fp64
restatement in tests/depth_warp_ref.py and against the reference's own outputs in tests/golden/depth_warp.npz (three pairs of the
23 x 37 -> 29 x 31 scene, recorded by tests/golden/make_golden_depth_warp.py).

Tolerances.  Device, restatement and reference run the same chain of about 30 fp64 operations from the same fp32 key-points and
depths, so they differ by fp64 rounding only (operation order, fused multiply-adds, the inverse of K_A): 1e-9 * max(1, |ref|) on x2 and
on the relative depth error is about five orders above that and five below 1e-4 px, the least a metric could see.  Masks and PCK
counts must be EQUAL at every point: the generator asserts that no decision of the fixture comes within 1e-6 of its threshold
(the closest are 6e-4 for the relative error, 2e-3 px for a border and for a PCK radius).  epe_sum: 1e-12 relative."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import depth_warp_ref as D
from tests.helpers import kernel_resources

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HA, WA, HB, WB = 23, 37, 29, 31
NS = (1, 257, 851)
THRESHOLD = 0.05
TOL = 1e-9
MODE_CODE = {"bilinear": 0, "nearest": 1, "combined": 2}


@functools.lru_cache(maxsize=None)
def fixture():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "depth_warp.npz")))
    assert g["kpts"].shape == (3, HA * WA, 2) and g["kpts"].dtype == np.float32 and g["depth_A"].dtype == np.float32
    assert g["depth_A"].shape == (3, HA, WA) and g["depth_B"].shape == (3, HB, WB) and g["T"].shape == (3, 3, 4)
    for v in g.values():
        v.setflags(write=False)
    return g


def pair_args(g, p):
    return g["depth_A"][p], g["depth_B"][p], g["T"][p], g["K_A"][p], g["K_B"][p]


@functools.lru_cache(maxsize=None)
def ref_warp(mode):
    """the restatement on the fixture's key-points, the three pairs stacked: valid (3,N), x2 (3,N,2), rel_err (3,N)"""
    g = fixture()
    outs = [D.warp_kpts(g["kpts"][p], *pair_args(g, p), mode, THRESHOLD) for p in range(3)]
    out = {k: np.stack([o[k] for o in outs]) for k in ("valid", "x2", "rel_err")}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_metrics(mode="bilinear"):
    g = fixture()
    outs = [D.geometric_dist(g["pred_warp"][p], *pair_args(g, p), mode, THRESHOLD) for p in range(3)]
    out = {k: np.stack([o[k] for o in outs]) for k in ("gd", "valid", "epe_sum", "counts")}
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_close(got, want, what):
    """got against want within TOL * max(1, |want|) where want is finite; inf and NaN in the same places"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) \
        and np.array_equal(np.isneginf(got), np.isneginf(want)), f"{what}: inf / NaN in other places"
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: largest deviation {worst:.2e} of {err.size} values (tolerance {TOL:.0e})")
    assert worst <= TOL, (what, worst)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_reproduces_the_reference_fixture():
    """Pins the yardstick: passes without the feature."""
    g = fixture()
    for mode in ("bilinear", "nearest"):
        r = ref_warp(mode)
        assert np.array_equal(r["valid"], g[f"valid_{mode}"]), mode
        assert 0.40 < r["valid"].mean() < 0.70
        assert_close(r["x2"], g[f"x2_{mode}"], f"{mode} x2")
        assert_close(r["rel_err"], g[f"rel_{mode}"], f"{mode} rel_err")
    comb, bil, near = ref_warp("combined"), ref_warp("bilinear"), ref_warp("nearest")
    assert np.array_equal(comb["valid"], bil["valid"] | near["valid"]) and (comb["valid"] & ~bil["valid"]).sum() > 100
    for p in range(3):
        x2, prob = D.get_gt_warp(*pair_args(g, p))
        assert np.array_equal(D.gt_grid(HA, WA).reshape(HA, WA, 2), g["pred_warp"][p, ..., :2])      # the restated linspace is torch's
        assert np.array_equal(prob, g["gt_prob"][p]) and prob.dtype == np.float32
        assert_close(x2, g["gt_x2"][p], f"get_gt_warp pair {p}")
    m = ref_metrics()
    assert np.array_equal(m["valid"], g["gd_prob"] == 1) and np.array_equal(m["counts"][:, 0], g["gd_pairs"])
    gd_ref = np.split(g["gd"], np.cumsum(g["gd_pairs"])[:-1])
    for p in range(3):
        assert_close(m["gd"][p][m["valid"][p]], gd_ref[p], f"gd pair {p}")
        assert np.array_equal(m["counts"][p, 1:], [(gd_ref[p] < r).sum() for r in (1.0, 3.0, 5.0)])
        assert abs(m["epe_sum"][p] - gd_ref[p].sum()) <= 1e-12 * gd_ref[p].sum()
    tot = m["counts"].sum(0)
    assert np.array_equal((tot[1:].astype(np.float32) / np.float32(tot[0])), g["pck"])
    assert abs(m["epe_sum"].sum() / tot[0] - g["gd"].mean()) <= 1e-12 * g["gd"].mean()


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "roma_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("roma_warp_kpts", 19), ("roma_dense_match_metrics", 23)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared in include/roma_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert lib.roma_abi_version() == 5 and _lib.ABI_VERSION == 5


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 32)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)

    def kpts(x=a, stride=2, da=a, db=a, T=a, Ka=a, Kb=a, P=1, N=4, dims=(8, 8, 8, 8), mode=0, thr=0.05, outs=(a, a, a)):
        return lib.roma_warp_kpts(x, stride, da, db, T, Ka, Kb, P, N, *dims, mode, thr, *outs, None)

    def metrics(w=a, pitch=32, da=a, db=a, T=a, Ka=a, Kb=a, P=1, H=4, W=8, dims=(8, 8, 8, 8), mode=0, thr=0.05, ws=a, nbytes=40, epe=a,
                counts=a, maps=(None, None)):
        return lib.roma_dense_match_metrics(w, pitch, da, db, T, Ka, Kb, P, H, W, *dims, mode, thr, ws, nbytes, epe, counts, *maps, None)

    for fn, name, ptrs in ((kpts, b"roma_warp_kpts", ("x", "da", "db", "T", "Ka", "Kb")),
                           (metrics, b"roma_dense_match_metrics", ("w", "da", "db", "T", "Ka", "Kb", "ws", "epe", "counts"))):
        for k in ptrs:
            assert fn(**{k: None}) == _lib.ROMA_E_ARG and name + b": null pointer" in lib.roma_last_error(), k
        for kw in ({"P": 0}, {"P": -1}, {"P": 65536}, {"dims": (0, 8, 8, 8)}, {"dims": (8, 8, 8, 40000)}):
            assert fn(**kw) == _lib.ROMA_E_SHAPE and name + b": bad shape" in lib.roma_last_error(), kw
        for mode in (-1, 3):
            assert fn(mode=mode) == _lib.ROMA_E_ARG and name + b": unknown mode" in lib.roma_last_error()
        assert fn(thr=float("nan")) == _lib.ROMA_E_ARG and name + b": threshold" in lib.roma_last_error()
    for N in (0, -3):
        assert kpts(N=N) == _lib.ROMA_E_SHAPE and b"roma_warp_kpts: bad shape N" in lib.roma_last_error()
    for stride in (0, 1, 3, 8):
        assert kpts(stride=stride) == _lib.ROMA_E_ARG and b"roma_warp_kpts: bad stride" in lib.roma_last_error()
    assert kpts(outs=(None, None, None)) == _lib.ROMA_E_ARG and b"roma_warp_kpts: every output is null" in lib.roma_last_error()
    assert kpts(x=odd) == _lib.ROMA_E_ALIGN and b"roma_warp_kpts" in lib.roma_last_error()
    for kw in ({"H": 0}, {"W": 0}, {"W": -2}):
        assert metrics(**kw) == _lib.ROMA_E_SHAPE and b"roma_dense_match_metrics: bad shape warp" in lib.roma_last_error()
    for pitch in (0, 28, 34, -32):                                    # below 4 W, or no multiple of 4
        assert metrics(pitch=pitch) == _lib.ROMA_E_ARG and b"roma_dense_match_metrics: bad stride" in lib.roma_last_error()
    assert metrics(nbytes=39) == _lib.ROMA_E_ARG and b"roma_dense_match_metrics: workspace" in lib.roma_last_error()
    assert metrics(H=33, W=32, pitch=128, nbytes=40) == _lib.ROMA_E_ARG and b"80 needed" in lib.roma_last_error()      # 1056 pixels: 2 partials
    assert metrics(w=odd) == _lib.ROMA_E_ALIGN and b"roma_dense_match_metrics" in lib.roma_last_error()


def test_workspace_helper_states_the_header_formula():
    from roma_amd import geometry
    assert geometry.dense_metrics_workspace(1, 4, 8) == 40 and geometry.dense_metrics_workspace(1, 32, 32) == 40
    assert geometry.dense_metrics_workspace(1, 33, 32) == 80 and geometry.dense_metrics_workspace(8, 384, 512) == 8 * 192 * 40
    assert "ceil(H * W / 1024) * 40" in open(os.path.join(ROOT, "include", "roma_hip.h")).read()


def test_wrappers_refuse_cpu_tensors_smooth_mask_and_unknown_modes():
    from roma_amd import geometry
    g = fixture()
    k, dA, dB, T, KA, KB, w = (torch.from_numpy(np.array(g[n])) for n in ("kpts", "depth_A", "depth_B", "T", "K_A", "K_B", "pred_warp"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.warp_kpts(k, dA, dB, T, KA, KB)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.get_gt_warp(dA, dB, T, KA, KB)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.dense_match_metrics(w, dA, dB, T, KA, KB)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.geometric_dist(dA, dB, T, KA, KB, w)
    for sm in (True, 0.1):
        with pytest.raises(NotImplementedError, match="smooth_mask"):
            geometry.warp_kpts(k, dA, dB, T, KA, KB, smooth_mask=sm)
    for fn in (lambda **kw: geometry.warp_kpts(k, dA, dB, T, KA, KB, **kw), lambda **kw: geometry.get_gt_warp(dA, dB, T, KA, KB, **kw),
               lambda **kw: geometry.dense_match_metrics(w, dA, dB, T, KA, KB, **kw)):
        with pytest.raises(ValueError, match="unknown depth_interpolation_mode 'nearest-exact'"):
            fn(depth_interpolation_mode="nearest-exact")
        with pytest.raises(ValueError, match="NaN"):
            fn(relative_depth_error_threshold=float("nan"))


def test_depth_warp_kernels_use_no_scratch_and_spill_nothing():
    """The compiler's resource report of csrc/depth_warp.hip (the recipe of test_triangulate.py); LDS holds the pair constants and,
    in the metrics kernel, one partial per wave."""
    kernels = kernel_resources("depth_warp.hip")
    assert sum("warp_kpts_kernel" in k for k in kernels) == 3 and sum("dense_metrics_kernel" in k for k in kernels) == 3, sorted(kernels)
    assert sum("dense_metrics_finish_kernel" in k for k in kernels) == 1 and len(kernels) == 7, sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] <= 512, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the cached fixtures are read-only


def _inputs(g=None, **replace):
    """the fixture's three pairs on the device: kpts, depth_A, depth_B, T, K_A, K_B"""
    g = fixture() if g is None else g
    return tuple(_dev(replace.get(k, g[k])) for k in ("kpts", "depth_A", "depth_B", "T", "K_A", "K_B"))


def _guarded(n, dtype):
    fill = {torch.float64: -7.5, torch.uint8: 171, torch.int64: -77}[dtype]
    return torch.full((n + GUARD,), fill, dtype=dtype, device=DEV), fill


def _collect(bufs, shapes):
    torch.cuda.synchronize()
    out = {}
    for name, (b, fill) in bufs.items():
        n = int(np.prod(shapes[name]))
        assert bool((b[n:] == fill).all()), f"{name}: the guard band was written"
        out[name] = b[:n].reshape(shapes[name]).clone()
    return out


def _raw_kpts(x, stride, dA, dB, T, KA, KB, mode, want=("x2", "valid", "rel_err"), threshold=THRESHOLD):
    """roma_warp_kpts itself, every requested output with a guard band behind its last element; the others NULL"""
    P, N = x.shape[:2]
    shapes = {"x2": (P, N, 2), "valid": (P, N), "rel_err": (P, N)}
    bufs = {k: _guarded(int(np.prod(shapes[k])), torch.uint8 if k == "valid" else torch.float64) for k in want}
    ptrs = [bufs[k][0].data_ptr() if k in bufs else None for k in ("x2", "valid", "rel_err")]
    _lib.check(_lib.load().roma_warp_kpts(x.data_ptr(), stride, dA.data_ptr(), dB.data_ptr(), T.data_ptr(), KA.data_ptr(), KB.data_ptr(), P, N,
                                          dA.shape[1], dA.shape[2], dB.shape[1], dB.shape[2], mode, threshold, *ptrs,
                                          torch.cuda.current_stream().cuda_stream), "roma_warp_kpts")
    return _collect(bufs, shapes)


def _raw_metrics(w, pitch, H, W, dA, dB, T, KA, KB, mode, want=("gd", "valid"), threshold=THRESHOLD):
    """roma_dense_match_metrics itself with guard bands; the workspace is exactly the header's formula plus a band, filled with NaN"""
    from roma_amd import geometry
    P = dA.shape[0]
    shapes = {"epe_sum": (P,), "counts": (P, 4), "gd": (P, H, W), "valid": (P, H, W)}
    dtypes = {"epe_sum": torch.float64, "counts": torch.int64, "gd": torch.float64, "valid": torch.uint8}
    bufs = {k: _guarded(int(np.prod(shapes[k])), dtypes[k]) for k in ("epe_sum", "counts") + tuple(want)}
    nbytes = geometry.dense_metrics_workspace(P, H, W)
    ws = torch.full((nbytes // 8 + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    ptrs = [bufs[k][0].data_ptr() if k in bufs else None for k in ("epe_sum", "counts", "gd", "valid")]
    _lib.check(_lib.load().roma_dense_match_metrics(w.data_ptr(), pitch, dA.data_ptr(), dB.data_ptr(), T.data_ptr(), KA.data_ptr(),
                                                    KB.data_ptr(), P, H, W, dA.shape[1], dA.shape[2], dB.shape[1], dB.shape[2], mode, threshold,
                                                    ws.data_ptr(), nbytes, *ptrs, torch.cuda.current_stream().cuda_stream),
               "roma_dense_match_metrics")
    out = _collect(bufs, shapes)
    assert bool(torch.isnan(ws[nbytes // 8:]).all()), "the band behind the workspace was written"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_warp_kpts_parity_with_the_restatement_and_the_reference(N):
    from roma_amd import geometry
    g = fixture()
    k, dA, dB, T, KA, KB = _inputs()
    k = k[:, :N].contiguous()
    T44 = torch.cat([T, torch.tensor([0.0, 0, 0, 1], dtype=torch.float64, device=DEV).expand(3, 1, 4)], 1)
    for mode in D.MODES:
        r = ref_warp(mode)
        valid, x2 = geometry.warp_kpts(k, dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        rel, x2b = geometry.warp_kpts(k.double(), dA.double(), dB, T44, KA, KB, return_relative_depth_error=True, depth_interpolation_mode=mode)
        assert valid.shape == (3, N) and valid.dtype == torch.bool and x2.shape == (3, N, 2) and x2.dtype == torch.float64
        assert rel.shape == (3, N) and rel.dtype == torch.float64 and torch.equal(x2, x2b)
        differ = int((valid.cpu().numpy() != r["valid"][:, :N]).sum())
        print(f"{mode} N={N}: {int(valid.sum())} valid of {3 * N}, masks differ at {differ} points")
        assert differ == 0
        assert_close(x2.cpu().numpy(), r["x2"][:, :N], f"{mode} N={N} x2 against the restatement")
        assert_close(rel.cpu().numpy(), r["rel_err"][:, :N], f"{mode} N={N} rel_err against the restatement")
        if mode != "combined":
            assert np.array_equal(valid.cpu().numpy(), g[f"valid_{mode}"][:, :N])
            assert_close(x2.cpu().numpy(), g[f"x2_{mode}"][:, :N], f"{mode} N={N} x2 against the reference")
            assert_close(rel.cpu().numpy(), g[f"rel_{mode}"][:, :N], f"{mode} N={N} rel_err against the reference")
    # the first two columns of a (P,N,4) warp, read in place
    w4 = torch.cat([k, torch.full_like(k, 9.0)], -1)
    v4, x4 = geometry.warp_kpts(w4[..., :2], dA, dB, T, KA, KB)
    v2, x2 = geometry.warp_kpts(k, dA, dB, T, KA, KB)
    assert torch.equal(v4, v2) and torch.equal(x4, x2)


@pytest.mark.gpu
def test_get_gt_warp_parity():
    from roma_amd import geometry
    g = fixture()
    _, dA, dB, T, KA, KB = _inputs()
    grid = geometry.gt_warp_grid(3, HA, WA, DEV)
    assert grid.shape == (3, HA * WA, 2) and grid.dtype == torch.float32 and grid.is_contiguous()
    gn, want = grid.cpu().numpy(), D.gt_grid(HA, WA)
    # one fp32 ulp of each value, and near the centre of the grid (values around 0, where an ulp of the value means nothing) one ulp
    # of the end point the element is computed from: its rounding, up to half of that, is in every element
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(want)).max())
    ulps = np.abs(gn.astype(np.float64) - want[None]) / ulp[None]
    print(f"the device's linspace is within {ulps.max():.2f} fp32 ulp of the CPU's")
    assert ulps.max() <= 1.0
    for mode in D.MODES:
        x2, prob = geometry.get_gt_warp(dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        assert x2.shape == (3, HA, WA, 2) and x2.dtype == torch.float64 and prob.shape == (3, HA, WA) and prob.dtype == torch.float32
        for p in range(3):
            rx2, rprob = D.get_gt_warp(*pair_args(g, p), mode, THRESHOLD, grid=gn[p])
            assert np.array_equal(prob[p].cpu().numpy(), rprob), (mode, p)
            assert_close(x2[p].cpu().numpy(), rx2, f"get_gt_warp {mode} pair {p}")
    # the reference's own grid through warp_kpts: its get_gt_warp
    valid, x2 = geometry.warp_kpts(_dev(np.broadcast_to(want, (3, HA * WA, 2))), dA, dB, T, KA, KB)
    assert np.array_equal(valid.cpu().numpy().reshape(3, HA, WA), g["gt_prob"] == 1)
    assert_close(x2.cpu().numpy().reshape(3, HA, WA, 2), g["gt_x2"], "get_gt_warp against the reference")
    # another grid size than the depth map's
    x2, prob = geometry.get_gt_warp(dA, dB, T, KA, KB, H=7, W=11)
    rx2, rprob = D.get_gt_warp(*pair_args(g, 1), H=7, W=11, grid=geometry.gt_warp_grid(1, 7, 11, DEV)[0].cpu().numpy())
    assert x2.shape == (3, 7, 11, 2) and np.array_equal(prob[1].cpu().numpy(), rprob)
    assert_close(x2[1].cpu().numpy(), rx2, "get_gt_warp on a 7 x 11 grid")


@pytest.mark.gpu
def test_dense_match_metrics_against_the_reference_and_the_restatement():
    from roma_amd import geometry
    g = fixture()
    _, dA, dB, T, KA, KB = _inputs()
    w = _dev(g["pred_warp"])
    gd_ref = np.split(g["gd"], np.cumsum(g["gd_pairs"])[:-1])
    for mode in D.MODES:
        r = ref_metrics(mode)
        m = geometry.dense_match_metrics(w, dA, dB, T, KA, KB, depth_interpolation_mode=mode, return_maps=True)
        counts = np.stack([v.cpu().numpy() for v in (m.n_valid, m.n_pck_1, m.n_pck_3, m.n_pck_5)], -1)
        epe_sum = m.epe_sum.cpu().numpy()
        print(f"{mode}: counts {counts.tolist()} against {r['counts'].tolist()}; epe_sum relative deviation "
              f"{np.abs(epe_sum / r['epe_sum'] - 1).max():.2e}; epe {float(m.epe):.6f} px")
        assert counts.dtype == np.int64 and np.array_equal(counts, r["counts"])
        assert np.abs(epe_sum - r["epe_sum"]).max() <= 1e-12 * r["epe_sum"].min()
        tot = r["counts"].sum(0)
        assert abs(float(m.epe) - r["epe_sum"].sum() / tot[0]) <= 1e-12 * float(m.epe)
        assert [float(m.pck_1), float(m.pck_3), float(m.pck_5)] == [tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0]]
        assert m.gd.shape == (3, HA, WA) and m.gd.dtype == torch.float64 and m.prob.dtype == torch.float32
        assert np.array_equal(m.prob.cpu().numpy() == 1, r["valid"])
        assert_close(m.gd.cpu().numpy(), r["gd"], f"{mode} gd map")
        # return_maps against warp_kpts plus torch arithmetic
        valid, x2 = geometry.warp_kpts(w[..., :2].reshape(3, -1, 2), dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        x2 = x2.reshape(3, HA, WA, 2)
        x2_px = torch.stack((WA * (x2[..., 0] + 1) / 2, HA * (x2[..., 1] + 1) / 2), -1)
        hat = torch.stack((WA * (w[..., 2] + 1) / 2, HA * (w[..., 3] + 1) / 2), -1)
        assert hat.dtype == torch.float32
        assert torch.equal(valid.reshape(3, HA, WA), m.prob == 1)
        assert_close(m.gd.cpu().numpy(), (hat - x2_px).norm(dim=-1).cpu().numpy(), f"{mode} gd map against warp_kpts + torch")
        assert abs(float(m.gd[m.prob == 1].sum()) - float(m.epe_sum.sum())) <= 1e-12 * float(m.epe_sum.sum())
        if mode == "bilinear":                                          # the reference's own numbers
            for p in range(3):
                assert np.array_equal(counts[p], [len(gd_ref[p])] + [(gd_ref[p] < k).sum() for k in (1.0, 3.0, 5.0)])
                assert abs(epe_sum[p] - gd_ref[p].sum()) <= 1e-12 * gd_ref[p].sum()
                assert_close(m.gd[p][m.prob[p] == 1].cpu().numpy(), gd_ref[p], f"gd of pair {p} against the reference")
            gd, pck_1, pck_3, pck_5, prob = geometry.geometric_dist(dA, dB, T, KA, KB, w)
            assert gd.dtype == torch.float64 and pck_1.dtype == torch.float32 and prob.dtype == torch.float32 and pck_1.dim() == 0
            assert_close(gd.cpu().numpy(), g["gd"], "geometric_dist gd against the reference")
            assert np.array_equal(np.array([pck_1.item(), pck_3.item(), pck_5.item()], np.float32), g["pck"])
            assert np.array_equal(prob.cpu().numpy(), g["gd_prob"])
        # without the maps: the same bits
        m2 = geometry.dense_match_metrics(w, dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        assert m2.gd is None and m2.prob is None and torch.equal(m2.epe_sum, m.epe_sum) and torch.equal(m2.n_pck_3, m.n_pck_3)


@pytest.mark.gpu
def test_dense_match_metrics_pitch_reproducibility_and_batch_independence():
    from roma_amd import geometry
    g = fixture()
    _, dA, dB, T, KA, KB = _inputs()
    w = _dev(g["pred_warp"])
    fields = ("epe_sum", "n_valid", "n_pck_1", "n_pck_3", "n_pck_5", "epe", "pck_1", "pck_3", "pck_5", "gd", "prob")

    def same(a, b):
        return all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields[:5] + fields[9:])

    base = geometry.dense_match_metrics(w, dA, dB, T, KA, KB, return_maps=True)
    again = geometry.dense_match_metrics(w, dA, dB, T, KA, KB, return_maps=True)
    assert same(base, again) and all(torch.equal(getattr(base, f), getattr(again, f)) for f in fields[5:9])
    # the left half of a symmetric (P,H,2W,4) buffer, through the pitch
    sym = torch.cat([w, torch.full_like(w, float("nan"))], 2)
    left = sym[:, :, :WA]
    assert not left.is_contiguous() and left.stride() == (HA * 8 * WA, 8 * WA, 4, 1) and left.data_ptr() == sym.data_ptr()
    assert same(base, geometry.dense_match_metrics(left, dA, dB, T, KA, KB, return_maps=True))
    # the raw call reads it in place: pitch 8 W, against pitch 4 W on the copy
    a = _raw_metrics(sym, 8 * WA, HA, WA, dA, dB, T, KA, KB, 0)
    b = _raw_metrics(w, 4 * WA, HA, WA, dA, dB, T, KA, KB, 0)
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(a["epe_sum"], base.epe_sum) and torch.equal(a["gd"], base.gd)
    # a strided view no pitch describes goes through a copy
    assert same(base, geometry.dense_match_metrics(w.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), dA, dB, T, KA, KB, return_maps=True))
    # a batch of 3 equals three batches of 1
    for p in range(3):
        one = geometry.dense_match_metrics(w[p:p + 1], dA[p:p + 1], dB[p:p + 1], T[p:p + 1], KA[p:p + 1], KB[p:p + 1], return_maps=True)
        assert all(torch.equal(getattr(base, f)[p:p + 1], getattr(one, f)) for f in fields[:5] + fields[9:]), p
    # more than one partial per pair (2 x 851 pixels) and a partial with a single pixel in its last wave
    tall = torch.cat([w, w.flip(1)], 1)
    m = geometry.dense_match_metrics(tall, dA, dB, T, KA, KB, return_maps=True)
    assert geometry.dense_metrics_workspace(3, 2 * HA, WA) == 3 * 2 * 40
    for p in range(3):
        r = D.geometric_dist(tall[p].cpu().numpy(), *pair_args(g, p))
        assert np.array_equal(np.array([int(v[p]) for v in (m.n_valid, m.n_pck_1, m.n_pck_3, m.n_pck_5)]), r["counts"])
        assert abs(float(m.epe_sum[p]) - r["epe_sum"]) <= 1e-12 * r["epe_sum"]


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_outputs_are_fully_written_guard_bands_untouched_and_independent(N):
    k, dA, dB, T, KA, KB = _inputs()
    k = k[:, :N].contiguous()
    for mode in (0, 1, 2):
        r = ref_warp(D.MODES[mode])
        every = _raw_kpts(k, 2, dA, dB, T, KA, KB, mode)
        assert np.array_equal(every["valid"].cpu().numpy(), r["valid"][:, :N].astype(np.uint8))          # 0 / 1, every element written
        assert not bool((every["x2"] == -7.5).any()) and not bool((every["rel_err"] == -7.5).any())
        for name in every:
            one = _raw_kpts(k, 2, dA, dB, T, KA, KB, mode, want=(name,))
            assert list(one) == [name] and torch.equal(one[name].view(torch.uint8), every[name].view(torch.uint8)), (mode, name)
        for p in range(3):
            alone = _raw_kpts(k[p:p + 1].clone(), 2, dA[p:p + 1].clone(), dB[p:p + 1].clone(), T[p:p + 1].clone(), KA[p:p + 1].clone(),
                              KB[p:p + 1].clone(), mode)
            assert all(torch.equal(alone[n][0].view(torch.uint8), every[n][p].view(torch.uint8)) for n in every), (mode, p)
    if N == NS[-1]:
        w = _dev(fixture()["pred_warp"])
        for mode in (0, 1, 2):
            every = _raw_metrics(w, 4 * WA, HA, WA, dA, dB, T, KA, KB, mode)
            r = ref_metrics(D.MODES[mode])
            assert np.array_equal(every["counts"].cpu().numpy(), r["counts"]) and int(every["valid"].max()) == 1
            assert not bool((every["gd"] == -7.5).any())
            for want in ((), ("gd",), ("valid",)):
                part = _raw_metrics(w, 4 * WA, HA, WA, dA, dB, T, KA, KB, mode, want=want)
                assert all(torch.equal(part[n].view(torch.uint8), every[n].view(torch.uint8)) for n in part), (mode, want)


@pytest.mark.gpu
def test_defined_behaviour_on_bad_input():
    """Key-points that are NaN, inf or 1e30, a depth of 1e30, a singular K_A, a pose that puts every point behind camera B: valid is
    0 there, nothing else changes, the counts ignore them, and the calls return success.  (The sampler's range checks precede any
    integer conversion: csrc/depth_warp.hip, sample_depth.)"""
    from roma_amd import geometry
    g = fixture()
    k, dA, dB, T, KA, KB = _inputs()
    rows = np.array([0, 5, 63, 64, 300, 600, 850])
    bad_k = g["kpts"].copy()
    bad_k[0, rows[0], 0], bad_k[0, rows[1], 1], bad_k[0, rows[2], 0], bad_k[0, rows[3], 1] = np.nan, np.inf, -np.inf, 1e30
    bad_k[0, rows[4]], bad_k[0, rows[5], 0], bad_k[0, rows[6]] = -1e30, 1e30, np.nan
    bad_dA = g["depth_A"].copy()
    bad_dA[0, 11, 20] = 1e30
    bad_KA = g["K_A"].copy()
    bad_KA[1, 1, 1] = 0.0                                                # pair 1: singular
    for mode in D.MODES:
        base_v, base_x = geometry.warp_kpts(k, dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        v, x = geometry.warp_kpts(_dev(bad_k), _dev(bad_dA), dB, T, _dev(bad_KA), KB, depth_interpolation_mode=mode)
        torch.cuda.synchronize()
        r0 = D.warp_kpts(bad_k[0], bad_dA[0], *pair_args(g, 0)[1:], mode, THRESHOLD)
        v, base_v = v.cpu().numpy(), base_v.cpu().numpy()
        touched = np.zeros(HA * WA, bool)
        touched[rows] = True
        # the key-points that sample the 1e30: those whose restated result changes with it
        clean = D.warp_kpts(bad_k[0], g["depth_A"][0], *pair_args(g, 0)[1:], mode, THRESHOLD)
        hit = ~touched & ~((clean["x2"] == r0["x2"]).all(-1))
        assert 1 <= hit.sum() <= 12
        assert not v[0][touched].any() and not v[0][hit].any()
        keep = ~touched & ~hit
        assert np.array_equal(v[0][keep], base_v[0][keep]) and torch.equal(x[0][_dev(keep)], base_x[0][_dev(keep)])
        assert np.array_equal(v[0], r0["valid"])
        assert not v[1].any()                                           # the singular K_A
        assert np.array_equal(v[2], base_v[2]) and torch.equal(x[2], base_x[2])
    # every point behind camera B: turn the camera round
    behind = g["T"].copy()
    behind[2] = np.array([[-1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, -1.0]])
    v, x = geometry.warp_kpts(k, dA, dB, _dev(behind), KA, KB)
    base_v, base_x = geometry.warp_kpts(k, dA, dB, T, KA, KB)
    assert not bool(v[2].any()) and torch.equal(v[:2], base_v[:2]) and torch.equal(x[:2], base_x[:2])
    # the metrics: bad pixels count nowhere, the other pairs keep their bits
    w = g["pred_warp"].copy()
    w[0].reshape(-1, 4)[rows, :2] = bad_k[0, rows]
    base = geometry.dense_match_metrics(_dev(g["pred_warp"]), dA, dB, T, KA, KB)
    m = geometry.dense_match_metrics(_dev(w), _dev(bad_dA), dB, _dev(behind), _dev(bad_KA), KB, return_maps=True)
    r0 = D.geometric_dist(w[0], bad_dA[0], *pair_args(g, 0)[1:])
    assert [int(c[0]) for c in (m.n_valid, m.n_pck_1, m.n_pck_3, m.n_pck_5)] == r0["counts"].tolist()
    assert abs(float(m.epe_sum[0]) - r0["epe_sum"]) <= 1e-12 * r0["epe_sum"] and int(m.n_valid[0]) < int(base.n_valid[0])
    assert not bool(m.prob[0].reshape(-1)[_dev(rows)].any())
    assert int(m.n_valid[1]) == 0 and int(m.n_valid[2]) == 0 and float(m.epe_sum[1]) == 0.0 and float(m.epe_sum[2]) == 0.0
    assert int(m.n_pck_5[1]) == 0 and not bool(m.prob[1:].any())
    assert float(m.epe) == float(m.epe_sum[0]) / int(m.n_valid[0])


@pytest.mark.gpu
def test_round_trip_of_the_ground_truth_warp():
    """get_gt_warp stored as an fp32 warp, then dense_match_metrics: every valid pixel within 1 px and the mean end-point error
    within the fp32 rounding of the stored coordinates, W * 2^-24 + H * 2^-24 px."""
    from roma_amd import geometry
    _, dA, dB, T, KA, KB = _inputs()
    for mode in D.MODES:
        x2, prob = geometry.get_gt_warp(dA, dB, T, KA, KB, depth_interpolation_mode=mode)
        warp = torch.cat([geometry.gt_warp_grid(3, HA, WA, DEV).reshape(3, HA, WA, 2), x2.float()], -1)
        m = geometry.dense_match_metrics(warp, dA, dB, T, KA, KB, depth_interpolation_mode=mode, return_maps=True)
        bound = (WA + HA) * 2.0 ** -24
        print(f"{mode}: {int(m.n_valid.sum())} valid pixels, epe {float(m.epe):.3e} px (bound {bound:.3e}), pck_1 {float(m.pck_1)}")
        assert torch.equal(m.prob, prob) and int(m.n_valid.sum()) == int(prob.sum()) > 1000
        assert float(m.pck_1) == 1.0 and torch.equal(m.n_pck_1, m.n_valid)
        assert float(m.epe) <= bound
