"""roma_amd.geometry.triangulate_nview / depth_from_warps (csrc/triangulate_nview.hip) against the numpy restatement in
tests/triangulate_nview_ref.py, on the scenes of tests/multiview_scenes.py.  CPU tests pin the restatement (the robust view set is the
clean views, N views beat two, the refinement never raises the cost, V = 2 is the two-view midpoint, the world's origin does not
matter), the C-ABI argument checks and the kernel's resource report; GPU tests pin the kernel and the wrappers.

Parity tolerance, as in tests/test_triangulate.py.  Device and restatement run the same algorithm from the same fp32 observations and
the same fp64 view constants; the device computes per point in fp32 where the reference run of the restatement computes in fp64.  What
fp32 costs is measured by running the restatement itself in float32: per scene and mode, the largest deviation of its float32 run
from its float64 run over the compared points, times 4 for the kernel's other operation order and its fused multiply-adds.  Nothing
in it comes from the kernel.  Compared are the points the fp64 run fits with at least two views and a parallax of at least 2 degrees;
in robust mode without those that have an observed view whose error under the winning hypothesis lies within 1 % of the threshold
(there the choice of the views is a coin toss in any precision).  They are at least 95 % of the fitted points and include every point
without an outlier: both asserted on the CPU.  Deviations: |dX| / |X - c0| for points (c0 the mean camera centre), |dz| / |z| for the
depth, |dr| / max(r, 1 px) for reproj_error, |d cos| for cos_parallax.  `views` must be identical on the compared points but for at
most 0.5 % of them, which are then left out of the value comparison; the restatement's own float32 run differs on none."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import multiview_scenes as MS
from tests import triangulate_nview_ref as NR
from tests import triangulate_ref as T
from tests.helpers import dev, kernel_resources

DEV = "cuda:0"
FIELDS = ("points", "depth", "reproj", "cos_parallax")
OUTPUTS = FIELDS + ("views", "valid")
THR = 3.0                                                          # max_view_error of the robust runs, pixels
GATE_REPROJ = 2.0
MIN_PARALLAX_DEG = 2.0
COS_MIN_PARALLAX = math.cos(math.radians(MIN_PARALLAX_DEG))
INF = float("inf")


@functools.lru_cache(maxsize=None)
def scene(V, seed, N=1000, offset=False):
    return MS.multiview_scene(V, seed, N=N, offset=MS.WORLD_OFFSET if offset else None)


@functools.lru_cache(maxsize=None)
def ref(V, seed, N, robust, dtype="float64", iters=3, offset=False):
    s = scene(V, seed, N, offset)
    return NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], max_view_error=THR if robust else INF, iters=iters, dtype=getattr(np, dtype))


def compared(r, robust):
    sel = r["finite"] & (r["cos_parallax"] <= COS_MIN_PARALLAX)
    if robust:
        with np.errstate(all="ignore"):
            sel = sel & ~(r["observed"] & (np.abs(r["hyp_error"] - THR) <= 0.01 * THR)).any(0)
    return sel


def deviations(o, r, sel):
    """the four deviation measures of the module docstring of outputs o against the fp64 run r, largest over the points sel"""
    if not sel.any():
        return {k: 0.0 for k in FIELDS}
    scale = np.linalg.norm(r["points"] - r["c0"], axis=-1)
    with np.errstate(all="ignore"):
        d = {"points": np.linalg.norm(o["points"].astype(np.float64) - r["points"], axis=-1) / scale,
             "depth": np.abs(o["depth"] - r["depth"]) / np.abs(r["depth"]),
             "reproj": np.abs(o["reproj"] - r["reproj"]) / np.maximum(r["reproj"], 1.0),
             "cos_parallax": np.abs(o["cos_parallax"] - r["cos_parallax"])}
    return {k: float(v[sel].max()) for k, v in d.items()}


def tolerance(r64, r32, sel):
    return {k: 4.0 * v for k, v in deviations(r32, r64, sel & (r32["views"] == r64["views"])).items()}


def relative_error(points, s, c0):
    return np.linalg.norm(points - s["X"], axis=-1) / np.linalg.norm(s["X"] - c0, axis=-1)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_robust_view_set_is_the_clean_views_and_leaves_clean_points_whole():
    for offset in (False, True):
        for seed in range(3):
            s, r = scene(5, seed, 2000, offset), ref(5, seed, 2000, True, offset=offset)
            seen, out = s["seen"], s["outlier"]
            assert np.array_equal(r["observed"], seen)
            clean_pt = ~out.any(0)
            n_clean = (seen & ~out).sum(0)
            contaminated = out.any(0) & (n_clean >= 3)
            whole = (r["member"] == seen)[:, clean_pt].all(0)
            exact = (r["member"] == (seen & ~out))[:, contaminated].all(0)
            err = relative_error(r["points"], s, r["c0"])
            fit = r["finite"] & clean_pt
            with np.errstate(all="ignore"):
                near = (seen & (np.abs(r["hyp_error"] - THR) <= 0.01 * THR)).any(0)
            print(f"scene {seed} offset {offset}: {seen.sum(0).mean():.2f} views observe a point, {clean_pt.mean():.3f} without an outlier, "
                  f"{contaminated.mean():.3f} contaminated with >= 3 clean views; median relative point error {np.median(err[fit]):.4f}; "
                  f"{int(near.sum())} points with an error within 1 % of the threshold")
            assert 3.9 < seen.sum(0).mean() < 4.5 and 0.65 < clean_pt.mean() < 0.78 and 0.2 < contaminated.mean() < 0.3
            assert whole.all() and exact.all()
            assert 0.0005 < np.median(err[fit]) < 0.0045           # two views at baseline 1: 0.0045 (tests/test_triangulate.py)
            assert np.array_equal(r["num_views"], r["member"].sum(0))
            assert np.array_equal(r["views"], sum(r["member"][v].astype(np.uint32) << np.uint32(v) for v in range(5)))


def test_n_views_beat_two_views_on_clean_points():
    for seed in range(3):
        s, r = scene(5, seed, 2000), ref(5, seed, 2000, True)
        both = s["seen"][0] & s["seen"][1] & ~s["outlier"].any(0) & r["finite"] & (r["num_views"] >= 3)
        m = np.concatenate([s["x"][0], s["x"][1]], -1)[both]
        two = T.triangulate(m, s["K"][0], s["K"][1], s["R"][1], s["t"][1], "optimal")
        assert two["valid"].all()
        e_two = np.linalg.norm(two["points"] - s["X"][both], axis=-1) / np.linalg.norm(s["X"][both] - r["c0"], axis=-1)
        e_n = relative_error(r["points"], s, r["c0"])[both]
        print(f"scene {seed}: {int(both.sum())} clean points seen by views 0, 1 and more: median relative point error {np.median(e_n):.5f} "
              f"from all views, {np.median(e_two):.5f} from views 0 and 1")
        assert both.sum() > 500 and np.median(e_n) < np.median(e_two)


def test_refinement_never_raises_the_cost_and_three_steps_are_enough():
    for robust in (False, True):
        for seed in range(3):
            r0, r3, r10 = ref(5, seed, 2000, robust, iters=0), ref(5, seed, 2000, robust), ref(5, seed, 2000, robust, iters=10)
            fit = r3["finite"]
            assert np.array_equal(r0["views"], r3["views"]) and np.array_equal(r0["cost"], r0["cost0"])
            assert np.array_equal(r3["cost0"][fit], r0["cost"][fit])
            assert (r3["cost"][fit] <= r3["cost0"][fit]).all() and (r10["cost"][fit] <= r3["cost"][fit] * (1 + 1e-12)).all()
            if robust:
                d = np.linalg.norm(r10["points"] - r3["points"], axis=-1) / np.linalg.norm(r3["points"] - r3["c0"], axis=-1)
                print(f"scene {seed}: 3 steps against 10: {d[fit].max():.2e} relative in the point")
                assert d[fit].max() < 4e-5


def test_two_views_without_refinement_are_the_two_view_midpoint():
    for seed in range(3):
        s = scene(2, seed, 2000)
        r = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], iters=0)
        mid = T.triangulate(np.concatenate([s["x"][0], s["x"][1]], -1).astype(np.float64), s["K"][0], s["K"][1], s["R"][1], s["t"][1], "midpoint")
        both = r["finite"] & mid["finite"]
        assert both.sum() > 1000 and np.array_equal(r["finite"], s["seen"].all(0))
        # in units of max(1, |X|): a match with an outlier puts its midpoint hundreds of baselines away at a fraction of a degree
        d = (np.abs(r["points"] - mid["points"]).max(-1) / np.maximum(1.0, np.linalg.norm(mid["points"], axis=-1)))[both].max()
        print(f"scene {seed}: V = 2, iters = 0 against triangulate_ref midpoint: {d:.2e}")
        assert d < 1e-9
        assert (np.abs(r["depth"] - mid["depth_a"]) / np.maximum(1.0, np.abs(mid["depth_a"])))[both].max() < 1e-9
        # reproj is the root of the MEAN here, of the SUM there
        assert np.abs(r["reproj"] * math.sqrt(2.0) - mid["reproj"])[both & (mid["reproj"] < 1e3)].max() < 1e-6


def test_world_offset_changes_nothing():
    """The same scene 2.3e4 away from the origin.  The linear start and one step are continuous in their inputs, and the shifted run
    lands within 1e-9 of the depth range (12) of the plain one.  From the second or third step on the accept rule decides: near the
    minimum a step's true gain, 0.5 d^T H d, sinks below the rounding of the cost (2^-53 of about 1 px^2), so whether it is kept is a
    coin toss and the point wanders by sqrt(2^-52 / H) — measured 2e-8 to 4e-8 on the points with the weakest geometry, 3e-9 of the depth
    range, in the plain scene no less than in the shifted one.  For iters = 3 and 10 the bound is therefore 1e-9 of the size of the
    shifted scene's coordinates, |offset| = 2.3e4, with identical view sets and valid flags; the figures are printed."""
    extent = float(np.linalg.norm(MS.WORLD_OFFSET))
    for robust in (False, True):
        for seed in range(3):
            s, so = scene(5, seed, 2000), scene(5, seed, 2000, True)
            # without the robust choice a point with an outlier among its views is a least-squares fit to a gross error: where it lands
            # is ill-conditioned in any arithmetic, so there the points without an outlier are the ones compared
            for iters, bound in ((0, 1e-9 * 12.0), (1, 1e-9 * 12.0), (3, 1e-9 * extent), (10, 1e-9 * extent)):
                r = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], max_view_error=THR if robust else INF, iters=iters)
                ro = NR.triangulate_nview(so["x"], so["K"], so["R"], so["t"], max_view_error=THR if robust else INF, iters=iters)
                assert np.array_equal(r["views"], ro["views"]) and np.array_equal(r["valid"], ro["valid"])
                fit = r["finite"] & (r["cos_parallax"] <= COS_MIN_PARALLAX) & (robust | ~s["outlier"].any(0))
                d = np.abs(ro["points"] - MS.WORLD_OFFSET - r["points"])[fit].max()
                print(f"scene {seed} robust {robust} iters {iters}: offset run - plain run {d:.2e} (bound {bound:.1e})")
                assert d < bound
            # and in float32: the offset does not reach the per-point arithmetic
            r, r32, ro32 = ref(5, seed, 2000, robust), ref(5, seed, 2000, robust, "float32"), ref(5, seed, 2000, robust, "float32", offset=True)
            assert np.array_equal(r32["views"], ro32["views"])
            fit32 = r["finite"] & (r["cos_parallax"] <= COS_MIN_PARALLAX) & (robust | ~s["outlier"].any(0)) & r32["finite"]
            scale = np.linalg.norm(r["points"] - r["c0"], axis=-1)
            d32 = (np.linalg.norm(ro32["points"].astype(np.float64) - MS.WORLD_OFFSET - r32["points"], axis=-1) / scale)[fit32].max()
            print(f"    float32: {d32:.2e} relative (the shifted points are rounded to fp32 at 2e4: 2^-24 * 2e4 / 4 = 3e-4)")
            assert d32 < 1e-3


@pytest.mark.parametrize("V", [3, 5])
@pytest.mark.parametrize("robust", [False, True])
def test_float32_run_of_the_restatement_and_the_shares_of_compared_points(V, robust):
    """What the GPU parity test relies on, checked here without a device."""
    for seed in range(3):
        s, r64, r32 = scene(V, seed), ref(V, seed, 1000, robust), ref(V, seed, 1000, robust, "float32")
        assert r32["points"].dtype == np.float32 and r32["reproj"].dtype == np.float32
        sel = compared(r64, robust)
        clean_pt = ~s["outlier"].any(0) & r64["finite"]
        d = deviations(r32, r64, sel)
        print(f"V {V} robust {robust} scene {seed}: fitted {r64['finite'].mean():.3f}, compared {sel.sum() / r64['finite'].sum():.3f} of them; "
              f"fp32 - fp64: {d}")
        assert sel.sum() >= 0.95 * r64["finite"].sum() and sel[clean_pt].all()
        assert np.array_equal(r32["views"][sel], r64["views"][sel])
        assert not any(np.isnan(r32[k]).any() for k in FIELDS)
        if robust:
            assert d["points"] < 1e-3 and d["depth"] < 1e-3 and d["reproj"] < 1e-2 and d["cos_parallax"] < 1e-5


def _host_call(lib, a, V=3, **kw):
    """roma_triangulate_nview on host pointers: only good for the argument checks, which run before anything touches a device"""
    tab = (ctypes.c_void_p * 32)(*([a.value] * 32))
    arg = dict(obs=ctypes.cast(tab, ctypes.c_void_p), to_px=None, visible=None, vis_stride=0, K=a, R=a, t=a, V=V, rows=1, row_len=4, row_stride=0,
               point_stride=2, mve=INF, iters=3, min_views=2, ref_view=0, max_reproj=INF, max_cos=1.0, outs=(a,) * 6)
    arg.update(kw)
    return lib.roma_triangulate_nview(arg["obs"], arg["to_px"], arg["visible"], arg["vis_stride"], arg["K"], arg["R"], arg["t"], arg["V"], arg["rows"],
                                      arg["row_len"], arg["row_stride"], arg["point_stride"], arg["mve"], arg["iters"], arg["min_views"],
                                      arg["ref_view"], arg["max_reproj"], arg["max_cos"], *arg["outs"], None)


def test_entry_point_validates_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    call = functools.partial(_host_call, lib, a)
    for kw in ({"obs": None}, {"K": None}, {"R": None}, {"t": None}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"roma_triangulate_nview: null pointer" in lib.roma_last_error()
    holed = (ctypes.c_void_p * 32)(a.value, None, a.value)
    assert call(obs=ctypes.cast(holed, ctypes.c_void_p)) == _lib.ROMA_E_ARG and b"null pointer (observations of view 1)" in lib.roma_last_error()
    assert call(outs=(None,) * 6) == _lib.ROMA_E_ARG and b"every output is null" in lib.roma_last_error()
    for kw in ({"V": 1}, {"V": 33}, {"V": 0}, {"rows": 0}, {"row_len": 0}, {"rows": 65536}, {"row_len": -3}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error(), kw
    for kw in ({"row_stride": 3}, {"row_stride": -2}, {"point_stride": 3}, {"point_stride": -2}, {"point_stride": 0},
               {"visible": ctypes.cast(holed, ctypes.c_void_p), "vis_stride": -1}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"bad strides" in lib.roma_last_error(), kw
    for kw in ({"iters": -1}, {"iters": 11}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"iters" in lib.roma_last_error()
    for kw in ({"min_views": 1}, {"min_views": 4}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"min_views" in lib.roma_last_error()
    for kw in ({"ref_view": -1}, {"ref_view": 3}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"ref_view" in lib.roma_last_error()
    for kw in ({"mve": float("nan")}, {"max_reproj": float("nan")}, {"max_cos": float("nan")}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"NaN" in lib.roma_last_error()
    for kw in ({"mve": 0.0}, {"mve": -1.0}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"max_view_error must be positive" in lib.roma_last_error()
    odd = (ctypes.c_void_p * 32)(a.value, a.value + 4, a.value)
    assert call(obs=ctypes.cast(odd, ctypes.c_void_p)) == _lib.ROMA_E_ALIGN and b"8-byte aligned" in lib.roma_last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from roma_amd import geometry
    x = torch.rand(3, 50, 2) * 500
    K = torch.eye(3, dtype=torch.float64)
    R, t = torch.eye(3, dtype=torch.float64).expand(3, 3, 3), torch.zeros(3, 3, dtype=torch.float64)
    warps, certs = [torch.rand(8, 16, 4) for _ in range(2)], [torch.rand(8, 16) for _ in range(2)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.triangulate_nview(x, R, t, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.depth_from_warps(warps, certs, R[:2], t[:2], K, K, 480, 640)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.depth_from_warps(torch.stack(warps), torch.stack(certs), R[:2], t[:2], K, K, 480, 640)
    # bad arguments are refused before anything looks at a tensor: the CPU tensors are not reached
    for fn in (lambda **kw: geometry.triangulate_nview(x, R, t, K, **kw),
               lambda **kw: geometry.depth_from_warps(warps, certs, R[:2], t[:2], K, K, 480, 640, **kw)):
        for kw, what in (({"max_view_error": 0.0}, "max_view_error"), ({"max_view_error": -1.0}, "max_view_error"), ({"iters": 11}, "iters"),
                         ({"iters": -1}, "iters"), ({"min_views": 1}, "min_views"), ({"min_views": 40}, "min_views"),
                         ({"max_reproj_error": -2.0}, "max_reproj_error"), ({"min_parallax_deg": -1.0}, "min_parallax_deg")):
            with pytest.raises(ValueError, match=what):
                fn(**kw)
    with pytest.raises(ValueError, match="ref_view"):
        geometry.triangulate_nview(x, R, t, K, ref_view=-1)


def test_kernel_uses_no_scratch_and_spills_nothing():
    """The compiler's resource report of csrc/triangulate_nview.hip; static LDS holds the view constants, the slab is dynamic."""
    kernels = kernel_resources("triangulate_nview.hip")
    assert sum("triangulate_nview_kernel" in k for k in kernels) == 1, sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] <= 5 * 1024, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _fields(tri):
    """a MultiViewTriangulation -> the restatement's dict of numpy arrays"""
    return {"points": tri.points.cpu().numpy(), "depth": tri.depth.cpu().numpy(), "reproj": tri.reproj_error.cpu().numpy(),
            "cos_parallax": tri.cos_parallax.cpu().numpy(), "views": tri.views.cpu().numpy().view(np.uint32), "valid": tri.valid.cpu().numpy(),
            "num_views": tri.num_views.cpu().numpy()}


def _run(s, robust, x=None, **kw):
    from roma_amd import geometry
    return geometry.triangulate_nview(dev(s["x"] if x is None else x), dev(s["R"]), dev(s["t"]), dev(s["K"]),
                                      max_view_error=THR if robust else None, **kw)


GUARD = 64
_FILL = {"views": 0x5A5A5A5A, "valid": 171}
_DTYPE = {"views": torch.int32, "valid": torch.uint8}


def _raw(obs, K, R, t, rows, row_len, row_stride, point_stride, want=OUTPUTS, to_px=None, vis=None, vis_stride=0, mve=INF, iters=3, min_views=2,
         ref_view=0, max_reproj=INF, max_cos=1.0):
    """roma_triangulate_nview itself: obs a list of V device addresses, vis None or a list of addresses / None; each requested output
    allocated with a guard band behind its N elements (asserted untouched), the others passed as NULL.  Returns {name: tensor}."""
    V, N = len(obs), rows * row_len
    bufs, ptrs = {}, []
    for name in OUTPUTS:
        if name not in want:
            ptrs.append(None)
            continue
        k = 3 if name == "points" else 1
        bufs[name] = torch.full((N * k + GUARD,), _FILL.get(name, -7.5), dtype=_DTYPE.get(name, torch.float32), device=DEV)
        ptrs.append(bufs[name].data_ptr())
    obs_tab = (ctypes.c_void_p * V)(*obs)
    vis_tab = None if vis is None else (ctypes.c_void_p * V)(*vis)
    px_tab = None if to_px is None else (ctypes.c_float * (4 * V))(*[float(v) for row in to_px for v in row])
    rc = _lib.load().roma_triangulate_nview(ctypes.cast(obs_tab, ctypes.c_void_p), None if px_tab is None else ctypes.cast(px_tab, ctypes.c_void_p),
                                            None if vis_tab is None else ctypes.cast(vis_tab, ctypes.c_void_p), vis_stride, K.data_ptr(),
                                            R.data_ptr(), t.data_ptr(), V, rows, row_len, row_stride, point_stride, mve, iters, min_views,
                                            ref_view, max_reproj, max_cos, *ptrs, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "roma_triangulate_nview")
    torch.cuda.synchronize()
    out = {}
    for name, b in bufs.items():
        k = 3 if name == "points" else 1
        assert bool((b[N * k:] == _FILL.get(name, -7.5)).all()), f"{name}: the guard band was written"
        out[name] = b[:N * k].reshape((N, 3) if name == "points" else (N,)).clone()
    return out


def _raw_packed(x, K, R, t, **kw):
    """x (V,N,2) float32 contiguous on the device"""
    V, N = x.shape[0], x.shape[1]
    return _raw([x.data_ptr() + 8 * N * v for v in range(V)], K, R, t, 1, N, 0, 2, **kw)


def _np(out):
    o = {k: v.cpu().numpy() for k, v in out.items()}
    if "views" in o:
        o["views"] = o["views"].view(np.uint32)
    if "valid" in o:
        o["valid"] = o["valid"].astype(bool)
    return o


def _assert_parity(o, r64, r32, robust, what, gates=None, clean=None):
    """The value comparison of the module docstring over the compared points, and once more over those of them in `clean` (the
    points without an outlier) with the tolerance that the same rule gives for them: without the robust choice one point fitted to a
    gross outlier can cost fp32 everything and so widen the first tolerance until it says little.  gates = (max_reproj, max_cos) of
    the call: then `valid` is compared too, on the clean compared points, wherever no gated quantity is within the tolerance of its
    gate."""
    assert all(np.isfinite(o[k]).all() for k in FIELDS), what
    sel = compared(r64, robust)
    same = o["views"] == r64["views"]
    print(f"{what}: views differ on {int((sel & ~same).sum())} of {int(sel.sum())} compared points")
    assert (sel & ~same).sum() <= 0.005 * sel.sum(), what
    for name, sub in (("compared", sel),) + ((("compared, no outlier", sel & clean),) if clean is not None else ()):
        tol = tolerance(r64, r32, sub)
        d = deviations(o, r64, sub & same)
        print(f"{what}, {int(sub.sum())} {name}: device - fp64 restatement {d}; tolerance {tol}")
        for k in FIELDS:
            assert d[k] <= tol[k], (what, name, k, d[k], tol[k])
    if gates is not None:
        max_reproj, max_cos = gates
        want = r64["valid"] & (r64["reproj"] <= max_reproj) & (r64["cos_parallax"] <= max_cos)
        scale = np.linalg.norm(r64["points"] - r64["c0"], axis=-1)
        with np.errstate(all="ignore"):
            near = (np.abs(r64["reproj"] - max_reproj) <= tol["reproj"] * np.maximum(r64["reproj"], 1.0)) \
                | (np.abs(r64["cos_parallax"] - max_cos) <= tol["cos_parallax"]) | (np.abs(r64["minz"]) <= tol["depth"] * scale)
        differ = (o["valid"] != want) & sub & same
        print(f"{what}: valid {int(o['valid'][sub].sum())} / {int(want[sub].sum())}, {int(differ.sum())} differ, {int((near & sub).sum())} within the "
              "tolerance of a gate")
        assert (near & sub).sum() <= 0.005 * sub.sum() and not (differ & ~near).any(), what


@pytest.mark.gpu
@pytest.mark.parametrize("V", [3, 5])
@pytest.mark.parametrize("robust", [False, True])
def test_parity_with_the_restatement(V, robust):
    for seed in range(3):
        s, r64, r32 = scene(V, seed), ref(V, seed, 1000, robust), ref(V, seed, 1000, robust, "float32")
        tri = _run(s, robust, max_reproj_error=GATE_REPROJ, min_parallax_deg=MIN_PARALLAX_DEG)
        assert tri.points.shape == (1000, 3) and tri.points.dtype == torch.float32 and tri.valid.dtype == torch.bool
        assert tri.views.dtype == torch.int32 and tri.num_views.dtype == torch.uint8 and tri.depth.shape == (1000,)
        o = _fields(tri)
        assert np.array_equal(o["num_views"], sum((o["views"] >> np.uint32(v)) & 1 for v in range(V)))
        clean_pt = ~s["outlier"].any(0) & r64["finite"]
        _assert_parity(o, r64, r32, robust, f"V {V} robust {robust} scene {seed}", (GATE_REPROJ, COS_MIN_PARALLAX), clean_pt)
        assert o["valid"][clean_pt].mean() > 0.9


def _device_scene(V, seed, N):
    s = scene(V, seed)
    return dev(np.ascontiguousarray(s["x"][:, :N])), dev(s["K"]), dev(s["R"]), dev(s["t"])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_shapes_null_outputs_and_guard_bands(N):
    x, K, R, t = _device_scene(3, 1, N)
    for mve in (INF, THR):
        kw = dict(mve=mve, max_reproj=GATE_REPROJ, max_cos=COS_MIN_PARALLAX)
        every = _raw_packed(x, K, R, t, **kw)
        assert all(torch.isfinite(every[k]).all() for k in FIELDS) and int(every["valid"].max()) <= 1
        if N >= 63:
            assert int(every["valid"].sum()) > 0
        # each output alone, and the subset whose values depth_from_warps reads, the others NULL
        for want in [(k,) for k in OUTPUTS] + [("points", "depth", "reproj", "views", "valid")]:
            part = _raw_packed(x, K, R, t, want=want, **kw)
            assert tuple(part) == want and all(torch.equal(part[k], every[k]) for k in want), (mve, want)
        # the first N points of the N = 1000 call
        if N < 1000:
            bx = _device_scene(3, 1, 1000)[0]
            big = _raw_packed(bx, K, R, t, **kw)
            assert all(torch.equal(big[k][:N], every[k]) for k in every), mve


@pytest.mark.gpu
@pytest.mark.parametrize("V", [2, 32])
def test_fewest_and_most_views(V):
    """V = 32 is where the slab of observations takes 64 KiB of dynamic LDS"""
    s = MS.multiview_scene(V, 4, N=65)
    x, K, R, t = dev(s["x"]), dev(s["K"]), dev(s["R"]), dev(s["t"])
    for robust in (False, True):
        mve = THR if robust else INF
        o = _np(_raw_packed(x, K, R, t, mve=mve))
        r64 = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], max_view_error=mve)
        r32 = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], max_view_error=mve, dtype=np.float32)
        assert compared(r64, robust).sum() >= 40
        _assert_parity(o, r64, r32, robust, f"V {V} robust {robust}", clean=~s["outlier"].any(0))
        if V == 32 and robust:
            assert int(max(bin(int(v)).count("1") for v in o["views"])) >= 8


@pytest.mark.gpu
def test_strided_observations_equal_the_packed_copy():
    """the warp layout: rows of row_len points inside wider rows, points 4 floats apart, the observation in the upper half of each"""
    Hh, Ww, V = 5, 13, 3
    s = scene(V, 2)
    xs = s["x"][:, :Hh * Ww].reshape(V, Hh, Ww, 2)
    K, R, t = dev(s["K"]), dev(s["R"]), dev(s["t"])
    rng = np.random.default_rng(3)
    wide = rng.normal(0, 500, (V, Hh, 2 * Ww, 4)).astype(np.float32)
    wide[:, :, :Ww, 2:] = xs
    vis = rng.random((V, Hh, 2 * Ww)) < 0.8
    dwide, dvis = dev(wide), dev(vis.astype(np.uint8))
    packed, pvis = dev(np.ascontiguousarray(xs.reshape(V, -1, 2))), dev(np.ascontiguousarray(vis[:, :, :Ww].reshape(V, -1).astype(np.uint8)))
    N = Hh * Ww
    for mve in (INF, THR):
        a = _raw([dwide[v].data_ptr() + 8 for v in range(V)], K, R, t, Hh, Ww, 8 * Ww, 4, mve=mve, vis=[dvis[v].data_ptr() for v in range(V)],
                 vis_stride=2 * Ww)
        b = _raw([packed[v].data_ptr() for v in range(V)], K, R, t, 1, N, 0, 2, mve=mve, vis=[pvis[v].data_ptr() for v in range(V)], vis_stride=N)
        assert all(torch.equal(a[k], b[k]) for k in OUTPUTS), mve
        assert int(a["valid"].sum()) > N // 3
        # a null entry of the visibility table: that view is always visible
        c = _raw([packed[v].data_ptr() for v in range(V)], K, R, t, 1, N, 0, 2, mve=mve, vis=[None] + [pvis[v].data_ptr() for v in (1, 2)],
                 vis_stride=N)
        pv2 = pvis.clone()
        pv2[0] = 1
        d = _raw([packed[v].data_ptr() for v in range(V)], K, R, t, 1, N, 0, 2, mve=mve, vis=[pv2[v].data_ptr() for v in range(V)], vis_stride=N)
        assert all(torch.equal(c[k], d[k]) for k in OUTPUTS), mve


@pytest.mark.gpu
def test_two_views_against_the_device_two_view_midpoint():
    from roma_amd import geometry
    for seed in range(3):
        s = scene(2, seed)
        tri = _fields(_run(s, False, iters=0))
        two = geometry.triangulate(dev(s["x"][0]), dev(s["x"][1]), dev(s["R"][1]), dev(s["t"][1]), dev(s["K"][0]), dev(s["K"][1]), method="midpoint")
        r64 = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], iters=0)
        r32 = NR.triangulate_nview(s["x"], s["K"], s["R"], s["t"], iters=0, dtype=np.float32)
        m = np.concatenate([s["x"][0], s["x"][1]], -1)
        t64, t32 = T.triangulate(m, s["K"][0], s["K"][1], s["R"][1], s["t"][1], "midpoint"), \
            T.triangulate(m, s["K"][0], s["K"][1], s["R"][1], s["t"][1], "midpoint", dtype=np.float32)
        sel = compared(r64, False) & t64["finite"]
        scale = np.linalg.norm(r64["points"] - r64["c0"], axis=-1)
        # each kernel within 4 x what fp32 costs its own restatement; the two restatements agree in fp64 (CPU test above)
        tol = 4.0 * float((np.linalg.norm(r32["points"].astype(np.float64) - r64["points"], axis=-1) / scale)[sel].max()) \
            + 4.0 * float((np.linalg.norm(t32["points"].astype(np.float64) - t64["points"], axis=-1) / scale)[sel].max())
        d = float((np.linalg.norm(tri["points"].astype(np.float64) - two.points.cpu().numpy(), axis=-1) / scale)[sel].max())
        print(f"scene {seed}: triangulate_nview(V = 2, iters = 0) - triangulate(midpoint) {d:.2e} relative over {int(sel.sum())} points, tolerance {tol:.2e}")
        assert sel.sum() > 500 and d <= tol


def _zero_rows(o, rows):
    return all(not o[k][rows].any() for k in OUTPUTS)


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True])
def test_defined_behaviour_on_bad_input(robust):
    V = 4
    s = scene(V, 1)
    base = _fields(_run(s, robust))
    N = 1000
    # NaN and inf observations: the same as not visible; nobody else notices
    bad, vis = s["x"].copy(), np.ones((V, N), bool)
    rows = np.array([0, 5, 63, 64, 65, 500, 999])
    for i, n in enumerate(rows):
        v = i % V
        bad[v, n, i % 2] = (np.nan, np.inf, -np.inf)[i % 3]
        vis[v, n] = False
    o = _fields(_run(s, robust, x=bad))
    hidden = _fields(_run(s, robust, visible=dev(vis)))
    keep = np.ones(N, bool)
    keep[rows] = False
    for k in OUTPUTS:
        assert np.isfinite(o[k].astype(np.float64)).all() and np.array_equal(o[k], hidden[k]), k
        assert np.array_equal(o[k][keep], base[k][keep]), k
    assert not ((o["views"][rows] >> (np.arange(len(rows)) % V).astype(np.uint32)) & 1).any()
    # a point seen by one view, or by none
    one = s["x"].copy()
    one[1:, :40] = np.nan
    one[:, 40:50] = np.nan
    o = _fields(_run(s, robust, x=one))
    assert _zero_rows(o, slice(0, 50)) and all(np.array_equal(o[k][50:], base[k][50:]) for k in OUTPUTS)
    # visible all zero
    o = _fields(_run(s, robust, visible=torch.zeros(V, N, dtype=torch.bool, device=DEV)))
    assert _zero_rows(o, slice(None))
    # a singular K in one view, a pose that is not finite in one view: that view sees nothing, and the others compute bit for bit what
    # they compute without it (c0 is the mean over the usable views)
    others = [0, 1, 3]
    from roma_amd import geometry
    less = _fields(geometry.triangulate_nview(dev(s["x"][others]), dev(s["R"][others]), dev(s["t"][others]), dev(s["K"][others]),
                                              max_view_error=THR if robust else None))
    moved = (less["views"] & np.uint32(3)) | ((less["views"] & np.uint32(4)) << np.uint32(1))
    for what in ("K", "R", "t"):
        broken = {k: s[k].copy() for k in ("K", "R", "t")}
        if what == "K":
            broken["K"][2, 1, 1] = 0.0
        else:
            broken[what][2, 0] = (np.nan if what == "R" else np.inf)
        o = _fields(geometry.triangulate_nview(dev(s["x"]), dev(broken["R"]), dev(broken["t"]), dev(broken["K"]), max_view_error=THR if robust else None))
        assert all(np.isfinite(o[k].astype(np.float64)).all() for k in OUTPUTS), what
        assert np.array_equal(o["views"], moved) and all(np.array_equal(o[k], less[k]) for k in FIELDS + ("valid",)), what
    # two identical cameras: parallel rays, no parallax; nothing is NaN or inf and nothing is valid behind a parallax gate
    same = dev(np.stack([s["x"][0], s["x"][0]]))
    eye, zero = dev(np.stack([np.eye(3)] * 2)), dev(np.zeros((2, 3)))
    o = _fields(geometry.triangulate_nview(same, eye, zero, dev(s["K"][:2] * 0 + s["K"][0]), max_view_error=THR if robust else None, min_parallax_deg=1.0))
    assert all(np.isfinite(o[k].astype(np.float64)).all() for k in OUTPUTS) and not o["valid"].any()


@pytest.mark.gpu
def test_refinement_never_raises_the_error_on_the_device():
    for robust in (False, True):
        for seed in range(3):
            s = scene(5, seed)
            o0, o3 = _fields(_run(s, robust, iters=0)), _fields(_run(s, robust, iters=3))
            same = o0["views"] == o3["views"]
            assert same.mean() > 0.99
            assert (o3["reproj"][same] <= o0["reproj"][same]).all()
            assert (o3["reproj"][same] < o0["reproj"][same]).mean() > 0.3


# ------------------------------------------------------------------------------------------------------------------ depth_from_warps
SIZE_A, SIZES_B = (1024, 1024), [(512, 1024), (1024, 512), (2048, 1024)]      # (H, W): powers of two, so that s * c + o rounds once


@functools.lru_cache(maxsize=None)
def synthetic_warps(seed, H=16, W=16, sigma=0.5):
    """k = 3 symmetric warps (H, 2W, 4) float32 of one known depth map of A in [4, 12] against the cameras 1 .. 3 of MS.cameras: the left
    half rows are [grid_A, x_Bv of the point + noise], the right half is filled with values that must not be read; 10 % of the rows
    of warp 0 are wrong, and the certainty of warp 1 is below the threshold on a block.  -> warps, certainties, depth, K, R, t"""
    rng = np.random.default_rng([seed, 21])
    K, R, t, _ = MS.cameras(4, seed)
    g = np.stack(np.meshgrid(np.linspace(-1 + 1 / W, 1 - 1 / W, W), np.linspace(-1 + 1 / H, 1 - 1 / H, H), indexing="xy"), -1)
    pa = np.stack([SIZE_A[1] / 2 * (g[..., 0] + 1), SIZE_A[0] / 2 * (g[..., 1] + 1)], -1)
    d = rng.uniform(4, 12, (H, W))
    X = (np.concatenate([pa, np.ones((H, W, 1))], -1) @ np.linalg.inv(K[0]).T) * d[..., None]
    warps, certs = [], []
    for v in range(1, 4):
        q = X @ R[v].T + t[v]
        assert (q[..., 2] > 1).all()
        p = q @ K[v].T
        pb = p[..., :2] / p[..., 2:] + rng.normal(0, sigma, (H, W, 2))
        hb, wb = SIZES_B[v - 1]
        nb = np.stack([2 / wb * pb[..., 0] - 1, 2 / hb * pb[..., 1] - 1], -1)
        if v == 1:
            wrong = rng.random((H, W)) < 0.1
            nb = np.where(wrong[..., None], rng.uniform(-1, 1, (H, W, 2)), nb)
        left = np.concatenate([g, nb], -1)
        right = rng.uniform(-1, 1, (H, W, 4))
        warps.append(np.concatenate([left, right], 1).astype(np.float32))
        c = rng.uniform(0.3, 1.0, (H, 2 * W))
        if v == 2:
            c[4:9, 3:11] = 0.01
        certs.append(c.astype(np.float32))
    return warps, certs, d, K, R, t


def _depth_fields(out):
    return out.depth_A, out.valid_A, out.num_views, out.reproj_error, out.points


@pytest.mark.gpu
def test_depth_from_warps_on_synthetic_warps():
    from roma_amd import geometry
    H = W = 16
    warps, certs, d, K, R, t = synthetic_warps(0)
    dw, dc = [dev(w) for w in warps], [dev(c) for c in certs]
    dR, dt, dKA, dK = dev(R[1:]), dev(t[1:]), dev(K[0]), dev(K[1:])
    kw = dict(sizes=SIZES_B, max_view_error=THR, max_reproj_error=GATE_REPROJ, min_parallax_deg=1.0)
    out = geometry.depth_from_warps(tuple(dw), tuple(dc), dR, dt, dKA, dK, *SIZE_A, **kw)
    assert out.depth_A.shape == (H, W) and out.valid_A.shape == (H, W) and out.valid_A.dtype == torch.bool and out.points.shape == (H, W, 3)
    assert out.num_views.dtype == torch.uint8 and out.depth_A.dtype == torch.float32 and out.reproj_error.shape == (H, W)
    assert all(bool(torch.isfinite(v.float()).all()) for v in _depth_fields(out))
    assert not bool(out.depth_A[~out.valid_A].any()) and float(out.valid_A.float().mean()) > 0.9
    # the block without certainty in warp 1 (view 2) never uses that view; A is used wherever anything is
    nv = out.num_views.cpu().numpy()
    assert nv[4:9, 3:11].max() <= 3 and nv.max() == 4
    # the same as triangulate_nview on the gathered pixel observations, bit for bit
    def px(c, size):
        return torch.stack([c[..., 0] * (size[1] / 2) + size[1] / 2, c[..., 1] * (size[0] / 2) + size[0] / 2], -1)
    x = torch.stack([px(dw[0][:, :W, :2], SIZE_A)] + [px(dw[i][:, :W, 2:], SIZES_B[i]) for i in range(3)]).reshape(4, H * W, 2)
    vis = torch.stack([torch.ones(H, W, dtype=torch.bool, device=DEV)] + [c[:, :W] > 0.05 for c in dc]).reshape(4, H * W)
    tri = geometry.triangulate_nview(x, dev(R), dev(t), dev(K), visible=vis, max_view_error=THR, max_reproj_error=GATE_REPROJ, min_parallax_deg=1.0)
    assert torch.equal(out.points.reshape(-1, 3), tri.points) and torch.equal(out.valid_A.reshape(-1), tri.valid)
    assert torch.equal(out.depth_A.reshape(-1), torch.where(tri.valid, tri.depth, 0.0)) and torch.equal(out.num_views.reshape(-1), tri.num_views)
    assert torch.equal(out.reproj_error.reshape(-1), tri.reproj_error)
    # one stacked tensor; the A halves with symmetric=False (views into the same memory); masks
    stacked = geometry.depth_from_warps(torch.stack(dw), torch.stack(dc), dR, dt, dKA, dK, *SIZE_A, **kw)
    halves = geometry.depth_from_warps([w[:, :W] for w in dw], [c[:, :W] for c in dc], dR, dt, dKA, dK, *SIZE_A, symmetric=False, **kw)
    for other in (stacked, halves):
        assert all(torch.equal(a, b) for a, b in zip(_depth_fields(other), _depth_fields(out)))
    masks = [torch.ones(H, 2 * W, device=DEV) for _ in range(3)]
    masks[1][4:9, 3:11] = 0
    high = [c.clone() for c in dc]
    high[1][4:9, 3:11] = 0.9
    masked = geometry.depth_from_warps(dw, high, dR, dt, dKA, dK, *SIZE_A, masks=masks, **kw)
    assert all(torch.equal(a, b) for a, b in zip(_depth_fields(masked), _depth_fields(out)))
    # a layout that cannot be read in place is refused
    with pytest.raises(ValueError, match="cannot be read in place"):
        geometry.depth_from_warps([w.transpose(0, 1).contiguous().transpose(0, 1) if i else w for i, w in enumerate(dw)], dc, dR, dt, dKA, dK,
                                  *SIZE_A, **kw)
    # better than the first warp alone
    alone = geometry.depth_from_warp(dw[0], dc[0], dR[0], dt[0], dKA, dK[0], *SIZE_A, *SIZES_B[0], max_reproj_error=GATE_REPROJ)
    va, vn = alone.valid_A.cpu().numpy(), out.valid_A.cpu().numpy()
    e_alone = float(np.median(np.abs(alone.depth_A.cpu().numpy() / d - 1)[va]))
    e_all = float(np.median(np.abs(out.depth_A.cpu().numpy() / d - 1)[vn]))
    print(f"median relative depth error: {e_all:.5f} from three warps over {int(vn.sum())} pixels, {e_alone:.5f} from the first alone over {int(va.sum())}")
    assert e_all < e_alone


@pytest.mark.gpu
def test_the_chain_on_four_views():
    """estimate_pose -> refine_pose -> triangulate on views 0, 1; find_absolute_pose of views 2 and 3 against that cloud; then all four"""
    from roma_amd import geometry
    from tests import general_scenes as GS
    s = MS.multiview_scene(4, 3, N=2000)
    both = s["seen"][0] & s["seen"][1]
    x = s["x"][:, both]
    z_true = s["X"][both, 2]                                                            # view 0 is the identity
    dx, K = dev(x), s["K"]
    thr = GS.calibrated_threshold(1.5, K[0], K[1])
    R1, t1, _ = geometry.estimate_pose(dx[0], dx[1], K[0], K[1], thr, seed=0)
    R1, t1, _ = geometry.refine_pose(R1, t1, dx[0], dx[1], K[0], K[1], thr)
    two = geometry.triangulate(dx[0], dx[1], R1, t1, K[0], K[1], max_reproj_error=GATE_REPROJ, min_parallax_deg=1.0)
    cloud = torch.where(two.valid[:, None], two.points.double(), float("nan"))
    Rs, ts = [torch.eye(3, dtype=torch.float64, device=DEV), R1], [torch.zeros(3, dtype=torch.float64, device=DEV), t1]
    for v in (2, 3):
        Rv, tv, mask = geometry.find_absolute_pose(cloud, dx[v], K[v], threshold=2.0, seed=0, refine_iters=15)
        assert int(mask.sum()) > 200
        Rs.append(Rv), ts.append(tv)
    tri = geometry.triangulate_nview(dx, torch.stack(Rs), torch.stack(ts), dev(K), max_view_error=THR, max_reproj_error=GATE_REPROJ, min_parallax_deg=1.0)
    scale = float(np.linalg.norm(s["t"][1])) / float(torch.linalg.norm(t1))             # the first baseline fixes the scale
    sel = (two.valid & tri.valid).cpu().numpy()
    e_two = float(np.median(np.abs(scale * two.depth_A.cpu().numpy() / z_true - 1)[sel]))
    e_all = float(np.median(np.abs(scale * tri.depth.cpu().numpy() / z_true - 1)[sel]))
    print(f"median relative depth error over {int(sel.sum())} tracks: {e_all:.5f} from four estimated views, {e_two:.5f} from the two-view cloud")
    assert sel.sum() > 800 and e_all < e_two


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    s = scene(5, 2)
    x, R, t, K = dev(s["x"]), dev(s["R"]), dev(s["t"]), dev(s["K"])
    warps, certs, _, Kw, Rw, tw = synthetic_warps(0)
    dw, dc = [dev(w) for w in warps], [dev(c) for c in certs]
    dRw, dtw, dKA, dKw = dev(Rw[1:]), dev(tw[1:]), dev(Kw[0]), dev(Kw[1:])

    def both():
        a = geometry.triangulate_nview(x, R, t, K, max_view_error=THR, max_reproj_error=GATE_REPROJ, min_parallax_deg=1.0)
        b = geometry.depth_from_warps(dw, dc, dRw, dtw, dKA, dKw, *SIZE_A, sizes=SIZES_B, max_view_error=THR)
        return (a.points, a.depth, a.reproj_error, a.cos_parallax, a.views, a.num_views, a.valid) + _depth_fields(b)

    eager = both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert int(out[6].sum()) > 500 and float(out[8].float().mean()) > 0.9
