"""roma_amd.geometry.refine_homography, the refine_iters keyword of find_homography and homography_corner_error
(csrc/homography_refine.hip) against the numpy restatement in tests/homography_refine_ref.py.  CPU tests pin the restatement (its
Jacobian, its descent, what it buys over 20 scenes), the C-ABI argument checks and the kernel's resource report; GPU tests pin the
kernel.

Parity bounds.  Device and restatement run the same fp64 algorithm from the same start and differ in the order of their sums, in
where a multiply-add is fused and in the last bits of division.  The cost is continuous but its minimiser is not a smooth function
of those last bits (a match whose e crosses thr^2 on one side only changes the weights), so the bounds are measured, not derived:
the largest discrepancy over scenes 11-14 (MEASURED_*, on an MI355X) times 10 — the margin is for another summation order —, under
hard ceilings that hold whatever is measured: 1e-9 for |H_dev - H_np|_F / |H_np|_F and 1e-10 for the relative cost, the ceilings of
the F refinement.  Measured: 1.77e-15 in the model, 1.28e-15 relative in the final cost, 5.18e-10 thr^2 in any match's e (an
outlier's), the same kept steps (3 / 6 / 6 / 4), inlier counts and masks on all four scenes; bounds: 1.77e-14, 1.28e-14, 5.18e-9
thr^2."""

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import geometry_ref as G
from tests import homography_refine_ref as HR
from tests.helpers import check_refine_entry_point_validates_arguments, dev, kernel_resources, to_np

DEV = "cuda:0"
THR = 1.5
SAMPLES = 300
SCENES = list(range(100, 120))

# largest device-vs-restatement discrepancy over scenes 11-14 (test_refine_parity_with_the_restatement prints them)
MEASURED_MODEL, MEASURED_COST_REL, MEASURED_E_REL = 1.77e-15, 1.28e-15, 5.18e-10
CEILING_MODEL, CEILING_COST_REL = 1e-9, 1e-10
PARITY_MODEL = min(10 * MEASURED_MODEL, CEILING_MODEL)       # |H_dev - H_np|_F / |H_np|_F
PARITY_COST_REL = min(10 * MEASURED_COST_REL, CEILING_COST_REL)   # |cost_dev - cost_np| / cost_np
PARITY_E_REL = 10 * MEASURED_E_REL                           # |e_dev - e_np| / thr^2 per match: the band in which masks may differ


def _assert_model(H):
    """what a refined model is: find_homography's convention"""
    assert H[2, 2] == 1.0 and np.isfinite(H).all()


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_analytic_jacobian_matches_central_differences():
    """dr/dh^ of the restatement at a perturbed model of a noisy scene, all matches (outliers included), the held column dropped,
    against central differences of the residual of the model that a step returns (in pixels, times s_B): 1e-8 relative to the largest
    entry."""
    xa, xb, _, H_true = G.planar_scene(5, N=400)
    ok = HR.usable(xa, xb)
    TA, TB, xah, xbh, sB = HR.normalised_points(xa, xb, ok)
    Hh = HR.to_normalised(H_true, TA, TB)
    Hh = HR.step(Hh, HR.held_entry(Hh), np.array([0.01, -0.02, 0.015, 0.02, 0.01, -0.01, 0.03, -0.015]))
    k = HR.held_entry(Hh)
    r, J = HR.residuals_and_jacobian(Hh, xah, xbh)
    J = J[:, :, np.arange(9) != k].reshape(-1, HR.NPAR)
    assert np.abs(r - sB * HR.residuals(HR.pixel_model(Hh, TA, TB), xa, xb)).max() < 1e-9      # the same residual in both coordinates
    h = 1e-6
    Jn = np.zeros_like(J)
    for j in range(HR.NPAR):
        d = np.zeros(HR.NPAR)
        d[j] = h
        rp = sB * HR.residuals(HR.pixel_model(HR.step(Hh, k, d), TA, TB), xa, xb)
        rm = sB * HR.residuals(HR.pixel_model(HR.step(Hh, k, -d), TA, TB), xa, xb)
        Jn[:, j] = ((rp - rm) / (2 * h)).reshape(-1)
    err, big = np.abs(J - Jn).max(), np.abs(J).max()
    print(f"analytic vs central differences: max |dJ| = {err:.2e}, max |J| = {big:.2e}, relative {err / big:.2e}")
    assert err < 1e-8 * big                                  # h^2 |r'''| + eps |r| / h ~ 1e-9 absolute here
    assert np.abs(J).max(0).min() > 1.0                      # every one of the eight columns is exercised


def test_restatement_descends_on_a_ransac_model():
    xa, xb = G.planar_scene(1)[:2]
    H0, _ = G.ransac("homography", xa, xb, THR, SAMPLES, seed=1)
    o = HR.refine(H0, xa, xb, THR)
    print(f"scene 1: cost {o['cost0']:.6e} -> {o['cost']:.6e} in {o['steps']} kept steps, {o['count']} inliers")
    assert o["steps"] >= 1 and all(b < a for a, b in zip(o["costs"], o["costs"][1:]))
    assert o["cost"] <= o["cost0"] and o["cost"] == o["costs"][-1] and o["count"] == int(o["mask"].sum())
    assert HR.truncated_cost(o["H"], xa, xb, THR) <= HR.truncated_cost(H0, xa, xb, THR)
    _assert_model(o["H"])
    again = HR.refine(o["H"], xa, xb, THR)
    assert again["steps"] == 0 and again["H"].tobytes() == o["H"].tobytes()
    # unchanged returns: too few weighted matches, a model that is not finite, zero
    few = HR.refine(H0, xa, xb, THR, mask=np.arange(len(xa)) < 3)
    assert few["count"] <= 3 and few["steps"] == 0 and np.array_equal(few["H"], H0)
    inl = np.nonzero(o["mask"])[0][:3]
    three = HR.refine(H0, xa, xb, THR, mask=np.isin(np.arange(len(xa)), inl))
    assert three["steps"] == 0 and np.array_equal(three["H"], H0)
    bad = H0.copy()
    bad[1, 1] = np.nan
    o1 = HR.refine(bad, xa, xb, THR)
    assert o1["steps"] == 0 and o1["H"].tobytes() == bad.tobytes() and o1["count"] == 0
    o2 = HR.refine(np.zeros((3, 3)), xa, xb, THR)
    assert o2["steps"] == 0 and np.array_equal(o2["H"], np.zeros((3, 3))) and o2["cost"] == len(xa) * THR ** 2


def test_refinement_improves_the_mean_accuracy_over_20_scenes():
    """From geometry_ref.ransac (300 samples, seed = scene), all 5 000 matches, thr = 1.5 px, 15 steps."""
    rows = []
    for seed in SCENES:
        xa, xb, _, H_true = G.planar_scene(seed)
        H0, _ = G.ransac("homography", xa, xb, THR, SAMPLES, seed=seed)
        o = HR.refine(H0, xa, xb, THR, iters=15)
        assert o["cost"] <= o["cost0"]
        assert HR.truncated_cost(o["H"], xa, xb, THR) <= HR.truncated_cost(H0, xa, xb, THR)
        rows.append((G.corner_error(H0, H_true), G.corner_error(o["H"], H_true)))
        print(f"scene {seed}: RANSAC corner error {rows[-1][0]:.4f} px, refined {rows[-1][1]:.4f} px, {o['steps']} steps, "
              f"cost {o['cost0']:.3f} -> {o['cost']:.3f}")
    m, a = np.mean(rows, 0), np.array(rows)
    print(f"mean over {len(rows)} scenes: corner error {m[0]:.4f} -> {m[1]:.4f} px (better on {(a[:, 1] < a[:, 0]).sum()})")
    assert m[1] < m[0]


def test_refine_homography_entry_point_validates_arguments_without_a_gpu():
    def bind(lib, a):
        def call(xa=a, xb=a, H_in=a, out=a, steps=a, P=1, N=100, thr=1.5, iters=15):
            return lib.roma_refine_homography(xa, xb, H_in, None, P, N, thr, iters, out, a, a, a, steps, None)
        return call

    check_refine_entry_point_validates_arguments("roma_refine_homography", bind, 4, null=("xa", "xb", "H_in", "out", "steps"),
                                                 misaligned=("xa", "xb"))
    assert _lib.load().roma_abi_version() == 5


def test_new_entry_points_refuse_cpu_tensors_and_bad_counts():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    H = torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.refine_homography(H, x, x, 1.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_homography(x, x, refine_iters=15)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.homography_corner_error(H, H, 1024, 768)
    with pytest.raises(ValueError, match="refine_iters"):
        geometry.find_homography(x, x, refine_iters=-1)


def test_homography_refine_kernel_uses_no_scratch_and_spills_nothing():
    """The compiler's resource report of csrc/homography_refine.hip (the recipe of test_fundamental_refine.py)."""
    kernels = kernel_resources("homography_refine.hip")
    assert any("refine_homography_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _assert_never_worse(H0, H, xa, xb, mask=None, thr=THR):
    """the truncated cost of the returned model, recomputed in numpy fp64, is not above that of the given one"""
    c0, c1 = HR.truncated_cost(H0, xa, xb, thr, mask), HR.truncated_cost(H, xa, xb, thr, mask)
    assert c1 <= c0, (c0, c1)
    return c0, c1


def _assert_output(H0, H, mask, info, xa, xb, mask_in=None, thr=THR):
    """what every call promises per pair: never worse; mask and count agree; the input bit for bit, or a model with H[2,2] = 1 below it"""
    c0, c1 = _assert_never_worse(H0, H, xa, xb, mask_in, thr)
    assert int(info["count"]) == int(mask.sum())
    if int(info["steps"]) == 0:
        assert H.tobytes() == H0.tobytes()
    else:
        _assert_model(H)
        assert c1 < c0


def _batch(first, n=8, N=2000, **kw):
    scenes = [G.planar_scene(first + i, N=N, **kw) for i in range(n)]
    return np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), np.stack([s[3] for s in scenes])


def _info(info, i):
    return {k: v[i] for k, v in info.items()}


def _same(o1, o2):
    return all(torch.equal(a, b) for a, b in zip(o1[:2], o2[:2])) and all(torch.equal(o1[2][k], o2[2][k]) for k in o1[2])


@pytest.mark.gpu
def test_refine_parity_with_the_restatement():
    from roma_amd import geometry
    figs, checks = [], []
    for seed in (11, 12, 13, 14):
        xa, xb = G.planar_scene(seed)[:2]
        H0, _ = geometry.find_homography(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=seed)
        H, mask, info = geometry.refine_homography(H0, dev(xa), dev(xb), THR, return_info=True)
        assert H.shape == (3, 3) and H.dtype == torch.float64 and mask.shape == (5000,) and mask.dtype == torch.bool
        H0, H, mask = to_np(H0, H, mask)
        o = HR.refine(H0, xa, xb, THR)
        _assert_output(H0, H, mask, info, xa, xb)
        ed, en = (HR.residuals(H, xa, xb) ** 2).sum(-1), (HR.residuals(o["H"], xa, xb) ** 2).sum(-1)
        fig = np.array([np.linalg.norm(H - o["H"]) / np.linalg.norm(o["H"]), abs(float(info["cost"]) - o["cost"]) / o["cost"],
                        np.abs(ed - en).max() / THR ** 2])
        differ = mask != o["mask"]
        print(f"scene {seed}: device vs restatement: |dH| / |H| {fig[0]:.3e}, cost {fig[1]:.3e} relative, e {fig[2]:.3e} thr^2; steps "
              f"{int(info['steps'])} / {o['steps']}, inliers {int(info['count'])} / {o['count']}, {int(differ.sum())} mask entries differ; "
              f"cost {o['cost0']:.4f} -> {o['cost']:.4f}, the start was {np.linalg.norm(H0 - o['H']) / np.linalg.norm(o['H']):.3e} away")
        figs.append(fig)
        band = np.abs(en - THR ** 2) <= PARITY_E_REL * THR ** 2
        checks.append((seed, differ, band, int(info["steps"]), o["steps"], int(info["count"]), o["count"]))
    worst = np.max(figs, 0)
    print(f"largest: |dH| / |H| {worst[0]:.3e}, cost {worst[1]:.3e}, e {worst[2]:.3e} thr^2")
    assert worst[0] <= PARITY_MODEL and worst[1] <= PARITY_COST_REL and worst[2] <= PARITY_E_REL, worst
    for seed, differ, band, sd, sn, cd, cn in checks:
        assert sd == sn and sd >= 1, (seed, sd, sn)
        assert cd == cn, (seed, cd, cn)
        assert not (differ & ~band).any(), seed                # masks differ only where e is within the tolerance of thr^2


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("N", [4, 100, 257, 1000])
def test_refine_small_and_awkward_shapes(N, P):
    """N = 4 is the minimal problem (no outliers, started from the scene's true H: the RANSAC fit of four matches is exact and leaves
    nothing to refine), 100 is fewer matches than threads, 257 and 1000 leave a tail."""
    from roma_amd import geometry
    xa, xb, H_true = _batch(40, n=P, N=N, **({"outlier_frac": 0.0} if N == 4 else {}))
    da, db = dev(xa), dev(xb)
    H0 = dev(H_true) if N == 4 else geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=3)[0]
    H, mask, info = geometry.refine_homography(H0, da, db, THR, return_info=True)
    assert H.shape == (P, 3, 3) and mask.shape == (P, N) and mask.dtype == torch.bool and info["steps"].shape == (P,)
    assert torch.equal(info["count"], mask.sum(-1).int())
    for i in range(P):
        _assert_output(*to_np(H0[i], H[i], mask[i]), _info(info, i), xa[i], xb[i])
    print(f"N = {N}, P = {P}: kept steps {info['steps'].tolist()}, inliers {info['count'].tolist()}")
    assert int(info["steps"].max()) >= 1


@pytest.mark.gpu
def test_refine_determinism_and_batch_independence():
    from roma_amd import geometry
    xa, xb, _ = _batch(20)
    da, db = dev(xa), dev(xb)
    H0, _ = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=5)
    o1 = geometry.refine_homography(H0, da, db, THR, return_info=True)
    o2 = geometry.refine_homography(H0, da, db, THR, return_info=True)
    assert o1[0].shape == (8, 3, 3) and o1[1].shape == (8, 2000) and o1[2]["steps"].shape == (8,)
    assert _same(o1, o2)
    assert int(o1[2]["steps"].max()) >= 1
    for i in range(8):
        _assert_output(*to_np(H0[i], o1[0][i], o1[1][i]), _info(o1[2], i), xa[i], xb[i])
        # pair i alone
        s = geometry.refine_homography(H0[i], da[i], db[i], THR, return_info=True)
        assert all(torch.equal(a, b[i]) for a, b in zip(s[:2], o1[:2])) and all(torch.equal(s[2][k], o1[2][k][i]) for k in s[2])
    # a refined model given back comes out bit for bit, with 0 steps
    o3 = geometry.refine_homography(o1[0], da, db, THR, return_info=True)
    assert torch.equal(o3[0], o1[0]) and torch.equal(o3[1], o1[1]) and int(o3[2]["steps"].max()) == 0
    assert torch.equal(o3[2]["cost"], o1[2]["cost"]) and torch.equal(o3[2]["count"], o1[2]["count"])
    # iters = 0 is the identity, with the model's own mask and count
    o4 = geometry.refine_homography(H0, da, db, THR, iters=0, return_info=True)
    assert torch.equal(o4[0], H0) and int(o4[2]["steps"].max()) == 0 and torch.equal(o4[2]["count"], o4[1].sum(-1).int())
    # the mask restricts the matches that carry weight: the same as handing over those matches alone
    only = torch.zeros(8, 2000, dtype=torch.bool, device=DEV)
    only[:, :1000] = True
    Hm, mm, im = geometry.refine_homography(H0, da, db, THR, mask=only, return_info=True)
    assert not bool(mm[:, 1000:].any()) and int(mm.sum()) > 0
    Hh, mh = geometry.refine_homography(H0, da[:, :1000], db[:, :1000], THR)
    assert torch.equal(Hm, Hh) and torch.equal(mm[:, :1000], mh)
    for i in range(8):
        _assert_output(*to_np(H0[i], Hm[i], mm[i]), _info(im, i), xa[i], xb[i], mask_in=only[i].cpu().numpy())
    # fp32 points are the same points in fp64
    H32, m32 = geometry.refine_homography(H0, da.float(), db.float(), THR)
    H64, m64 = geometry.refine_homography(H0, da.float().double(), db.float().double(), THR)
    assert torch.equal(H32, H64) and torch.equal(m32, m64)


@pytest.mark.gpu
def test_refine_of_degenerate_input_returns_the_input():
    """The guarded paths in one batch, and a model whose vanishing line crosses the data (w <= 0 for part of it): none of them faults,
    each guarded pair returns the model it was given, and the pairs next to them are what they are alone."""
    from roma_amd import geometry
    N = 500
    xa, xb, _ = _batch(60, n=7, N=N)
    H0, _ = geometry.find_homography(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=2)
    H0 = H0.clone()
    H0[1] = 0.0                                                                                     # a zero H
    H0[2, 2] = dev(np.array([1.0 / 512.0, 0.0, -1.0]))                                             # w = x / 512 - 1: zero at x = 512
    H0[3, 1, 1] = float("nan")                                                                      # an H that is not finite
    mask = torch.ones(7, N, dtype=torch.bool, device=DEV)
    mask[4, 3:] = False                                                                             # fewer than 4 matches
    xa[5], xb[5] = np.nan, np.nan                                                                   # no finite match
    H, m, info = geometry.refine_homography(H0, dev(xa), dev(xb), THR, mask=mask, return_info=True)
    for i in (1, 3, 4, 5):
        assert H[i].cpu().numpy().tobytes() == H0[i].cpu().numpy().tobytes(), i
        assert int(info["steps"][i]) == 0 and int(info["count"][i]) == int(m[i].sum()), i
        _assert_never_worse(*to_np(H0[i], H[i]), xa[i], xb[i], mask[i].cpu().numpy())
    assert not bool(m[1].any()) and not bool(m[3].any()) and not bool(m[5].any()) and int(m[4].sum()) <= 3 and not bool(m[4, 3:].any())
    assert float(info["cost"][5]) == 0.0 and float(info["cost"][1]) == N * THR ** 2
    w = xa[2, :, 0] / 512.0 - 1.0
    assert (w < 0).any() and (w > 0).any()
    _assert_output(*to_np(H0[2], H[2], m[2]), _info(info, 2), xa[2], xb[2])
    assert torch.isfinite(H[2]).all() and torch.isfinite(info["cost"][2])
    for i in (0, 2, 6):
        s = geometry.refine_homography(H0[i], dev(xa[i]), dev(xb[i]), THR, return_info=True)
        assert torch.equal(s[0], H[i]) and torch.equal(s[1], m[i]) and all(torch.equal(s[2][k], info[k][i]) for k in s[2])
    for i in (0, 6):
        assert int(info["steps"][i]) >= 1
        _assert_output(*to_np(H0[i], H[i], m[i]), _info(info, i), xa[i], xb[i])


@pytest.mark.gpu
def test_refine_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    xa, xb = G.planar_scene(30, N=3000)[:2]
    xa, xb = dev(xa), dev(xb)
    H0, _ = geometry.find_homography(xa, xb, threshold=THR, max_iters=SAMPLES, seed=11)
    eager = geometry.refine_homography(H0, xa, xb, THR, return_info=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        geometry.refine_homography(H0, xa, xb, THR, return_info=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = geometry.refine_homography(H0, xa, xb, THR, return_info=True)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    assert int(out[2]["steps"]) >= 1
    _assert_output(*to_np(H0, out[0], out[1]), out[2], xa.cpu().numpy(), xb.cpu().numpy())


@pytest.mark.gpu
def test_refine_iters_zero_is_the_unchanged_default():
    from roma_amd import geometry
    xa, xb, _ = _batch(80, n=3, N=1500)
    da, db = dev(xa).float(), dev(xb).float()
    a = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=9)
    b = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=9, refine_iters=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and refine_iters > 0 is find_homography followed by refine_homography on all matches
    c = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=9, refine_iters=15)
    d = geometry.refine_homography(a[0], da, db, THR, iters=15)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and not torch.equal(c[0], a[0])


@pytest.mark.gpu
def test_refined_find_homography_is_more_accurate_over_20_scenes():
    """find_homography with refine_iters = 15 against the same call without, 300 samples, seed = scene, thr = 1.5 px: the mean
    distance of the four warped corners to where the true H puts them drops."""
    from roma_amd import geometry
    rows = []
    for seed in SCENES:
        xa, xb, _, H_true = G.planar_scene(seed)
        da, db = dev(xa), dev(xb)
        H0, _ = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=seed)
        H1, _ = geometry.find_homography(da, db, threshold=THR, max_iters=SAMPLES, seed=seed, refine_iters=15)
        H0, H1 = to_np(H0, H1)
        c0, c1 = _assert_never_worse(H0, H1, xa, xb)
        rows.append((G.corner_error(H0, H_true), G.corner_error(H1, H_true)))
        print(f"scene {seed}: find_homography corner error {rows[-1][0]:.4f} px, refine_iters=15 {rows[-1][1]:.4f} px, "
              f"cost {c0:.3f} -> {c1:.3f}")
    m, a = np.mean(rows, 0), np.array(rows)
    print(f"mean over {len(rows)} scenes: corner error {m[0]:.4f} -> {m[1]:.4f} px (better on {(a[:, 1] < a[:, 0]).sum()})")
    assert m[1] < m[0]


@pytest.mark.gpu
def test_homography_corner_error_is_the_benchmark_metric():
    """against the numpy restatement of the benchmark's lines, 1e-9 px, on planar_scene truths and estimates, w, h = 1024, 768"""
    from roma_amd import geometry
    W, Hh = G.W_IMG, G.H_IMG
    xa, xb, H_true = _batch(90, n=4, N=1000)
    H_est, _ = geometry.find_homography(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=1)
    scale = min(W, Hh) / 480.0
    got = geometry.homography_corner_error(H_est, dev(H_true), W, Hh, scale)
    assert got.shape == (4,) and got.dtype == torch.float64
    want = np.array([HR.corner_error_hpatches(e, t, W, Hh, scale) for e, t in zip(H_est.cpu().numpy(), H_true)])
    print(f"corner errors {got.tolist()} px, restatement {want.tolist()}")
    assert np.abs(got.cpu().numpy() - want).max() < 1e-9 and (want > 0).all()
    one = geometry.homography_corner_error(H_est[0], H_true[0], W, Hh)                 # a single pair, a numpy truth, scale 1
    assert one.shape == () and abs(float(one) - HR.corner_error_hpatches(H_est[0].cpu().numpy(), H_true[0], W, Hh)) < 1e-9
    zero = H_est.clone()
    zero[2] = 0.0                                                                      # find_homography's "no model"
    z = geometry.homography_corner_error(zero, dev(H_true), W, Hh, scale)
    assert torch.isinf(z[2]) and z[2] > 0 and torch.equal(z[[0, 1, 3]], got[[0, 1, 3]])


@pytest.mark.gpu
def test_refined_homography_integration_with_match_and_sample():
    from roma_amd import geometry
    from roma_amd.model_zoo import build_roma
    from roma_amd.synthetic import load_synthetic_weights, synthetic_pair
    torch.set_grad_enabled(False)
    model = build_roma((112, 112), upsample_preds=True, amp_dtype=torch.float32)
    load_synthetic_weights(model, seed=0)
    model.upsample_res = (168, 168)
    model = model.to(DEV).eval()
    pairs = [synthetic_pair(i, (112, 112), (168, 168)) for i in range(2)]
    batch = [torch.cat([p[j] for p in pairs]).to(DEV) for j in range(4)]
    warp, cert = model.match_tensors(*batch)
    kA, kB = [], []
    for i in range(2):
        m, c = model.sample(warp[i], cert[i], num=500, seed=i)
        a, b = model.to_pixel_coordinates(m, 480, 640, 480, 640)
        kA.append(a)
        kB.append(b)
    kA, kB = torch.stack(kA), torch.stack(kB)
    H0, m0 = geometry.find_homography(kA, kB, max_iters=1000, seed=0)
    H, mask = geometry.find_homography(kA, kB, max_iters=1000, seed=0, refine_iters=15)
    assert H.shape == (2, 3, 3) and mask.shape == (2, 500) and mask.dtype == torch.bool and torch.isfinite(H).all()
    for i in range(2):
        xa, xb = kA[i].double().cpu().numpy(), kB[i].double().cpu().numpy()
        c0, c1 = _assert_never_worse(*to_np(H0[i], H[i]), xa, xb, thr=3.0)
        print(f"pair {i}: cost {c0:.4f} -> {c1:.4f}, {int(m0[i].sum())} -> {int(mask[i].sum())} inliers")
