"""roma_amd.geometry.refine_fundamental and the refine_iters keyword of find_fundamental / estimate_pose_uncalibrated
(csrc/fundamental_refine.hip) against the numpy restatement in tests/fundamental_refine_ref.py.  CPU tests pin the restatement (its
Jacobian, its descent, what it buys over 20 scenes), the C-ABI argument checks and the kernel's resource report; GPU tests pin the
kernel.

Parity bounds.  Device and restatement run the same fp64 algorithm from the same start and differ in the order of their sums and in
the last bits of sqrt and division.  The cost is continuous but its minimiser is not a smooth function of those last bits (a match
whose r^2 crosses thr^2 on one side only changes the weights), so the bounds are measured, not derived: the largest discrepancy over
scenes 11-14 (MEASURED_*, on an MI355X) times 10 — the margin is for another summation order —, under hard ceilings that hold
whatever is measured: 1e-9 for |F_dev - F_np|_F (unit-norm models) and 1e-10 for the relative cost.  Measured: 1.51e-16 in the
model, 3.49e-16 relative in the final cost, 1.30e-10 thr^2 in any match's r^2 (an outlier's), the same kept steps (6 / 7 / 3 / 4),
inlier counts and masks on all four scenes; bounds: 1.51e-15, 3.49e-15, 1.30e-9 thr^2."""

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import fundamental_refine_ref as FR
from tests import geometry_ref as G
from tests import pose_ref as PR
from tests.helpers import check_refine_entry_point_validates_arguments, dev, kernel_resources, to_np

DEV = "cuda:0"
THR = 1.5
SAMPLES = 300
SCENES = list(range(100, 120))

# largest device-vs-restatement discrepancy over scenes 11-14 (test_refine_parity_with_the_restatement prints them)
MEASURED_MODEL, MEASURED_COST_REL, MEASURED_R2_REL = 1.51e-16, 3.49e-16, 1.30e-10
CEILING_MODEL, CEILING_COST_REL = 1e-9, 1e-10
PARITY_MODEL = min(10 * MEASURED_MODEL, CEILING_MODEL)       # |F_dev - F_np|_F
PARITY_COST_REL = min(10 * MEASURED_COST_REL, CEILING_COST_REL)   # |cost_dev - cost_np| / cost_np
PARITY_R2_REL = 10 * MEASURED_R2_REL                         # |r^2_dev - r^2_np| / thr^2 per match: the band in which masks may differ


def _rms_clean(F, scene):
    """RMS Sampson distance (pixels) of the noise-free true inliers of a two_view_scene to the model"""
    truth, ca, cb = scene[2], scene[4], scene[5]
    return float(np.sqrt(G.errors("fundamental", F, ca[truth], cb[truth]).mean()))


def _pose_errors(F, mask, xa, xb, seed):
    """(rotation, translation) error in degrees of the pose pose_ref.recover_pose makes from K^T F K"""
    K, R_true, t_true = PR.scene_pose(seed)
    R, t = PR.recover_pose(K.T @ F @ K, xa, xb, K, K, mask)[:2]
    return PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)


def _assert_model(F):
    """what a refined model is: rank 2, unit Frobenius norm, largest-magnitude entry positive"""
    sv = np.linalg.svd(F, compute_uv=False)
    assert sv[2] / sv[0] < 1e-12, sv
    assert abs(np.linalg.norm(F) - 1.0) < 1e-12
    assert F.flat[np.abs(F).argmax()] > 0


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_analytic_jacobian_matches_central_differences():
    """dr/d(w_u, w_v, ds) of the restatement at a perturbed model of a noisy scene, all matches (outliers included), against central
    differences of the residual of the model that a step returns: 1e-8 relative to the largest entry."""
    xa, xb, _, F_true = G.two_view_scene(5, N=400)[:4]
    TA, TB = FR.normalisation(xa, xb, FR.usable(xa, xb))
    U, s, V = FR.step(*FR.factorise(F_true, TA, TB), np.array([0.01, -0.02, 0.015, 0.02, 0.01, -0.01, 0.03]))
    r, J = FR.residuals_and_jacobian(U, s, V, TA, TB, xa, xb)
    sign = np.sign(FR.residuals(FR.pixel_model(U, s, V, TA, TB), xa, xb) * r)      # the returned model fixes its sign, r follows it
    assert (sign != 0).all() and len(set(sign)) == 1
    h = 1e-6
    Jn = np.zeros_like(J)
    for k in range(FR.NPAR):
        d = np.zeros(FR.NPAR)
        d[k] = h
        rp = FR.residuals(FR.pixel_model(*FR.step(U, s, V, d), TA, TB), xa, xb)
        rm = FR.residuals(FR.pixel_model(*FR.step(U, s, V, -d), TA, TB), xa, xb)
        Jn[:, k] = sign * (rp - rm) / (2 * h)
    err, big = np.abs(J - Jn).max(), np.abs(J).max()
    print(f"analytic vs central differences: max |dJ| = {err:.2e}, max |J| = {big:.2e}, relative {err / big:.2e}")
    assert err < 1e-8 * big                                  # h^2 |r'''| + eps |r| / h ~ 1e-7 absolute here
    assert np.abs(J).max(0).min() > 1.0                      # every one of the seven columns is exercised


def test_restatement_descends_on_a_ransac_model():
    xa, xb = G.two_view_scene(1)[:2]
    F0, _ = G.ransac("fundamental", xa, xb, THR, SAMPLES, seed=1)
    o = FR.refine(F0, xa, xb, THR)
    print(f"scene 1: cost {o['cost0']:.6e} -> {o['cost']:.6e} in {o['steps']} kept steps, {o['count']} inliers")
    assert o["steps"] >= 1 and all(b < a for a, b in zip(o["costs"], o["costs"][1:]))
    assert o["cost"] <= o["cost0"] and o["cost"] == o["costs"][-1] and o["count"] == int(o["mask"].sum())
    assert FR.truncated_cost(o["F"], xa, xb, THR) <= FR.truncated_cost(F0, xa, xb, THR)
    _assert_model(o["F"])
    again = FR.refine(o["F"], xa, xb, THR)
    assert again["steps"] == 0 and np.array_equal(again["F"], o["F"])
    # unchanged returns: too few weighted matches, a model that is not finite, rank 1, zero
    few = FR.refine(F0, xa, xb, THR, mask=np.arange(len(xa)) < 7)
    assert few["steps"] == 0 and np.array_equal(few["F"], F0)
    bad = FR.refine(F0 * np.nan, xa, xb, THR)
    assert bad["steps"] == 0 and np.isnan(bad["F"]).all()
    rank1 = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0])
    for F in (rank1, np.zeros((3, 3))):
        o1 = FR.refine(F, xa, xb, THR)
        assert o1["steps"] == 0 and np.array_equal(o1["F"], F)


def test_refinement_improves_the_mean_accuracy_over_20_scenes():
    """From geometry_ref.ransac (300 samples, seed = scene), all 5 000 matches, thr = 1.5 px, 15 steps."""
    rows = []
    for seed in SCENES:
        scene = G.two_view_scene(seed)
        xa, xb = scene[:2]
        F0, m0 = G.ransac("fundamental", xa, xb, THR, SAMPLES, seed=seed)
        o = FR.refine(F0, xa, xb, THR, iters=15)
        assert o["cost"] <= o["cost0"]
        assert FR.truncated_cost(o["F"], xa, xb, THR) <= FR.truncated_cost(F0, xa, xb, THR)
        rows.append((_rms_clean(F0, scene), *_pose_errors(F0, m0, xa, xb, seed), _rms_clean(o["F"], scene),
                     *_pose_errors(o["F"], o["mask"], xa, xb, seed)))
        print(f"scene {seed}: RANSAC rms {rows[-1][0]:.4f} px, pose {rows[-1][1]:.4f} / {rows[-1][2]:.4f} deg; refined rms "
              f"{rows[-1][3]:.4f} px, pose {rows[-1][4]:.4f} / {rows[-1][5]:.4f} deg (rotation / translation), {o['steps']} steps, "
              f"cost {o['cost0']:.3f} -> {o['cost']:.3f}")
    m = np.mean(rows, 0)
    a = np.array(rows)
    print(f"mean over {len(rows)} scenes: rms {m[0]:.4f} -> {m[3]:.4f} px (better on {(a[:, 3] < a[:, 0]).sum()}), rotation "
          f"{m[1]:.4f} -> {m[4]:.4f} deg, translation {m[2]:.4f} -> {m[5]:.4f} deg (better on {(a[:, 5] < a[:, 2]).sum()})")
    assert m[3] < m[0] and m[5] < m[2]


def test_refine_fundamental_entry_point_validates_arguments_without_a_gpu():
    def bind(lib, a):
        def call(xa=a, xb=a, F_in=a, out=a, steps=a, P=1, N=100, thr=1.5, iters=15):
            return lib.roma_refine_fundamental(xa, xb, F_in, None, P, N, thr, iters, out, a, a, a, steps, None)
        return call

    check_refine_entry_point_validates_arguments("roma_refine_fundamental", bind, 8, null=("xa", "xb", "F_in", "out", "steps"),
                                                 misaligned=("xa", "xb"))
    assert _lib.load().roma_abi_version() == 5


def test_new_entry_points_refuse_cpu_tensors_and_bad_counts():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    F = torch.eye(3, dtype=torch.float64)
    K = torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.refine_fundamental(F, x, x, 1.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_fundamental(x, x, refine_iters=15)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_pose_uncalibrated(x, x, K, K, 1.5, refine_iters=15)
    with pytest.raises(ValueError, match="refine_iters"):
        geometry.find_fundamental(x, x, refine_iters=-1)
    with pytest.raises(ValueError, match="refine_iters"):
        geometry.estimate_pose_uncalibrated(x, x, K, K, 1.5, refine_iters=-1)


def test_fundamental_refine_kernel_uses_no_scratch_and_spills_nothing():
    """The compiler's resource report of csrc/fundamental_refine.hip (the recipe of test_pose_refine.py)."""
    kernels = kernel_resources("fundamental_refine.hip")
    assert any("refine_fundamental_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _assert_never_worse(F0, F, xa, xb, mask=None, thr=THR):
    """the truncated cost of the returned model, recomputed in numpy fp64, is not above that of the given one"""
    c0, c1 = FR.truncated_cost(F0, xa, xb, thr, mask), FR.truncated_cost(F, xa, xb, thr, mask)
    assert c1 <= c0, (c0, c1)
    return c0, c1


def _assert_output(F0, F, mask, info, xa, xb, mask_in=None, thr=THR):
    """what every call promises per pair: never worse; mask and count agree; the input bit for bit, or a rank-2 model below it"""
    c0, c1 = _assert_never_worse(F0, F, xa, xb, mask_in, thr)
    assert int(info["count"]) == int(mask.sum())
    if int(info["steps"]) == 0:
        assert F.tobytes() == F0.tobytes()
    else:
        _assert_model(F)
        assert c1 < c0


def _batch(first, n=8, N=2000):
    scenes = [G.two_view_scene(first + i, N=N) for i in range(n)]
    return np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])


def _info(info, i):
    return {k: v[i] for k, v in info.items()}


@pytest.mark.gpu
def test_refine_parity_with_the_restatement():
    from roma_amd import geometry
    figs, checks = [], []
    for seed in (11, 12, 13, 14):
        xa, xb = G.two_view_scene(seed)[:2]
        F0, _ = geometry.find_fundamental(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=seed)
        F, mask, info = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, return_info=True)
        assert F.shape == (3, 3) and F.dtype == torch.float64 and mask.shape == (5000,) and mask.dtype == torch.bool
        F0, F, mask = to_np(F0, F, mask)
        o = FR.refine(F0, xa, xb, THR)
        _assert_output(F0, F, mask, info, xa, xb)
        r2d, r2n = FR.residuals(F, xa, xb) ** 2, FR.residuals(o["F"], xa, xb) ** 2
        fig = np.array([np.linalg.norm(F - o["F"]), abs(float(info["cost"]) - o["cost"]) / o["cost"], np.abs(r2d - r2n).max() / THR ** 2])
        differ = mask != o["mask"]
        print(f"scene {seed}: device vs restatement: |dF| {fig[0]:.3e}, cost {fig[1]:.3e} relative, r^2 {fig[2]:.3e} thr^2; steps "
              f"{int(info['steps'])} / {o['steps']}, inliers {int(info['count'])} / {o['count']}, {int(differ.sum())} mask entries differ; "
              f"cost {o['cost0']:.4f} -> {o['cost']:.4f}, the start was {np.linalg.norm(F0 - o['F']):.3e} away")
        figs.append(fig)
        band = np.abs(r2n - THR ** 2) <= PARITY_R2_REL * THR ** 2
        checks.append((seed, differ, band, int(info["steps"]), o["steps"], int(info["count"]), o["count"]))
    worst = np.max(figs, 0)
    print(f"largest: |dF| {worst[0]:.3e}, cost {worst[1]:.3e}, r^2 {worst[2]:.3e} thr^2")
    assert worst[0] <= PARITY_MODEL and worst[1] <= PARITY_COST_REL and worst[2] <= PARITY_R2_REL, worst
    for seed, differ, band, sd, sn, cd, cn in checks:
        assert sd == sn and sd >= 1, (seed, sd, sn)
        assert cd == cn, (seed, cd, cn)
        assert not (differ & ~band).any(), seed                # masks differ only where r^2 is within the tolerance of thr^2


@pytest.mark.gpu
def test_refine_determinism_and_batch_independence():
    from roma_amd import geometry
    xa, xb = _batch(20)
    F0, _ = geometry.find_fundamental(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=5)
    o1 = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, return_info=True)
    o2 = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, return_info=True)
    assert o1[0].shape == (8, 3, 3) and o1[1].shape == (8, 2000) and o1[2]["steps"].shape == (8,)
    assert all(torch.equal(a, b) for a, b in zip(o1[:2], o2[:2])) and all(torch.equal(o1[2][k], o2[2][k]) for k in o1[2])
    assert int(o1[2]["steps"].max()) >= 1
    for i in range(8):
        _assert_output(*to_np(F0[i], o1[0][i], o1[1][i]), _info(o1[2], i), xa[i], xb[i])
        # pair i alone
        s = geometry.refine_fundamental(F0[i], dev(xa[i]), dev(xb[i]), THR, return_info=True)
        assert all(torch.equal(a, b[i]) for a, b in zip(s[:2], o1[:2])) and all(torch.equal(s[2][k], o1[2][k][i]) for k in s[2])
    # a refined model given back comes out bit for bit, with 0 steps
    o3 = geometry.refine_fundamental(o1[0], dev(xa), dev(xb), THR, return_info=True)
    assert torch.equal(o3[0], o1[0]) and torch.equal(o3[1], o1[1]) and int(o3[2]["steps"].max()) == 0
    assert torch.equal(o3[2]["cost"], o1[2]["cost"]) and torch.equal(o3[2]["count"], o1[2]["count"])
    # iters = 0 is the identity, with the model's own mask and cost
    o4 = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, iters=0, return_info=True)
    assert torch.equal(o4[0], F0) and int(o4[2]["steps"].max()) == 0 and torch.equal(o4[2]["count"], o4[1].sum(-1).int())
    # the mask restricts the matches that carry weight: the same as handing over those matches alone
    only = torch.zeros(8, 2000, dtype=torch.bool, device=DEV)
    only[:, :1000] = True
    Fm, mm, im = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, mask=only, return_info=True)
    assert not bool(mm[:, 1000:].any()) and int(mm.sum()) > 0
    Fh, mh = geometry.refine_fundamental(F0, dev(xa[:, :1000]), dev(xb[:, :1000]), THR)
    assert torch.equal(Fm, Fh) and torch.equal(mm[:, :1000], mh)
    for i in range(8):
        _assert_output(*to_np(F0[i], Fm[i], mm[i]), _info(im, i), xa[i], xb[i], mask_in=only[i].cpu().numpy())
    # fp32 points are the same points in fp64
    F32, m32 = geometry.refine_fundamental(F0, dev(xa).float(), dev(xb).float(), THR)
    F64, m64 = geometry.refine_fundamental(F0, dev(xa).float().double(), dev(xb).float().double(), THR)
    assert torch.equal(F32, F64) and torch.equal(m32, m64)


@pytest.mark.gpu
def test_refine_of_degenerate_input_returns_the_input():
    """The guarded paths in one batch: none of them faults, each returns the model it was given, and the pairs next to them are what
    they are alone."""
    from roma_amd import geometry
    N = 500
    xa, xb = _batch(60, n=7, N=N)
    F0, _ = geometry.find_fundamental(dev(xa), dev(xb), threshold=THR, max_iters=SAMPLES, seed=2)
    F0 = F0.clone()
    F0[1] = 0.0                                                                                     # a zero F
    F0[2] = dev(np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]) / 10.0)                                # a rank-1 F
    F0[3, 1, 1] = float("nan")                                                                      # an F that is not finite
    mask = torch.ones(7, N, dtype=torch.bool, device=DEV)
    mask[4, 7:] = False                                                                             # fewer than 8 matches
    xa[5], xb[5] = np.nan, np.nan                                                                   # no finite match
    F, m, info = geometry.refine_fundamental(F0, dev(xa), dev(xb), THR, mask=mask, return_info=True)
    for i in (1, 2, 3, 4, 5):
        assert F[i].cpu().numpy().tobytes() == F0[i].cpu().numpy().tobytes(), i
        assert int(info["steps"][i]) == 0 and int(info["count"][i]) == int(m[i].sum()), i
        _assert_never_worse(*to_np(F0[i], F[i]), xa[i], xb[i], mask[i].cpu().numpy())
    assert not bool(m[1].any()) and not bool(m[3].any()) and not bool(m[5].any()) and int(m[4].sum()) <= 7 and not bool(m[4, 7:].any())
    assert float(info["cost"][5]) == 0.0 and float(info["cost"][1]) == N * THR ** 2
    for i in (0, 6):
        s = geometry.refine_fundamental(F0[i], dev(xa[i]), dev(xb[i]), THR, return_info=True)
        assert torch.equal(s[0], F[i]) and torch.equal(s[1], m[i]) and all(torch.equal(s[2][k], info[k][i]) for k in s[2])
        assert int(info["steps"][i]) >= 1
        _assert_output(*to_np(F0[i], F[i], m[i]), _info(info, i), xa[i], xb[i])


@pytest.mark.gpu
def test_refine_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(30, N=3000)[:2]
    xa, xb = dev(xa), dev(xb)
    F0, _ = geometry.find_fundamental(xa, xb, threshold=THR, max_iters=SAMPLES, seed=11)
    eager = geometry.refine_fundamental(F0, xa, xb, THR, return_info=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        geometry.refine_fundamental(F0, xa, xb, THR, return_info=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = geometry.refine_fundamental(F0, xa, xb, THR, return_info=True)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out[:2], eager[:2])) and all(torch.equal(out[2][k], eager[2][k]) for k in out[2])
    assert int(out[2]["steps"]) >= 1
    _assert_output(*to_np(F0, out[0], out[1]), out[2], xa.cpu().numpy(), xb.cpu().numpy())


@pytest.mark.gpu
def test_refined_estimators_are_more_accurate_over_20_scenes():
    """find_fundamental and estimate_pose_uncalibrated with refine_iters = 15 against the same calls without, 300 samples, seed =
    scene, thr = 1.5 px: the mean RMS distance of the clean inliers and the mean translation error both drop."""
    from roma_amd import geometry
    K = PR.K_SCENE
    rows = []
    for seed in SCENES:
        scene = G.two_view_scene(seed)
        xa, xb = scene[:2]
        _, R_true, t_true = PR.scene_pose(seed)
        da, db = dev(xa), dev(xb)
        F0, m0 = geometry.find_fundamental(da, db, threshold=THR, max_iters=SAMPLES, seed=seed)
        F1, m1 = geometry.find_fundamental(da, db, threshold=THR, max_iters=SAMPLES, seed=seed, refine_iters=15)
        Rp, tp, _ = geometry.estimate_pose_uncalibrated(da, db, K, K, THR, max_iters=SAMPLES, seed=seed)
        Rq, tq, _ = geometry.estimate_pose_uncalibrated(da, db, K, K, THR, max_iters=SAMPLES, seed=seed, refine_iters=15)
        F0, F1, Rp, tp, Rq, tq = to_np(F0, F1, Rp, tp, Rq, tq)
        c0, c1 = _assert_never_worse(F0, F1, xa, xb)
        rows.append((_rms_clean(F0, scene), PR.rotation_error_deg(Rp, R_true), PR.translation_error_deg(tp, t_true),
                     _rms_clean(F1, scene), PR.rotation_error_deg(Rq, R_true), PR.translation_error_deg(tq, t_true)))
        print(f"scene {seed}: find_fundamental rms {rows[-1][0]:.4f} px, pose {rows[-1][1]:.4f} / {rows[-1][2]:.4f} deg; refine_iters=15 "
              f"rms {rows[-1][3]:.4f} px, pose {rows[-1][4]:.4f} / {rows[-1][5]:.4f} deg (rotation / translation), cost {c0:.3f} -> {c1:.3f}")
    m = np.mean(rows, 0)
    a = np.array(rows)
    print(f"mean over {len(rows)} scenes: rms {m[0]:.4f} -> {m[3]:.4f} px (better on {(a[:, 3] < a[:, 0]).sum()}), rotation "
          f"{m[1]:.4f} -> {m[4]:.4f} deg, translation {m[2]:.4f} -> {m[5]:.4f} deg (better on {(a[:, 5] < a[:, 2]).sum()})")
    assert m[3] < m[0] and m[5] < m[2]


@pytest.mark.gpu
def test_refine_iters_zero_is_the_unchanged_default():
    from roma_amd import geometry
    xa, xb = _batch(80, n=3, N=1500)
    da, db = dev(xa).float(), dev(xb).float()
    K = PR.K_SCENE
    a = geometry.find_fundamental(da, db, threshold=THR, max_iters=SAMPLES, seed=9)
    b = geometry.find_fundamental(da, db, threshold=THR, max_iters=SAMPLES, seed=9, refine_iters=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p = geometry.estimate_pose_uncalibrated(da, db, K, K, THR, max_iters=SAMPLES, seed=9)
    q = geometry.estimate_pose_uncalibrated(da, db, K, K, THR, max_iters=SAMPLES, seed=9, refine_iters=0)
    assert all(torch.equal(x, y) for x, y in zip(p, q))
    # and refine_iters > 0 is find_fundamental followed by refine_fundamental on all matches
    c = geometry.find_fundamental(da, db, threshold=THR, max_iters=SAMPLES, seed=9, refine_iters=15)
    d = geometry.refine_fundamental(a[0], da, db, THR, iters=15)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and not torch.equal(c[0], a[0])


@pytest.mark.gpu
def test_refined_fundamental_integration_with_match_and_sample():
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
    F0, m0 = geometry.find_fundamental(kA, kB, max_iters=1000, seed=0)
    F, mask = geometry.find_fundamental(kA, kB, max_iters=1000, seed=0, refine_iters=15)
    assert F.shape == (2, 3, 3) and mask.shape == (2, 500) and mask.dtype == torch.bool and torch.isfinite(F).all()
    for i in range(2):
        xa, xb = kA[i].double().cpu().numpy(), kB[i].double().cpu().numpy()
        c0, c1 = _assert_never_worse(*to_np(F0[i], F[i]), xa, xb, thr=3.0)
        sv = np.linalg.svd(F[i].cpu().numpy(), compute_uv=False)
        print(f"pair {i}: cost {c0:.4f} -> {c1:.4f}, sigma_3 / sigma_1 = {sv[2] / sv[0]:.2e}")
        assert sv[2] / sv[0] < 1e-12
