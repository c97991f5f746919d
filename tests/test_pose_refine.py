"""roma_amd.geometry.refine_pose / estimate_relative_pose / pose_error (csrc/pose_refine.hip) against the numpy restatement in
tests/pose_refine_ref.py.  CPU tests pin the restatement (its Jacobian, its descent, what it buys over 20 scenes), the C-ABI
argument checks and the kernel's resource report; GPU tests pin the kernel.

Parity bounds.  Device and restatement run the same fp64 algorithm from the same start and differ in the order of their sums and in
the last bits of sqrt and division.  The cost is continuous but its minimiser is not a smooth function of those last bits: a match
whose r^2 crosses thr^2 on one side only changes the weights.  So the bounds are measured, not derived: the largest discrepancy
over scenes 11-14 (MEASURED_*, on an MI355X) times 10.  Measured: 6.8e-15 deg in R, 4.3e-14 deg in t, 4.3e-16 relative in the final
cost, 1.27e-10 thr^2 in any match's r^2 (an outlier's), the same kept steps, inlier counts and masks on all four scenes; bounds:
6.8e-14 deg, 4.3e-13 deg, 4.3e-15, 1.27e-9 thr^2.  No match crossed thr^2 on one side only in these runs."""

import numpy as np
import pytest
import torch

from tests import geometry_ref as G
from tests import pose_ref as PR
from tests import pose_refine_ref as RR
from tests.helpers import check_refine_entry_point_validates_arguments, dev, kernel_resources, to_np

DEV = "cuda:0"
THR = 1.5 / 800                                              # 1.5 px at the scenes' focal length
ROT_BOUND_DEG, TRANS_BOUND_DEG = 0.1, 1.0                    # the per-scene bounds of tests/test_pose.py
SCENES = list(range(11, 15)) + list(range(100, 116))
CAMERA = {"model": "PINHOLE", "width": G.W_IMG, "height": G.H_IMG, "params": [800.0, 800.0, G.W_IMG / 2, G.H_IMG / 2]}

# largest device-vs-restatement discrepancy over scenes 11-14 (test_refine_parity_with_the_restatement prints them)
MEASURED_ROT_DEG, MEASURED_TRANS_DEG, MEASURED_COST_REL, MEASURED_R2_REL = 6.8e-15, 4.3e-14, 4.3e-16, 1.27e-10
PARITY_ROT_DEG, PARITY_TRANS_DEG = 10 * MEASURED_ROT_DEG, 10 * MEASURED_TRANS_DEG
PARITY_COST_REL = 10 * MEASURED_COST_REL                     # |cost_dev - cost_np| / cost_np
PARITY_R2_REL = 10 * MEASURED_R2_REL                         # |r^2_dev - r^2_np| / thr^2 per match: the band in which masks may differ


def _angle_deg(a, b):
    """angle between two unit vectors by the chord, 2 asin(|a - b| / 2): arccos of the dot product resolves nothing below 1e-6 deg"""
    return float(np.rad2deg(2.0 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(a - b)))))


def _rot_deg(Ra, Rb):
    """geodesic angle between two rotations by the chord |Ra - Rb|_F = 2 sqrt 2 sin(angle / 2)"""
    return float(np.rad2deg(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))))


def _cost(R, t, xa, xb, K, mask=None, thr=THR):
    xh, xh2 = PR.calibrate(xa, K), PR.calibrate(xb, K)
    return RR.truncated_cost(R, t, xh, xh2, thr, RR.usable(xh, xh2, mask))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_analytic_jacobian_matches_central_differences():
    """dr/d(w, a, b) of the restatement at a perturbed pose of a noisy scene — this pins dE/dw_k = [t]x [e_k]x R (not [e_k]x E)."""
    xa, xb = G.two_view_scene(5, N=400)[:2]
    K, R, t = PR.scene_pose(5)
    R = G.rodrigues(np.array([0.01, -0.02, 0.015])) @ R
    t = t / np.linalg.norm(t) + np.array([0.01, 0.02, -0.01])
    t /= np.linalg.norm(t)
    xh, xh2 = PR.calibrate(xa, K), PR.calibrate(xb, K)
    r, J = RR.residuals(R, t, xh, xh2, jacobian=True)
    h = 1e-6
    Jn = np.zeros_like(J)
    for k in range(5):
        d = np.zeros(5)
        d[k] = h
        Jn[:, k] = (RR.residuals(*RR.step(R, t, d), xh, xh2) - RR.residuals(*RR.step(R, t, -d), xh, xh2)) / (2 * h)
    err = np.abs(J - Jn).max()
    print(f"analytic vs central differences: max |dJ| = {err:.2e}, max |J| = {np.abs(J).max():.2e}")
    assert err < 1e-7 * max(1.0, np.abs(J).max())            # h^2 |r'''| + eps |r| / h ~ 1e-10 here
    wrong = np.stack([G.skew(e) @ G.skew(t) @ R for e in np.eye(3)])                  # [e_k]x E
    ha, hb = np.concatenate([xh, np.ones((len(xh), 1))], -1), np.concatenate([xh2, np.ones((len(xh), 1))], -1)
    dn_wrong = np.einsum("ni,kij,nj->nk", hb, wrong, ha)
    dn_right = np.einsum("ni,kij,nj->nk", hb, RR.model_matrices(R, t)[1:4], ha)
    assert np.abs(dn_wrong - dn_right).max() > 1e-3          # the two forms differ: the test above can tell them apart


def test_restatement_descends_on_a_ransac_pose():
    xa, xb, truth = G.two_view_scene(1)[:3]
    K = PR.K_SCENE
    E, emask = PR.ransac_essential(xa, xb, K, K, THR, 500, seed=3)
    R0, t0 = PR.recover_pose(E, xa, xb, K, K, emask)[:2]
    o = RR.refine(R0, t0, xa, xb, K, K, THR)
    print(f"scene 1: cost {o['costs'][0]:.6e} -> {o['cost']:.6e} in {o['steps']} kept steps, {o['count']} inliers")
    assert o["steps"] >= 1 and all(b < a for a, b in zip(o["costs"], o["costs"][1:]))
    assert o["cost"] <= o["cost0"] and o["cost"] == o["costs"][-1]
    assert _cost(o["R"], o["t"], xa, xb, K) <= _cost(R0, t0, xa, xb, K)
    assert abs(np.linalg.det(o["R"]) - 1) < 1e-12 and np.abs(o["R"].T @ o["R"] - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.norm(o["t"]) - 1) < 1e-12
    K2, R_true, t_true = PR.scene_pose(1)
    assert PR.rotation_error_deg(o["R"], R_true) <= ROT_BOUND_DEG and PR.translation_error_deg(o["t"], t_true) <= TRANS_BOUND_DEG
    # failure rules: too few weighted matches, a pose that is not finite -> the input, as it came
    few = RR.refine(R0, t0, xa, xb, K, K, THR, mask=np.arange(len(xa)) < 4)
    assert few["steps"] == 0 and np.array_equal(few["R"], R0) and np.array_equal(few["t"], t0)
    bad = RR.refine(R0 * np.nan, t0, xa, xb, K, K, THR)
    assert bad["steps"] == 0 and np.isnan(bad["R"]).all()


def test_refinement_improves_the_mean_pose_error_over_20_scenes():
    """From the truth-aware algebraic fit of the noisy matches (pose_ref.truth_aware_fit), all 5 000 matches, thr = 1.5 px / 800."""
    K = PR.K_SCENE
    rows = []
    for seed in SCENES:
        xa, xb, truth = G.two_view_scene(seed)[:3]
        _, R_true, t_true = PR.scene_pose(seed)
        R0, t0 = PR.truth_aware_fit(xa, xb, truth, K, K)
        o = RR.refine(R0, t0, xa, xb, K, K, THR)
        assert o["cost"] <= o["cost0"]
        rows.append((PR.rotation_error_deg(R0, R_true), PR.translation_error_deg(t0, t_true),
                     PR.rotation_error_deg(o["R"], R_true), PR.translation_error_deg(o["t"], t_true)))
        print(f"scene {seed}: algebraic {rows[-1][0]:.4f} / {rows[-1][1]:.4f} deg, refined {rows[-1][2]:.4f} / {rows[-1][3]:.4f} deg, "
              f"{o['steps']} steps")
    r0, t0m, r1, t1 = np.mean(rows, 0)
    print(f"mean rotation error {r0:.4f} -> {r1:.4f} deg, mean translation error {t0m:.4f} -> {t1:.4f} deg")
    assert t1 < t0m and r1 <= r0


def test_refine_pose_entry_point_validates_arguments_without_a_gpu():
    def bind(lib, a):
        def call(xa=a, R=a, out=a, P=1, N=100, thr=1e-3, iters=15):
            return lib.roma_refine_pose(xa, a, a, a, R, a, None, P, N, thr, iters, out, a, a, a, a, a, None)
        return call

    check_refine_entry_point_validates_arguments("roma_refine_pose", bind, 5, null=("xa", "R", "out"), misaligned=("xa",))


def test_new_functions_refuse_cpu_tensors():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    K = torch.eye(3, dtype=torch.float64)
    R, t = torch.eye(3, dtype=torch.float64), torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.refine_pose(R, t, x, x, K, K, 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_relative_pose(x, x, CAMERA, CAMERA, {"max_epipolar_error": 1.5})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.pose_error(R, t, torch.eye(4, dtype=torch.float64))


def test_estimate_relative_pose_rejects_unknown_options_and_cameras():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    with pytest.raises(ValueError, match="unknown key 'max_iters'"):
        geometry.estimate_relative_pose(x, x, CAMERA, CAMERA, {"max_iters": 10})
    with pytest.raises(ValueError, match="SIMPLE_RADIAL"):
        geometry.estimate_relative_pose(x, x, dict(CAMERA, model="SIMPLE_RADIAL"), CAMERA)
    with pytest.raises(ValueError, match="4 params"):
        geometry.estimate_relative_pose(x, x, CAMERA, dict(CAMERA, params=[800.0, 512.0, 384.0]))
    with pytest.raises(ValueError, match="max_epipolar_error"):
        geometry.estimate_relative_pose(x, x, CAMERA, CAMERA, {"max_epipolar_error": 0.0})
    with pytest.raises(ValueError, match="bad counts"):
        geometry.estimate_relative_pose(x, x, CAMERA, CAMERA, {"max_iterations": 0})
    # the reference's own option dict is accepted (and then stops at the CPU tensors)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_relative_pose(x, x, CAMERA, CAMERA, {"max_reproj_error": 2, "max_epipolar_error": 1, "min_inliers": 8,
                                                               "max_iterations": 10_000})
    assert abs(RR.calibrated_threshold(1.5, CAMERA, CAMERA) - THR) < 1e-18


def test_refine_kernel_uses_no_scratch_and_spills_nothing():
    """The compiler's resource report of csrc/pose_refine.hip (the recipe of test_pose.py)."""
    kernels = kernel_resources("pose_refine.hip")
    assert any("refine_pose_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _K():
    return dev(PR.K_SCENE)


def _assert_never_worse(R0, t0, R, t, xa, xb, K=PR.K_SCENE, mask=None, thr=THR):
    """the truncated cost of the returned pose, recomputed in numpy fp64, is not above that of the input pose"""
    c0, c1 = _cost(R0, t0, xa, xb, K, mask, thr), _cost(R, t, xa, xb, K, mask, thr)
    assert c1 <= c0, (c0, c1)
    return c0, c1


def _assert_pose(R, t):
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.norm(t) - 1) < 1e-12


@pytest.mark.gpu
def test_refine_parity_with_the_restatement():
    from roma_amd import geometry
    K = PR.K_SCENE
    figs, checks = [], []
    for seed in (11, 12, 13, 14):
        xa, xb = G.two_view_scene(seed)[:2]
        R0, t0, _ = geometry.estimate_pose(dev(xa), dev(xb), K, K, THR, seed=seed)
        R, t, mask, info = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, return_info=True)
        assert R.shape == (3, 3) and R.dtype == torch.float64 and t.shape == (3,) and mask.shape == (5000,) and mask.dtype == torch.bool
        R0, t0, R, t, mask = to_np(R0, t0, R, t, mask)
        o = RR.refine(R0, t0, xa, xb, K, K, THR)
        _assert_never_worse(R0, t0, R, t, xa, xb)
        _assert_pose(R, t)
        assert int(info["count"]) == int(mask.sum())
        xh, xh2 = PR.calibrate(xa, K), PR.calibrate(xb, K)
        r2d, r2n = RR.residuals(R, t, xh, xh2) ** 2, RR.residuals(o["R"], o["t"], xh, xh2) ** 2
        fig = np.array([_rot_deg(R, o["R"]), _angle_deg(t, o["t"]), abs(float(info["cost"]) - o["cost"]) / o["cost"],
                        np.abs(r2d - r2n).max() / THR ** 2])
        differ = mask != o["mask"]
        print(f"scene {seed}: device vs restatement: rotation {fig[0]:.3e} deg, translation {fig[1]:.3e} deg, cost {fig[2]:.3e} relative, "
              f"r^2 {fig[3]:.3e} thr^2; steps {int(info['steps'])} / {o['steps']}, inliers {int(info['count'])} / {o['count']}, "
              f"{int(differ.sum())} mask entries differ; the start was {_rot_deg(R0, o['R']):.4f} / {_angle_deg(t0, o['t']):.4f} deg away")
        figs.append(fig)
        band = np.abs(r2n - THR ** 2) <= PARITY_R2_REL * THR ** 2
        checks.append((seed, differ, band, int(info["count"]) - o["count"]))
    worst = np.max(figs, 0)
    print(f"largest: rotation {worst[0]:.3e} deg, translation {worst[1]:.3e} deg, cost {worst[2]:.3e}, r^2 {worst[3]:.3e} thr^2")
    assert worst[0] <= PARITY_ROT_DEG and worst[1] <= PARITY_TRANS_DEG and worst[2] <= PARITY_COST_REL and worst[3] <= PARITY_R2_REL, worst
    for seed, differ, band, dcount in checks:
        assert not (differ & ~band).any(), seed                # masks differ only where r^2 is within the tolerance of thr^2
        assert abs(dcount) <= int(band.sum()), seed


@pytest.mark.gpu
def test_estimate_relative_pose_accuracy_over_20_scenes():
    from roma_amd import geometry
    K = PR.K_SCENE
    scenes = [G.two_view_scene(s)[:2] for s in SCENES]
    rows = []
    for seed, (xa, xb) in zip(SCENES, scenes):
        _, R_true, t_true = PR.scene_pose(seed)
        R0, t0, _ = geometry.estimate_pose(dev(xa).float(), dev(xb).float(), K, K, THR, max_iters=2000, seed=seed)
        pose, info = geometry.estimate_relative_pose(dev(xa).float(), dev(xb).float(), CAMERA, CAMERA,
                                                     {"max_epipolar_error": 1.5, "max_iterations": 2000}, seed=seed)
        assert pose.Rt.shape == (3, 4) and torch.equal(pose.Rt[:, :3], pose.R) and torch.equal(pose.Rt[:, 3], pose.t)
        assert all(torch.is_tensor(info[k]) and info[k].is_cuda for k in ("inliers", "num_inliers", "model_score", "refinements"))
        assert info["iterations"] == 2000 and int(info["num_inliers"]) == int(info["inliers"].sum())
        R0, t0, R, t = to_np(R0, t0, pose.R, pose.t)
        xa32, xb32 = xa.astype(np.float32).astype(np.float64), xb.astype(np.float32).astype(np.float64)
        _assert_never_worse(R0, t0, R, t, xa32, xb32)
        _assert_pose(R, t)
        assert np.dot(t, t_true) > 0
        rows.append((PR.rotation_error_deg(R0, R_true), PR.translation_error_deg(t0, t_true), PR.rotation_error_deg(R, R_true),
                     PR.translation_error_deg(t, t_true)))
        print(f"scene {seed}: estimate_pose {rows[-1][0]:.4f} / {rows[-1][1]:.4f} deg, estimate_relative_pose {rows[-1][2]:.4f} / "
              f"{rows[-1][3]:.4f} deg (rotation / translation), {int(info['refinements'])} steps, {int(info['num_inliers'])} inliers")
        assert rows[-1][2] <= ROT_BOUND_DEG and rows[-1][3] <= TRANS_BOUND_DEG, rows[-1]
    r0, t0m, r1, t1 = np.mean(rows, 0)
    print(f"mean over {len(rows)} scenes: rotation {r0:.4f} -> {r1:.4f} deg, translation {t0m:.4f} -> {t1:.4f} deg")
    assert t1 < t0m and r1 <= r0


def _batch(first, n=8, N=2000):
    scenes = [G.two_view_scene(first + i, N=N) for i in range(n)]
    return np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])


@pytest.mark.gpu
def test_refine_determinism_and_batch_independence():
    from roma_amd import geometry
    xa, xb = _batch(20)
    K = _K()
    R0, t0, _ = geometry.estimate_pose(dev(xa), dev(xb), K, K, THR, max_iters=500, seed=5)
    o1 = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, return_info=True)
    o2 = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, return_info=True)
    assert o1[0].shape == (8, 3, 3) and o1[1].shape == (8, 3) and o1[2].shape == (8, 2000) and o1[3]["steps"].shape == (8,)
    assert all(torch.equal(a, b) for a, b in zip(o1[:3], o2[:3])) and all(torch.equal(o1[3][k], o2[3][k]) for k in o1[3])
    assert int(o1[3]["steps"].min()) >= 1
    for i in range(8):
        _assert_never_worse(*to_np(R0[i], t0[i], o1[0][i], o1[1][i]), xa[i], xb[i])
        _assert_pose(*to_np(o1[0][i], o1[1][i]))
    # pair 3 alone, and inside another batch with other intrinsics next to it
    s = geometry.refine_pose(R0[3], t0[3], dev(xa[3]), dev(xb[3]), K, K, THR, return_info=True)
    assert all(torch.equal(a, b[3]) for a, b in zip(s[:3], o1[:3])) and all(torch.equal(s[3][k], o1[3][k][3]) for k in s[3])
    xa2, xb2 = _batch(40)
    xa2[3], xb2[3] = xa[3], xb[3]
    Ks = K.expand(8, 3, 3).clone()
    Ks[5, 0, 0] = 700.0
    o3 = geometry.refine_pose(R0, t0, dev(xa2), dev(xb2), Ks, Ks, THR, return_info=True)
    assert all(torch.equal(a[3], b[3]) for a, b in zip(o1[:3], o3[:3])) and all(torch.equal(o1[3][k][3], o3[3][k][3]) for k in o1[3])
    for i in range(8):                                     # a pose of another scene: whatever happens, never worse
        _assert_never_worse(*to_np(R0[i], t0[i], o3[0][i], o3[1][i]), xa2[i], xb2[i], K=Ks[i].cpu().numpy())
    # the mask restricts the matches that carry weight
    only = torch.zeros(8, 2000, dtype=torch.bool, device=DEV)
    only[:, :1000] = True
    Rm, tm, mm = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, mask=only)
    assert not bool(mm[:, 1000:].any()) and int(mm.sum()) > 0
    Rh, th, mh = geometry.refine_pose(R0, t0, dev(xa[:, :1000]), dev(xb[:, :1000]), K, K, THR)
    assert torch.equal(Rm, Rh) and torch.equal(tm, th) and torch.equal(mm[:, :1000], mh)
    for i in range(8):
        _assert_never_worse(*to_np(R0[i], t0[i], Rm[i], tm[i]), xa[i], xb[i], mask=only[i].cpu().numpy())


@pytest.mark.gpu
def test_refining_a_refined_pose_stays_at_the_optimum():
    from roma_amd import geometry
    K = PR.K_SCENE
    for seed in (11, 12):
        xa, xb = G.two_view_scene(seed)[:2]
        R0, t0, _ = geometry.estimate_pose(dev(xa), dev(xb), K, K, THR, seed=seed)
        R1, t1, _ = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, iters=30)
        R2, t2, m2, info = geometry.refine_pose(R1, t1, dev(xa), dev(xb), K, K, THR, return_info=True)
        R1, t1, R2, t2 = to_np(R1, t1, R2, t2)
        _assert_never_worse(R1, t1, R2, t2, xa, xb)
        _assert_pose(R2, t2)
        print(f"scene {seed}: a second refinement moves the pose by {_rot_deg(R2, R1):.3e} deg / {_angle_deg(t2, t1):.3e} deg "
              f"in {int(info['steps'])} steps")
        assert _rot_deg(R2, R1) <= PARITY_ROT_DEG and _angle_deg(t2, t1) <= PARITY_TRANS_DEG
        # iters = 0 is the identity, with the pose's own mask and cost
        R3, t3, m3, i3 = geometry.refine_pose(dev(R1), dev(t1), dev(xa), dev(xb), K, K, THR, iters=0, return_info=True)
        assert np.array_equal(R3.cpu().numpy(), R1) and np.array_equal(t3.cpu().numpy(), t1) and int(i3["steps"]) == 0
        assert int(i3["count"]) == int(m3.sum())


@pytest.mark.gpu
def test_refine_of_degenerate_input_returns_the_input():
    """The guarded paths: none of them faults, each returns the pose it was given."""
    from roma_amd import geometry
    K = _K()
    xa, xb = G.two_view_scene(3, N=500)[:2]
    _, R_true, t_true = PR.scene_pose(3)
    R0, t0 = dev(R_true), dev(t_true / np.linalg.norm(t_true))
    nan = torch.full((500, 2), float("nan"), device=DEV, dtype=torch.float64)
    R, t, mask, info = geometry.refine_pose(R0, t0, nan, nan, K, K, THR, return_info=True)          # no finite match
    assert torch.equal(R, R0) and torch.equal(t, t0) and not bool(mask.any()) and int(info["steps"]) == 0 and float(info["cost"]) == 0.0
    few = torch.zeros(500, dtype=torch.bool, device=DEV)
    few[:4] = True
    R, t, mask, info = geometry.refine_pose(R0, t0, dev(xa), dev(xb), K, K, THR, mask=few, return_info=True)   # < 5 weighted matches
    assert torch.equal(R, R0) and torch.equal(t, t0) and int(mask.sum()) <= 4 and int(info["steps"]) == 0
    singular = K.clone()
    singular[1, 1] = 0.0
    Rz, tz, mz = geometry.estimate_pose(dev(xa), dev(xb), singular, K, THR, max_iters=100, seed=0)  # zero E: R = I, t = 0
    assert torch.equal(tz, torch.zeros_like(tz))
    R, t, mask, info = geometry.refine_pose(Rz, tz, dev(xa), dev(xb), singular, K, THR, return_info=True)
    assert torch.equal(R, Rz) and torch.equal(t, tz) and not bool(mask.any()) and int(info["steps"]) == 0
    R, t, mask = geometry.refine_pose(Rz, tz, dev(xa), dev(xb), K, K, THR)                        # t = 0 with a good K
    assert torch.equal(R, Rz) and torch.equal(t, tz)
    Rn = R0.clone()
    Rn[1, 1] = float("nan")
    R, t, mask = geometry.refine_pose(Rn, t0, dev(xa), dev(xb), K, K, THR)                        # a pose that is not finite
    assert torch.equal(R.isnan(), Rn.isnan()) and torch.equal(t, t0) and not bool(mask.any())
    pose, info = geometry.estimate_relative_pose(nan, nan, CAMERA, CAMERA, {"max_iterations": 100}, seed=0)
    assert torch.equal(pose.R, torch.eye(3, dtype=torch.float64, device=DEV)) and torch.equal(pose.t, torch.zeros_like(pose.t))
    assert int(info["num_inliers"]) == 0 and int(info["refinements"]) == 0
    # min_inliers above what the pair has: the RANSAC pose comes back unrefined
    Re, te, _ = geometry.estimate_pose(dev(xa), dev(xb), K, K, THR, max_iters=200, seed=1)
    cam = dict(CAMERA)
    pose, info = geometry.estimate_relative_pose(dev(xa), dev(xb), cam, cam, {"max_epipolar_error": 1.5, "max_iterations": 200,
                                                                                 "min_inliers": 501}, seed=1)
    assert torch.equal(pose.R, Re) and torch.equal(pose.t, te) and int(info["refinements"]) == 0


@pytest.mark.gpu
def test_refine_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(30, N=3000)[:2]
    xa, xb, K = dev(xa), dev(xb), _K()
    R0, t0, _ = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=11)
    eager = geometry.refine_pose(R0, t0, xa, xb, K, K, THR)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        geometry.refine_pose(R0, t0, xa, xb, K, K, THR)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = geometry.refine_pose(R0, t0, xa, xb, K, K, THR)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    _assert_never_worse(*to_np(R0, t0, out[0], out[1]), xa.cpu().numpy(), xb.cpu().numpy())
    assert PR.rotation_error_deg(out[0].cpu().numpy(), PR.scene_pose(30)[1]) < 0.5


@pytest.mark.gpu
def test_pose_error_matches_the_numpy_errors():
    from roma_amd import geometry
    rng = np.random.default_rng(0)
    Rs, ts, Tg, want = [], [], [], []
    for i in range(6):
        _, R_true, t_true = PR.scene_pose(i)
        R = G.rodrigues(rng.normal(size=3) * 0.02) @ R_true
        t = (t_true + rng.normal(size=3) * 0.05) * (1.0 if i % 2 else -1.0)       # the sign ambiguity folds
        Rs.append(R)
        ts.append(t)
        Tg.append(np.concatenate([R_true, t_true[:, None]], -1))
        want.append((PR.translation_error_deg(t, t_true), PR.rotation_error_deg(R, R_true)))
    e_t, e_R = geometry.pose_error(dev(np.stack(Rs)), dev(np.stack(ts)), np.stack(Tg))
    assert e_t.shape == (6,) and e_t.is_cuda
    assert np.abs(e_t.cpu().numpy() - [w[0] for w in want]).max() < 1e-6 and np.abs(e_R.cpu().numpy() - [w[1] for w in want]).max() < 1e-6
    e_t1, e_R1 = geometry.pose_error(dev(Rs[0]), dev(ts[0]), dev(np.vstack([Tg[0], [0, 0, 0, 1]])))
    assert abs(float(e_t1) - want[0][0]) < 1e-6 and abs(float(e_R1) - want[0][1]) < 1e-6 and want[0][0] < 90


@pytest.mark.gpu
def test_relative_pose_integration_with_match_and_sample():
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
    cam = {"model": "PINHOLE", "width": 640, "height": 480, "params": np.array([500.0, 500.0, 320.0, 240.0])}
    opt = {"max_reproj_error": 2, "max_epipolar_error": 1, "min_inliers": 8, "max_iterations": 500}
    pose, info = geometry.estimate_relative_pose(torch.stack(kA), torch.stack(kB), cam, cam, opt, seed=0)
    assert pose.R.shape == (2, 3, 3) and pose.t.shape == (2, 3) and pose.Rt.shape == (2, 3, 4) and info["inliers"].shape == (2, 500)
    assert torch.isfinite(pose.R).all() and torch.isfinite(pose.t).all() and torch.isfinite(info["model_score"]).all()
    assert (torch.linalg.det(pose.R) - 1).abs().max() < 1e-12
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    R0, t0, _ = geometry.estimate_pose(torch.stack(kA), torch.stack(kB), K, K, 1.0 / 500, max_iters=500, seed=0)
    for i in range(2):
        _assert_never_worse(*to_np(R0[i], t0[i], pose.R[i], pose.t[i]), kA[i].double().cpu().numpy(), kB[i].double().cpu().numpy(), K=K,
                            thr=1.0 / 500)
    p1, i1 = geometry.estimate_relative_pose(kA[0], kB[0], cam, cam, opt, seed=0)
    assert torch.equal(p1.R, pose.R[0]) and torch.equal(p1.t, pose.t[0]) and torch.equal(i1["inliers"], info["inliers"][0])
