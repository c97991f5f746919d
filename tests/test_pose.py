"""roma_amd.geometry, calibrated: find_essential / recover_pose / estimate_pose (csrc/essential.hip) against the numpy restatement in
tests/pose_ref.py.  CPU tests pin the restatement to ground truth, the C-ABI argument checks and the kernels' resource report; GPU
tests pin the kernels."""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import geometry_ref as G
from tests import pose_ref as PR
from tests.helpers import dev, kernel_resources

DEV = "cuda:0"
THR = 1.5 / 800                                              # 1.5 px at the scenes' focal length
ROT_BOUND_DEG, TRANS_BOUND_DEG = 0.1, 1.0                    # 5 x the worst error of the truth-aware fit over 8 scenes, rounded


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_essential_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    rc = lib.roma_essential_hypotheses(None, None, None, None, 1, 100, 10, 1e-3, 0, 0, None, 0, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_essential_hypotheses: null pointer" in lib.roma_last_error()
    rc = lib.roma_essential_select(None, None, None, None, 1, 100, 10, 1e-3, 3, None, 0, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_essential_select: null pointer" in lib.roma_last_error()
    rc = lib.roma_recover_pose(None, None, None, None, None, None, 1, 100, None, None, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_recover_pose: null pointer" in lib.roma_last_error()
    buf = (ctypes.c_double * 32)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    rc = lib.roma_essential_hypotheses(a, a, a, a, 1, 4, 10, 1e-3, 0, 0, a, big, None)             # N = 4 < 5
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 5" in lib.roma_last_error()
    rc = lib.roma_essential_select(a, a, a, a, 1, 4, 10, 1e-3, 3, a, big, a, a, None)
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 5" in lib.roma_last_error()
    rc = lib.roma_recover_pose(a, a, a, a, a, None, 1, 4, a, a, a, a, None)
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 5" in lib.roma_last_error()
    rc = lib.roma_essential_hypotheses(a, a, a, a, 0, 100, 10, 1e-3, 0, 0, a, big, None)           # P = 0
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    rc = lib.roma_recover_pose(a, a, a, a, a, None, 0, 100, a, a, a, a, None)
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    rc = lib.roma_essential_hypotheses(a, a, a, a, 1, 100, 0, 1e-3, 0, 0, a, big, None)            # iters = 0
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    need = lib.roma_essential_workspace(1, 100, 10, None)
    assert need > 0
    off = (ctypes.c_long * 10)()
    assert lib.roma_essential_workspace(1, 100, 10, ctypes.cast(off, ctypes.c_void_p)) == need
    assert list(off) == sorted(off) and off[0] == 0 and off[9] + 100 * 32 <= need
    rc = lib.roma_essential_hypotheses(a, a, a, a, 1, 100, 10, 1e-3, 0, 0, a, need - 1, None)      # workspace too small
    assert rc == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    rc = lib.roma_essential_select(a, a, a, a, 1, 100, 10, 1e-3, 3, a, need - 1, a, a, None)
    assert rc == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    for thr in (0.0, -1.0):                                                                        # threshold <= 0
        rc = lib.roma_essential_hypotheses(a, a, a, a, 1, 100, 10, thr, 0, 0, a, need, None)
        assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
        rc = lib.roma_essential_select(a, a, a, a, 1, 100, 10, thr, 3, a, need, a, a, None)
        assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    assert lib.roma_essential_workspace(0, 100, 10, None) < 0


def test_scene_pose_is_the_pose_of_two_view_scene():
    for seed in (0, 1, 11, 14):
        K, R, t = PR.scene_pose(seed)
        F = G.two_view_scene(seed, N=50)[3]
        Ki = np.linalg.inv(K)
        assert np.abs(G.sign_fixed(Ki.T @ G.skew(t) @ R @ Ki) - F).max() < 1e-15


def test_numpy_five_point_recovers_the_true_e_on_exact_data():
    for seed in range(5):
        K, R, t = PR.scene_pose(seed)
        _, _, _, _, ca, cb = G.two_view_scene(seed, outlier_frac=0.0, sigma=0.0)
        xh, xh2 = PR.calibrate(ca, K), PR.calibrate(cb, K)
        models, w, cond = PR.five_point(xh[:5], xh2[:5])
        assert 1 <= len(models) <= 10
        ha, hb = np.concatenate([xh[:5], np.ones((5, 1))], -1), np.concatenate([xh2[:5], np.ones((5, 1))], -1)
        for m in models:                                  # unit norm: |E|^3 = 1
            assert abs(np.linalg.norm(m) - 1) < 1e-12
            assert np.abs(np.einsum("ni,ij,nj->n", hb, m, ha)).max() < 1e-9
            assert abs(np.linalg.det(m)) < 1e-9
            assert np.abs(2 * m @ m.T @ m - np.trace(m @ m.T) * m).max() < 1e-9
        E = PR.essential_from_pose(R, t)
        errs = [np.abs(G.sign_fixed(m) - E).max() for m in models]
        assert min(errs) < 1e-7, errs
        Rr, tr, mask, count = PR.recover_pose(E, ca, cb, K, K)
        assert np.abs(Rr - R).max() < 1e-9 and np.abs(tr - t / np.linalg.norm(t)).max() < 1e-9
        assert mask.all() and count == len(ca)


def _check_pose_scene(seed, E, emask, R, t, mask, truth, what):
    """the scene criteria: E mask, rotation matrix, narrowed mask, pose accuracy (bounds: module header)"""
    K, R_true, t_true = PR.scene_pose(seed)
    rec, prec = G.recall_precision(emask, truth)
    assert rec >= 0.98 and prec >= 0.98, (rec, prec)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.norm(t) - 1) < 1e-12
    assert not (mask & ~emask).any()
    assert (mask & truth).sum() >= 0.98 * truth.sum(), ((mask & truth).sum(), truth.sum())
    er, et = PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)
    print(f"{what}, scene {seed}: rotation error {er:.4f} deg, translation error {et:.4f} deg, E mask recall {rec:.4f} precision "
          f"{prec:.4f}, {int(mask.sum())} of {int(emask.sum())} pass cheirality")
    assert er <= ROT_BOUND_DEG and et <= TRANS_BOUND_DEG, (er, et)
    assert np.dot(t, t_true) > 0                             # the cheirality vote picks the sign, not only the axis


def _print_truth_aware(seed, xa, xb, truth):
    K, R_true, t_true = PR.scene_pose(seed)
    R, t = PR.truth_aware_fit(xa, xb, truth, K, K)
    print(f"truth-aware fit, scene {seed}: rotation error {PR.rotation_error_deg(R, R_true):.4f} deg, translation error "
          f"{PR.translation_error_deg(t, t_true):.4f} deg")


def test_numpy_restatement_meets_the_pose_criteria():
    xa, xb, truth = G.two_view_scene(1)[:3]
    K = PR.K_SCENE
    E, emask = PR.ransac_essential(xa, xb, K, K, THR, 500, seed=3)
    s = np.linalg.svd(E, compute_uv=False)
    assert abs(s[0] - s[1]) / s[0] < 1e-9 and s[2] / s[0] < 1e-12
    R, t, mask, count = PR.recover_pose(E, xa, xb, K, K, emask)
    assert count == mask.sum()
    _print_truth_aware(1, xa, xb, truth)
    _check_pose_scene(1, E, emask, R, t, mask, truth, "restatement")


def test_pose_functions_refuse_cpu_tensors_and_too_few_matches():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    K = torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_essential(x, x, K, K, 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.recover_pose(torch.eye(3, dtype=torch.float64), x, x, K, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_pose(x, x, K, K, 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_pose_uncalibrated(x, x, K, K, 1.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.score_hypotheses(x, x, "essential", 1e-3, 10, 0, K, K)
    assert geometry.estimate_pose(x[:4], x[:4], K, K, 1e-3) is None
    assert geometry.estimate_pose_uncalibrated(x[:4], x[:4], K, K, 1.5) is None


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """The compiler's resource report of csrc/essential.hip (what tools/kres.sh wraps): the 5-point solver is spread over 32 lanes
    so that no kernel needs scratch memory or spills a register."""
    kernels = kernel_resources("essential.hip")
    for want in ("calibrate_kernel", "five_point_kernel", "essential_select_kernel", "recover_pose_kernel", "score_kernel",
                 "reduce_kernel"):
        assert any(want in k for k in kernels), (want, sorted(kernels))
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _K():
    return dev(PR.K_SCENE)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 6, 5000])
def test_essential_sample_indices_equal_the_restatement(N):
    from roma_amd import geometry
    rng = np.random.default_rng(N)
    xa, xb = rng.uniform(0, 1000, (3, N, 2)), rng.uniform(0, 1000, (3, N, 2))
    if N == 5000:
        xa[1, 17] = np.nan                                # a non-finite match is never drawn
    for seed in (0, 123456789):
        got = geometry.minimal_samples(dev(xa), dev(xb), "essential", max_iters=300, seed=seed, K_A=_K(), K_B=_K()).cpu().numpy()
        want = PR.minimal_samples(xa, xb, 300, seed)
        assert got.shape == (3, 300, 5) and np.array_equal(got, want), seed
    if N == 5:
        got = got.reshape(-1, 5)
        assert (got[:, 0] >= 0).mean() > 0.6 and all(sorted(r) == list(range(5)) for r in got if r[0] >= 0)
    if N == 5000:
        assert not (got[1] == 17).any()


@pytest.mark.gpu
def test_five_point_models_match_numpy_fp64():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(5, N=600, outlier_frac=0.3)[:2]
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "essential", THR, max_iters=400, seed=7, K_A=_K(), K_B=_K())
    assert np.abs(r["T_A"][0].cpu().numpy() - np.linalg.inv(PR.K_SCENE)).max() < 1e-15
    xh, xh2 = PR.calibrate(xa, PR.K_SCENE), PR.calibrate(xb, PR.K_SCENE)
    models, valid, samples = r["models"][0].cpu().numpy(), r["valid"][0].cpu().numpy(), r["samples"][0].cpu().numpy()
    assert models.shape == (400, 10, 3, 3) and np.array_equal(samples, PR.minimal_samples(xa[None], xb[None], 400, 7)[0])
    usable, skipped, checked, worst = 0, 0, 0, 0.0
    for h in range(400):
        if samples[h, 0] < 0:
            assert not valid[h].any()
            continue
        usable += 1
        want, w, cond = PR.five_point(xh[samples[h]], xh2[samples[h]])
        if not PR.well_conditioned(w, cond):
            skipped += 1
            continue
        assert valid[h].sum() == len(want), (h, valid[h], len(want))          # no root lost, none invented
        assert valid[h, :len(want)].all()                                     # valid slots first
        for s in range(10):
            if valid[h, s]:
                d = min(np.abs(G.sign_fixed(models[h, s]) - G.sign_fixed(m)).max() for m in want)
                worst = max(worst, d)
                assert d < 1e-6, (h, s, d)
                checked += 1
            else:
                assert not models[h, s].any()
    print(f"5-point vs numpy: {checked} slots of {usable - skipped} samples compared, worst max-abs difference {worst:.2e}; "
          f"{skipped} of {usable} valid samples left out as ill-conditioned")
    assert skipped <= 0.05 * usable, (skipped, usable)
    assert checked > 1000, checked


def _msac(E, xh, xh2, t2):
    e = G.errors("fundamental", E, xh, xh2)
    return np.where(e < t2, e, t2).sum()


@pytest.mark.gpu
def test_essential_inlier_counts_equal_an_fp64_recount():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(6, N=3000)[:2]
    xa[17] = np.nan
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "essential", THR, max_iters=100, seed=9, K_A=_K(), K_B=_K())
    xh, xh2 = PR.calibrate(xa, PR.K_SCENE), PR.calibrate(xb, PR.K_SCENE)
    models, valid, count = r["models"][0].cpu().numpy(), r["valid"][0].cpu().numpy(), r["count"][0].cpu().numpy()
    assert valid.sum() > 200
    t2 = THR * THR
    for h, s in zip(*np.nonzero(valid)):
        e = G.errors("fundamental", models[h, s], xh, xh2)
        lo, hi = (e < t2 * (1 - 1e-3)).sum(), (e < t2 * (1 + 1e-3)).sum()
        assert lo <= count[h, s] <= hi, (h, s, lo, count[h, s], hi)
    assert (count[~valid] == 0).all() and np.isinf(r["cost"][0].cpu().numpy()[~valid]).all()


@pytest.mark.gpu
def test_essential_selection_and_local_optimisation():
    """lo_iters = 0 returns the lowest-cost slot of score_hypotheses (lowest slot on ties, as np.argmin); lo_iters = 3 returns a model
    of strictly lower MSAC cost (fp64 recount); both lie on the essential manifold."""
    from roma_amd import geometry
    xa, xb = G.two_view_scene(13)[:2]
    xh, xh2 = PR.calibrate(xa, PR.K_SCENE), PR.calibrate(xb, PR.K_SCENE)
    r = geometry.score_hypotheses(dev(xa), dev(xb), "essential", THR, max_iters=500, seed=21, K_A=_K(), K_B=_K())
    best = int(np.argmin(r["cost"][0].cpu().numpy().reshape(-1)))
    want = G.sign_fixed(r["models"][0].cpu().numpy().reshape(-1, 3, 3)[best])
    E0, mask0 = geometry.find_essential(dev(xa), dev(xb), _K(), _K(), THR, max_iters=500, seed=21, lo_iters=0)
    E0 = E0.cpu().numpy()
    assert np.abs(E0 - want).max() <= 1e-9, (E0, want)
    E3, mask3 = geometry.find_essential(dev(xa), dev(xb), _K(), _K(), THR, max_iters=500, seed=21, lo_iters=3)
    E3 = E3.cpu().numpy()
    t2 = THR * THR
    assert _msac(E3, xh, xh2, t2) < _msac(E0, xh, xh2, t2), (_msac(E3, xh, xh2, t2), _msac(E0, xh, xh2, t2))
    for E in (E0, E3):
        s = np.linalg.svd(E, compute_uv=False)
        assert abs(np.linalg.norm(E) - 1) < 1e-12 and abs(s[0] - s[1]) / s[0] < 1e-9 and s[2] / s[0] < 1e-12, s
        assert E.reshape(-1)[np.abs(E).argmax()] > 0
    e = G.errors("fundamental", E3, xh, xh2)
    m = mask3.cpu().numpy()
    assert ((e < t2 * (1 - 1e-3)) <= m).all() and (m <= (e < t2 * (1 + 1e-3))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_pose_scene(seed):
    from roma_amd import geometry
    xa, xb, truth = G.two_view_scene(seed)[:3]
    K = PR.K_SCENE
    E, emask = geometry.find_essential(dev(xa).float(), dev(xb).float(), K, K, THR, seed=seed)
    out = geometry.estimate_pose(dev(xa).float(), dev(xb).float(), K, K, THR, seed=seed)
    R, t, mask = out
    assert R.shape == (3, 3) and R.dtype == torch.float64 and t.shape == (3,) and mask.shape == (5000,) and mask.dtype == torch.bool
    _print_truth_aware(seed, xa, xb, truth)
    _check_pose_scene(seed, E.cpu().numpy(), emask.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy(), truth, "device")


def _clean_scene(seed, sign, N=2000, outlier_frac=0.25):
    """depths 4-12, baseline 1, exact projections; `sign` = -1 puts camera B on the other side.  xa, xb, truth, R, t (unit)."""
    rng = np.random.default_rng(seed)
    K = PR.K_SCENE
    R = G.rodrigues(rng.normal(size=3) * 0.08)
    t = sign * np.array([1.0, 0.1 * rng.normal(), 0.1 * rng.normal()])
    t /= np.linalg.norm(t)
    u = np.stack([rng.uniform(0, G.W_IMG, N), rng.uniform(0, G.H_IMG, N)], -1)
    X = (np.concatenate([u, np.ones((N, 1))], -1) @ np.linalg.inv(K).T) * rng.uniform(4, 12, N)[:, None]
    Xb = X @ R.T + t
    ub = (Xb @ K.T)[:, :2] / (Xb @ K.T)[:, 2:3]
    truth = rng.uniform(size=N) >= outlier_frac
    ub[~truth] = np.stack([rng.uniform(0, G.W_IMG, N), rng.uniform(0, G.H_IMG, N)], -1)[~truth]
    return u, ub, truth, R, t


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("esign", [1.0, -1.0])
def test_recover_pose_picks_the_true_candidate(sign, esign):
    """The true pose against its twisted twin and both translation signs, from E and from -E: the vote finds it, and its count and
    narrowed mask equal the restatement's exactly (no masked match has a depth near zero under any candidate)."""
    from roma_amd import geometry
    K = PR.K_SCENE
    for seed in (0, 1):
        xa, xb, truth, R_true, t_true = _clean_scene(seed, sign)
        E = esign * 0.37 * G.skew(t_true) @ R_true
        xh, xh2 = PR.calibrate(xa, K), PR.calibrate(xb, K)
        for Rc, tc in PR.decompose(E):
            la, lb = PR.depths(Rc, tc, xh[truth], xh2[truth])
            assert np.isfinite(la).all() and np.isfinite(lb).all() and min(np.abs(la).min(), np.abs(lb).min()) > 1e-6
        Rw, tw, mw, cw = PR.recover_pose(E, xa, xb, K, K, truth)
        assert cw == truth.sum() and np.abs(Rw - R_true).max() < 1e-9 and np.abs(tw - t_true).max() < 1e-9
        R, t, mask = geometry.recover_pose(dev(E), dev(xa), dev(xb), K, K, dev(truth))
        assert np.abs(R.cpu().numpy() - R_true).max() < 1e-9 and np.abs(t.cpu().numpy() - t_true).max() < 1e-9
        assert np.array_equal(mask.cpu().numpy(), mw) and int(mask.sum()) == cw
        # without a mask every match votes: the outliers' votes are whatever their depths say, the same on both sides
        Rw, tw, mw, cw = PR.recover_pose(E, xa, xb, K, K)
        R, t, mask = geometry.recover_pose(dev(E), dev(xa), dev(xb), _K(), _K())
        assert np.abs(R.cpu().numpy() - Rw).max() < 1e-9 and np.abs(t.cpu().numpy() - tw).max() < 1e-9
        assert (mask.cpu().numpy() != mw).sum() <= 2 and abs(int(mask.sum()) - cw) <= 2       # outliers may sit at a zero depth


@pytest.mark.gpu
def test_pose_determinism_and_batch_independence():
    from roma_amd import geometry
    scenes = [G.two_view_scene(20 + i, N=2000) for i in range(8)]
    xa = dev(np.stack([s[0] for s in scenes])).float()
    xb = dev(np.stack([s[1] for s in scenes])).float()
    K = _K()
    o1 = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=5)
    o2 = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=5)
    assert o1[0].shape == (8, 3, 3) and o1[1].shape == (8, 3) and o1[2].shape == (8, 2000)
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    E1, m1 = geometry.find_essential(xa, xb, K, K, THR, max_iters=500, seed=5)
    other = [G.two_view_scene(40 + i, N=2000) for i in range(8)]
    xa2, xb2 = xa.clone(), xb.clone()
    for i in range(8):
        if i != 3:
            xa2[i], xb2[i] = dev(other[i][0]).float(), dev(other[i][1]).float()
    Ks = K.expand(8, 3, 3).clone()
    Ks[5, 0, 0] = 700.0                                   # per-pair intrinsics: another pair's K does not matter either
    E3, m3 = geometry.find_essential(xa2, xb2, Ks, Ks, THR, max_iters=500, seed=5)
    o3 = geometry.estimate_pose(xa2, xb2, Ks, Ks, THR, max_iters=500, seed=5)
    assert torch.equal(E3[3], E1[3]) and torch.equal(m3[3], m1[3])
    assert all(torch.equal(a[3], b[3]) for a, b in zip(o1, o3))
    for i in range(8):                                    # and the batch does what it should
        R_true = PR.scene_pose(20 + i)[1]
        assert PR.rotation_error_deg(o1[0][i].cpu().numpy(), R_true) < 0.5


@pytest.mark.gpu
def test_pose_of_degenerate_input_is_the_identity():
    from roma_amd import geometry
    K = _K()
    eye, zero = torch.eye(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    xa, xb = G.two_view_scene(3, N=500)[:2]
    singular = K.clone()
    singular[1, 1] = 0.0
    cases = [(torch.full((500, 2), 123.5, device=DEV), torch.full((500, 2), 123.5, device=DEV), K),
             (torch.full((500, 2), float("nan"), device=DEV), torch.full((500, 2), float("nan"), device=DEV), K),
             (dev(xa), dev(xb), singular)]
    for a, b, k in cases:
        E, emask = geometry.find_essential(a, b, k, K, THR, max_iters=100, seed=0)
        assert torch.equal(E, torch.zeros_like(E)) and not bool(emask.any())
        R, t, mask = geometry.estimate_pose(a, b, k, K, THR, max_iters=100, seed=0)
        assert torch.equal(R, eye) and torch.equal(t, zero) and not bool(mask.any())
    r = geometry.score_hypotheses(dev(xa), dev(xb), "essential", THR, 100, 0, singular, K)
    assert not bool(r["valid"].any()) and bool((r["samples"] == -1).all())


@pytest.mark.gpu
def test_pose_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(30, N=3000)[:2]
    xa, xb, K = dev(xa).float(), dev(xb).float(), _K()
    eager = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=11)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=11)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=500, seed=11)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert PR.rotation_error_deg(out[0].cpu().numpy(), PR.scene_pose(30)[1]) < 0.5


@pytest.mark.gpu
def test_estimate_pose_uncalibrated_is_find_fundamental_then_recover_pose():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(31, N=3000)[:2]
    xa, xb, K = dev(xa).float(), dev(xb).float(), _K()
    R, t, mask = geometry.estimate_pose_uncalibrated(xa, xb, K, K, 1.5, max_iters=2000, seed=17)
    F, fmask = geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=2000, seed=17)
    R2, t2, mask2 = geometry.recover_pose(K.transpose(-1, -2) @ F @ K, xa, xb, K, K, fmask)
    assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(mask, mask2)
    assert abs(float(torch.linalg.det(R)) - 1) < 1e-12 and not bool((mask & ~fmask).any()) and int(mask.sum()) > 1000


@pytest.mark.gpu
def test_megadepth_pose_batch_fits_in_256_mb():
    """P = 64 pairs of N = 10 000 matches, 2 000 samples (20 000 slots) each, in one estimate_pose call."""
    from roma_amd import geometry
    g = torch.Generator().manual_seed(0)
    xa = (torch.rand(64, 10000, 2, generator=g) * 1000).to(DEV)
    xb = (torch.rand(64, 10000, 2, generator=g) * 1000).to(DEV)
    K = _K()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    R, t, mask = geometry.estimate_pose(xa, xb, K, K, THR, max_iters=2000, seed=0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"P = 64, N = 10 000, 2 000 samples: peak {peak / 1e6:.1f} MB above the inputs")
    assert peak < 256e6, peak
    assert R.shape == (64, 3, 3) and t.shape == (64, 3) and mask.shape == (64, 10000) and torch.isfinite(R).all()


@pytest.mark.gpu
def test_pose_integration_with_match_and_sample():
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
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    R, t, mask = geometry.estimate_pose(torch.stack(kA), torch.stack(kB), K, K, 1.0 / 500, max_iters=500, seed=0)
    assert R.shape == (2, 3, 3) and t.shape == (2, 3) and mask.shape == (2, 500)
    assert torch.isfinite(R).all() and torch.isfinite(t).all()
    assert (torch.linalg.det(R) - 1).abs().max() < 1e-12
    R1, t1, mask1 = geometry.estimate_pose(kA[0], kB[0], K, K, 1.0 / 500, max_iters=500, seed=0)
    assert torch.equal(R1, R[0]) and torch.equal(t1, t[0]) and torch.equal(mask1, mask[0])
