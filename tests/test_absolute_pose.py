"""roma_amd.geometry, absolute pose: find_absolute_pose / refine_absolute_pose / estimate_absolute_pose / lift_keypoints
(csrc/absolute_pose.hip) against the numpy restatement in tests/absolute_pose_ref.py.  CPU tests pin the restatement to ground truth,
the C-ABI argument checks, the Python surface and the kernels' resource report; GPU tests pin the kernels.

Scenes: absolute_pose_ref.scene — cameras and motions of tests/general_scenes.py, N = 2000, 30 % outliers, sigma = 0.5 px, |t| = 1.5;
threshold 2.0 px (4 sigma).

Measured with the restatement (the CPU tests print the figures again):
  SLOT_BOUND       P3P on exact data, 200 samples per motion: every accepted sample has a slot at the true pose, worst max-abs
                   deviation of (R, t) 1.0e-12, no sample rejected; the bound is 10 x that
  ROT_BOUND_DEG,   5 x the worst error of the truth-aware fit (LM on the true inliers from the true pose) over 4 motions x 5 seeds:
  CENTRE_BOUND     0.0115 deg and 0.00149 world units, rounded up
  REFINE_TOL       the refinement from the truth moved by 0.5 deg and 0.05 units, summed over the matches in their order, in reverse
                   and in a shuffled order: the poses differ by at most 8.9e-16 (max-abs over R and t, 4 motions); 10 x that
  CHAIN_*          views A, B, C: the restatement on the points triangulated under the truth-aware two-view pose recovers C's
                   centre to 0.00135 baselines and its rotation to 0.0218 deg; 5 x, rounded up
"""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import absolute_pose_ref as A
from tests import general_scenes as GS
from tests import geometry_ref as G
from tests import pose_ref as PR
from tests import triangulate_ref as TR
from tests.helpers import dev, kernel_resources

K = GS.K_B
THR = 2.0
SLOT_BOUND = 1e-11
ROT_BOUND_DEG, CENTRE_BOUND = 0.06, 0.008
REFINE_TOL = 8.9e-15
CHAIN_CENTRE_BOUND, CHAIN_ROT_BOUND_DEG = 0.007, 0.11
MOTIONS = tuple(GS.MOTIONS)
PERTURB_W = np.radians(0.5) * np.array([0.6, -0.48, 0.64])
PERTURB_T = 0.05 * np.array([0.48, 0.6, -0.64])
CAMERA = {"model": "PINHOLE", "params": [610.0, 655.0, 390.0, 310.0]}


def _check_scene(R, t, mask, truth, R_true, t_true, what, X=None, x=None):
    """the scene criteria: mask against the truth, rotation matrix, pose within the bounds, no inlier behind the camera"""
    rec, prec = G.recall_precision(mask, truth)
    er, ec = A.rotation_error_deg(R, R_true), A.centre_error(R, t, R_true, t_true)
    print(f"{what}: rotation error {er:.4f} deg, centre error {ec:.5f}, recall {rec:.4f}, precision {prec:.4f}")
    assert rec >= 0.98 and prec >= 0.98, (rec, prec)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND, (er, ec)
    if X is not None:
        with np.errstate(invalid="ignore"):
            assert not (mask & ~((X @ R.T + t)[:, 2] > 0)).any()


def _print_truth_aware(X, x, truth, R_true, t_true, what):
    R, t = A.truth_aware_fit(X, x, truth, K, R_true, t_true)
    print(f"truth-aware fit, {what}: rotation error {A.rotation_error_deg(R, R_true):.4f} deg, centre error "
          f"{A.centre_error(R, t, R_true, t_true):.5f}")


def _perturbed(R, t):
    return A.exp_so3(PERTURB_W) @ R, t + PERTURB_T


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_absolute_pose_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    rc = lib.roma_absolute_pose_hypotheses(None, None, None, 1, 100, 10, 2.0, 0, 0, 0, None, 0, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_absolute_pose_hypotheses: null pointer" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_select(None, None, None, 1, 100, 10, 2.0, 0, 3, None, 0, None, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_absolute_pose_select: null pointer" in lib.roma_last_error()
    rc = lib.roma_refine_absolute_pose(None, None, None, None, None, None, 1, 100, 2.0, 15, None, None, None, None, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_refine_absolute_pose: null pointer" in lib.roma_last_error()
    buf = (ctypes.c_double * 32)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 2, 10, 2.0, 0, 0, 0, a, big, None)               # N = 2 < 3
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 3" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_select(a, a, a, 1, 2, 10, 2.0, 0, 3, a, big, a, a, a, None)
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 3" in lib.roma_last_error()
    rc = lib.roma_refine_absolute_pose(a, a, a, a, a, None, 1, 3, 2.0, 15, a, a, a, a, a, a, None)      # the refinement needs 4
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 4" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_hypotheses(a, a, a, 0, 100, 10, 2.0, 0, 0, 0, a, big, None)             # P = 0
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    rc = lib.roma_refine_absolute_pose(a, a, a, a, a, None, 0, 100, 2.0, 15, a, a, a, a, a, a, None)
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 100, 0, 2.0, 0, 0, 0, a, big, None)              # iters = 0
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    need = lib.roma_absolute_pose_workspace(1, 100, 10, None)
    assert need > 0
    off = (ctypes.c_long * 12)()
    assert lib.roma_absolute_pose_workspace(1, 100, 10, ctypes.cast(off, ctypes.c_void_p)) == need
    assert list(off) == sorted(off) and off[0] == 0 and len(set(off)) == 12 and off[11] + 100 * 40 <= need
    rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 100, 10, 2.0, 0, 0, 0, a, need - 1, None)        # workspace too small
    assert rc == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_select(a, a, a, 1, 100, 10, 2.0, 0, 3, a, need - 1, a, a, a, None)
    assert rc == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    for thr in (0.0, -1.0):                                                                             # threshold <= 0
        rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 100, 10, thr, 0, 0, 0, a, need, None)
        assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
        rc = lib.roma_absolute_pose_select(a, a, a, 1, 100, 10, thr, 0, 3, a, need, a, a, a, None)
        assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
        rc = lib.roma_refine_absolute_pose(a, a, a, a, a, None, 1, 100, thr, 15, a, a, a, a, a, a, None)
        assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    for scoring in (-1, 2):                                                                             # a bad scoring code
        rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 100, 10, 2.0, scoring, 0, 0, a, need, None)
        assert rc == _lib.ROMA_E_ARG and b"scoring" in lib.roma_last_error()
        rc = lib.roma_absolute_pose_select(a, a, a, 1, 100, 10, 2.0, scoring, 3, a, need, a, a, a, None)
        assert rc == _lib.ROMA_E_ARG and b"scoring" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_hypotheses(a, a, a, 1, 100, 10, 2.0, 0, 0, -1, a, need, None)           # a negative pair offset
    assert rc == _lib.ROMA_E_ARG and b"pair offset" in lib.roma_last_error()
    rc = lib.roma_absolute_pose_select(a, a, a, 1, 100, 10, 2.0, 0, -1, a, need, a, a, a, None)
    assert rc == _lib.ROMA_E_ARG and b"lo_iters" in lib.roma_last_error()
    rc = lib.roma_refine_absolute_pose(a, a, a, a, a, None, 1, 100, 2.0, -1, a, a, a, a, a, a, None)
    assert rc == _lib.ROMA_E_ARG and b"iters" in lib.roma_last_error()
    assert lib.roma_absolute_pose_workspace(0, 100, 10, None) < 0
    assert lib.roma_abi_version() == 5                                                                  # additive: the ABI stays


def test_numpy_p3p_recovers_the_true_pose_on_exact_data():
    worst, rejected, total = 0.0, 0, 0
    for motion in MOTIONS:
        X, x, _, R, t = A.scene(motion, 0, N=400, outlier_frac=0.0, sigma=0.0)
        idx, hyp = A.hypotheses(X, x, K, 200, seed=1)
        assert (idx >= 0).all()
        for sols in hyp:
            total += 1
            if not sols:
                rejected += 1
                continue
            assert len(sols) <= A.SLOTS
            worst = max(worst, min(max(np.abs(Rs - R).max(), np.abs(ts - t).max()) for Rs, ts in sols))
    print(f"P3P on exact data: worst deviation of the closest slot from the truth {worst:.2e} over {total - rejected} samples, "
          f"{rejected} of {total} rejected; bound {SLOT_BOUND:.0e}")
    assert worst <= SLOT_BOUND, worst
    assert rejected <= 0.02 * total, (rejected, total)


@pytest.mark.parametrize("motion", MOTIONS)
def test_numpy_restatement_meets_the_scene_criteria(motion):
    X, x, truth, R_true, t_true = A.scene(motion, 0)
    R, t, mask = A.ransac(X, x, K, THR, 500, seed=0)
    _check_scene(R, t, mask, truth, R_true, t_true, f"restatement RANSAC, {motion}", X, x)
    r = A.refine(R, t, X, x, K, THR)
    _print_truth_aware(X, x, truth, R_true, t_true, motion)
    _check_scene(r["R"], r["t"], r["mask"], truth, R_true, t_true, f"restatement RANSAC + refinement, {motion}", X, x)
    assert r["cost"] <= r["cost0"]


def test_truth_aware_bounds_are_five_times_the_worst_fit():
    """the figures of the module header, measured again: the bounds are 5 x the worst truth-aware error over 20 scenes, rounded up;
    the world offset moves the fit by less than 1e-3 deg"""
    wr = wc = 0.0
    for motion in MOTIONS:
        for seed in range(5):
            X, x, truth, R_true, t_true = A.scene(motion, seed)
            R, t = A.truth_aware_fit(X, x, truth, K, R_true, t_true)
            wr, wc = max(wr, A.rotation_error_deg(R, R_true)), max(wc, A.centre_error(R, t, R_true, t_true))
            if seed == 0:
                Ro, _ = A.truth_aware_fit(X + A.OFFSET, x, truth, K, R_true, t_true - R_true @ A.OFFSET)
                assert abs(A.rotation_error_deg(Ro, R_true) - A.rotation_error_deg(R, R_true)) < 1e-3
    print(f"truth-aware fit over 20 scenes: worst rotation error {wr:.4f} deg, worst centre error {wc:.5f}")
    assert 5 * wr <= ROT_BOUND_DEG <= 6 * wr and 5 * wc <= CENTRE_BOUND <= 6 * wc, (wr, wc)


def test_refinement_tolerance_is_ten_times_the_order_of_the_sums():
    worst = 0.0
    for motion in MOTIONS:
        X, x, _, R_true, t_true = A.scene(motion, 0)
        R0, t0 = _perturbed(R_true, t_true)
        r = [A.refine(R0, t0, X, x, K, THR, order=o) for o in (0, 1, 2)]
        assert all(q["steps"] >= 1 for q in r)
        worst = max([worst] + [max(np.abs(q["R"] - r[0]["R"]).max(), np.abs(q["t"] - r[0]["t"]).max()) for q in r[1:]])
    print(f"refinement, three orders of the sums: poses differ by at most {worst:.2e}; tolerance {REFINE_TOL:.1e}")
    assert 0 < 10 * worst <= REFINE_TOL * 1.0001, worst


def test_absolute_pose_surface_validates_without_a_gpu():
    from roma_amd import geometry
    x, X = torch.rand(100, 2) * 500, torch.rand(100, 3)
    Kt = torch.eye(3, dtype=torch.float64)
    I, z = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_absolute_pose(X, x, Kt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.refine_absolute_pose(I, z, X, x, Kt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.estimate_absolute_pose(x, X, CAMERA)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.absolute_pose_hypotheses(X, x, Kt, 2.0, 10, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.absolute_pose_error(I, z, torch.eye(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.lift_keypoints(x, torch.rand(600, 600), Kt)
    with pytest.raises(ValueError, match="needs 3"):                             # below the minimal sample
        geometry.find_absolute_pose(X[:2], x[:2], Kt)
    with pytest.raises(ValueError, match="needs 3"):
        geometry.estimate_absolute_pose(x[:2], X[:2], CAMERA)
    with pytest.raises(ValueError, match="unknown key"):
        geometry.estimate_absolute_pose(x, X, CAMERA, {"max_epipolar_error": 1.0})
    with pytest.raises(ValueError, match="PINHOLE"):
        geometry.estimate_absolute_pose(x, X, {"model": "SIMPLE_RADIAL", "params": [600.0, 320.0, 240.0, 0.1]})
    with pytest.raises(ValueError, match="max_reproj_error"):
        geometry.estimate_absolute_pose(x, X, CAMERA, {"max_reproj_error": 0.0})
    # refine_iters and scoring are checked before any tensor is examined: the CPU tensors are never reached
    with pytest.raises(ValueError, match="scoring"):
        geometry.find_absolute_pose(X, x, Kt, scoring="ransac")
    with pytest.raises(ValueError, match="refine_iters"):
        geometry.find_absolute_pose(X, x, Kt, refine_iters=-1)
    with pytest.raises(TypeError, match="refine_iters"):
        geometry.find_absolute_pose(X, x, Kt, 2.0, 1000, None, 3, "magsac")
    with pytest.raises(ValueError, match="scoring"):
        geometry.estimate_absolute_pose(x, X, CAMERA, scoring="ransac")
    with pytest.raises(ValueError, match="scoring"):
        geometry.absolute_pose_hypotheses(X, x, Kt, scoring="ransac")
    assert geometry.CameraPose is geometry.RelativePose
    # estimate_relative_pose still ignores max_reproj_error and still knows nothing of the new defaults
    assert geometry._RANSAC_OPT["max_reproj_error"] is None and geometry._AP_RANSAC_OPT["max_reproj_error"] == 12.0


def test_absolute_pose_kernels_resource_report():
    res = kernel_resources("absolute_pose.hip")
    seen = set()
    for name, r in res.items():
        for key in ("ap_score_kernel", "p3p_kernel", "ap_select_kernel", "refine_absolute_pose_kernel"):
            if key in name:
                seen.add(key)
                print(f"{key} ({name[-12:]}): VGPRs {r['VGPRs']}, AGPRs {r.get('AGPRs', 0)}, scratch {r['ScratchSize']} bytes")
                if key == "ap_score_kernel":
                    assert r["ScratchSize"] == 0, (name, r)
    assert len(seen) == 4, seen
    assert sum("ap_score_kernel" in n for n in res) == 2 and sum("ap_select_kernel" in n for n in res) == 2      # MSAC and MAGSAC++


# ------------------------------------------------------------------------------------------------------------------ GPU
def _find(X, x, **kw):
    from roma_amd import geometry
    R, t, mask = geometry.find_absolute_pose(dev(X), dev(x), dev(K), THR, **kw)
    return R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.gpu
def test_p3p_samples_and_slots_match_the_restatement():
    from roma_amd import geometry
    scenes = [A.scene(m, 0, N=300) for m in ("forward", "turn")]
    X, x = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    r = geometry.absolute_pose_hypotheses(dev(X), dev(x), dev(K), THR, 64, seed=3)
    samples, valid = r["samples"].cpu().numpy(), r["valid"].cpu().numpy()
    Rs, ts, count, cost = (r[k].cpu().numpy() for k in ("R", "t", "count", "cost"))
    assert samples.shape == (2, 64, 3) and Rs.shape == (2, 64, 4, 3, 3) and ts.shape == (2, 64, 4, 3)
    assert np.array_equal(samples, A.minimal_samples(X, x, 64, 3))
    worst, checked, t2 = 0.0, 0, THR * THR
    for p in range(2):
        _, hyp = A.hypotheses(X[p], x[p], K, 64, 3, p0=p)
        for h in range(64):
            assert valid[p, h].sum() == len(hyp[h]), (p, h, valid[p, h], len(hyp[h]))
            assert valid[p, h, :len(hyp[h])].all()                                  # valid slots first
            for s in range(4):
                if not valid[p, h, s]:
                    assert not Rs[p, h, s].any() and not ts[p, h, s].any() and count[p, h, s] == 0 and np.isinf(cost[p, h, s])
                    continue
                d = min(max(np.abs(Rs[p, h, s] - Rw).max(), np.abs(ts[p, h, s] - tw).max()) for Rw, tw in hyp[h])
                worst = max(worst, d)
                assert d <= SLOT_BOUND, (p, h, s, d)
                e = A.errors(Rs[p, h, s], ts[p, h, s], X[p], x[p], K)
                lo, hi = (e < t2 * (1 - 1e-3)).sum(), (e < t2 * (1 + 1e-3)).sum()
                assert lo <= count[p, h, s] <= hi, (p, h, s, lo, count[p, h, s], hi)
                checked += 1
    print(f"P3P vs numpy: {checked} slots compared, worst max-abs difference {worst:.2e} (bound {SLOT_BOUND:.0e})")
    assert checked > 100, checked


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["msac", "magsac"])
@pytest.mark.parametrize("motion", MOTIONS)
def test_find_absolute_pose_meets_the_scene_criteria(motion, scoring):
    X, x, truth, R_true, t_true = A.scene(motion, 0)
    R, t, mask = _find(X, x, max_iters=500, seed=0, scoring=scoring)
    _check_scene(R, t, mask, truth, R_true, t_true, f"find_absolute_pose, {motion}, {scoring}", X, x)


@pytest.mark.gpu
def test_world_offset_does_not_reach_the_fp32_scoring():
    X, x, truth, R_true, t_true = A.scene("turn", 0)
    Xo, to = X + A.OFFSET, t_true - R_true @ A.OFFSET
    for scoring in ("msac", "magsac"):
        R, t, mask = _find(Xo, x, max_iters=500, seed=0, scoring=scoring)
        _check_scene(R, t, mask, truth, R_true, to, f"world offset, {scoring}", Xo, x)
    R, t, mask = _find(Xo, x, max_iters=500, seed=0, refine_iters=15)
    _check_scene(R, t, mask, truth, R_true, to, "world offset, refined", Xo, x)


@pytest.mark.gpu
def test_points_behind_the_camera_are_never_inliers():
    X, x, truth, R_true, t_true = A.scene("sideways", 0)
    pick = np.nonzero(truth)[0][:200]
    mirrored = (-(X[pick] @ R_true.T + t_true) - t_true) @ R_true              # -X_cam back in the world: reprojects onto the same pixel
    Xm, xm = np.concatenate([X, mirrored]), np.concatenate([x, x[pick]])
    tm = np.concatenate([truth, np.zeros(200, bool)])
    assert (A.errors(R_true, t_true, Xm, xm, K)[-200:] == np.inf).all()
    for kw in (dict(), dict(scoring="magsac"), dict(refine_iters=15)):
        R, t, mask = _find(Xm, xm, max_iters=500, seed=0, **kw)
        assert not mask[-200:].any()
        _check_scene(R, t, mask, tm, R_true, t_true, f"mirrored points, {kw}", Xm, xm)


@pytest.mark.gpu
def test_rows_that_are_not_finite_are_never_sampled_and_never_inliers():
    from roma_amd import geometry
    X, x, truth, R_true, t_true = A.scene("forward", 0)
    rng = np.random.default_rng(7)
    bad = rng.permutation(len(X))[:200]
    X, x = X.copy(), x.copy()
    X[bad[:100], rng.integers(0, 3, 100)] = np.nan
    x[bad[100:], rng.integers(0, 2, 100)] = np.nan
    isbad = np.zeros(len(X), bool)
    isbad[bad] = True
    samples = geometry.absolute_pose_hypotheses(dev(X[None]), dev(x[None]), dev(K), THR, 500, seed=0)["samples"][0].cpu().numpy()
    assert np.array_equal(samples, A.minimal_samples(X[None], x[None], 500, 0)[0])
    assert (samples >= 0).all() and not isbad[samples].any()
    for kw in (dict(), dict(refine_iters=15)):
        R, t, mask = _find(X, x, max_iters=500, seed=0, **kw)
        assert not mask[isbad].any()
        _check_scene(R, t, mask, truth & ~isbad, R_true, t_true, f"5 % NaN in X, 5 % in x, {kw}", X, x)


@pytest.mark.gpu
def test_collinear_world_points_give_no_model():
    rng = np.random.default_rng(3)
    X = np.array([1.0, -2.0, 6.0]) + rng.uniform(-3, 3, (50, 1)) * np.array([0.3, 0.5, 0.8])
    x = GS._uniform(rng, GS.W_B, GS.H_B, 50)
    for scoring in ("msac", "magsac"):
        R, t, mask = _find(X, x, max_iters=200, seed=0, scoring=scoring)
        assert not R.any() and not t.any() and not mask.any()


@pytest.mark.gpu
def test_find_absolute_pose_is_deterministic_and_chunking_changes_no_bit(monkeypatch):
    from roma_amd import geometry
    scenes = [A.scene(MOTIONS[p % 4], p // 4, N=600) for p in range(5)]
    X, x = dev(np.stack([s[0] for s in scenes])), dev(np.stack([s[1] for s in scenes]))

    def run(scoring):
        return geometry.find_absolute_pose(X, x, dev(K), THR, 200, seed=11, refine_iters=5, scoring=scoring)

    whole = {scoring: run(scoring) for scoring in ("msac", "magsac")}
    assert all(torch.equal(a, b) for a, b in zip(whole["msac"], run("msac")))
    assert bool(whole["msac"][2].any(-1).all())                                  # every pair found a model
    single = geometry.find_absolute_pose(X[0], x[0], dev(K), THR, 200, seed=11, refine_iters=5)
    assert all(torch.equal(a, b[0]) for a, b in zip(single, whole["msac"]))      # pair 0 alone draws what it draws in the batch
    per_pair, _ = geometry.absolute_pose_workspace_layout(1, 600, 200)
    monkeypatch.setattr(geometry, "_WORKSPACE_LIMIT", 2 * per_pair + 1024)
    assert len(geometry._chunks(geometry._KIND_AP, 5, 600, 200)) == 3
    for scoring in ("msac", "magsac"):
        assert all(torch.equal(a, b) for a, b in zip(whole[scoring], run(scoring))), scoring


@pytest.mark.gpu
def test_refine_absolute_pose_matches_the_restatement():
    from roma_amd import geometry
    costs = []
    for motion in MOTIONS:
        X, x, truth, R_true, t_true = A.scene(motion, 0)
        R0, t0 = _perturbed(R_true, t_true)
        want = A.refine(R0, t0, X, x, K, THR)
        R, t, mask, info = geometry.refine_absolute_pose(dev(R0), dev(t0), dev(X), dev(x), dev(K), THR, 15, return_info=True)
        R, t, mask = R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy()
        d = max(np.abs(R - want["R"]).max(), np.abs(t - want["t"]).max())
        print(f"refine_absolute_pose, {motion}: {int(info['steps'])} steps (restatement {want['steps']}), cost {float(info['cost']):.6f} "
              f"from {want['cost0']:.6f} (restatement {want['cost']:.6f}), pose differs by {d:.2e} (tolerance {REFINE_TOL:.1e})")
        costs.append((motion, d))
        assert int(info["steps"]) >= 1
        assert float(info["cost"]) <= want["cost0"] and int(info["count"]) == mask.sum()
        assert np.array_equal(mask, want["mask"])
        _check_scene(R, t, mask, truth, R_true, t_true, f"refined from the perturbed truth, {motion}", X, x)
    assert all(d <= REFINE_TOL for _, d in costs), costs


@pytest.mark.gpu
def test_refine_absolute_pose_returns_the_input_where_it_cannot_refine():
    from roma_amd import geometry
    X, x, truth, R_true, t_true = A.scene("turn", 0)
    R0, t0 = _perturbed(R_true, t_true)
    three = np.zeros(len(X), bool)
    three[np.nonzero(truth)[0][:3]] = True
    nanR = R0.copy()
    nanR[1, 2] = np.nan
    for Rin, m in ((R0, three), (nanR, None)):
        R, t, mask, info = geometry.refine_absolute_pose(dev(Rin), dev(t0), dev(X), dev(x), dev(K), 50.0, 15,
                                                         mask=None if m is None else dev(m), return_info=True)
        assert R.cpu().numpy().tobytes() == Rin.tobytes() and t.cpu().numpy().tobytes() == t0.tobytes()
        assert int(info["steps"]) == 0 and int(info["count"]) == mask.sum() == (3 if m is not None else 0)


@pytest.mark.gpu
def test_refinement_behind_the_ransac_never_raises_the_cost():
    for motion in MOTIONS:
        X, x, _, _, _ = A.scene(motion, 0)
        R0, t0, _ = _find(X, x, max_iters=500, seed=0)
        R1, t1, _ = _find(X, x, max_iters=500, seed=0, refine_iters=15)
        c0 = A.cost_of(A.errors(R0, t0, X, x, K), THR * THR)
        c1 = A.cost_of(A.errors(R1, t1, X, x, K), THR * THR)
        print(f"{motion}: truncated cost {c0:.6f} after the RANSAC, {c1:.6f} after the refinement")
        assert c1 <= c0 * (1 + 1e-9)                       # the kernel compares in the normalised frame: 1e-9 is the recount's rounding


@pytest.mark.gpu
def test_a_third_view_is_placed_on_triangulated_points():
    from roma_amd import geometry
    xa, xb, xc, truth, (R_ab, t_ab), (R_ac, t_ac) = A.three_view_scene("sideways", "turn", 0)
    # the yardstick: the restatement on the points triangulated under the truth-aware two-view pose
    R2, t2 = PR.truth_aware_fit(xa, xb, np.ones(len(xa), bool), GS.K_A, GS.K_B)
    tri = TR.triangulate(np.concatenate([xa, xb], -1), GS.K_A, GS.K_B, R2, t2)
    Xr = np.where(tri["valid"][:, None], tri["points"], np.nan)
    Rr, tr, _ = A.ransac(Xr, xc, K, THR, 500, 0)
    ref = A.refine(Rr, tr, Xr, xc, K, THR)
    ec_ref, er_ref = A.chain_errors(ref["R"], ref["t"], R_ac, t_ac)
    thr = GS.calibrated_threshold(1.5, GS.K_A, GS.K_B)
    a, b, KA, KB = dev(xa), dev(xb), dev(GS.K_A), dev(GS.K_B)
    R, t, m = geometry.estimate_pose(a, b, KA, KB, thr, seed=0)
    R, t, m = geometry.refine_pose(R, t, a, b, KA, KB, thr)
    pts = geometry.triangulate(a, b, R, t, KA, KB)
    X = torch.where(pts.valid[:, None], pts.points.double(), torch.full((1,), float("nan"), dtype=torch.float64, device=a.device))
    Rc, tc, mask = geometry.find_absolute_pose(X, dev(xc), KB, THR, 500, seed=0, refine_iters=15)
    ec, er = A.chain_errors(Rc.cpu().numpy(), tc.cpu().numpy(), R_ac, t_ac)
    print(f"third view: centre error {ec:.5f} baselines, rotation error {er:.4f} deg (restatement on the truth-aware two-view pose: "
          f"{ec_ref:.5f}, {er_ref:.4f}; bounds {CHAIN_CENTRE_BOUND}, {CHAIN_ROT_BOUND_DEG}); {int(mask.sum())} inliers")
    assert 5 * ec_ref <= CHAIN_CENTRE_BOUND and 5 * er_ref <= CHAIN_ROT_BOUND_DEG
    assert ec <= CHAIN_CENTRE_BOUND and er <= CHAIN_ROT_BOUND_DEG, (ec, er)
    e_c, e_R = geometry.absolute_pose_error(Rc, tc, dev(np.concatenate([R_ac, t_ac[:, None] / A.BASELINE], -1)))
    assert abs(float(e_c) - ec) < 1e-12 and abs(float(e_R) - er) < 1e-6


@pytest.mark.gpu
def test_lift_keypoints_feeds_find_absolute_pose():
    from roma_amd import geometry
    depth, kpts, xb, truth, in_hole, X_true, R_true, t_true = A.depth_map_scene("forward", 0)
    assert 5 <= in_hole.sum() <= 100
    X = geometry.lift_keypoints(dev(kpts), dev(depth), dev(GS.K_A))
    assert X.dtype == torch.float64 and X.shape == (len(kpts), 3)
    Xn = X.cpu().numpy()
    assert np.array_equal(np.isnan(Xn).any(-1), in_hole) and np.array_equal(np.isnan(Xn).all(-1), in_hole)
    assert np.abs(Xn[~in_hole] - X_true[~in_hole]).max() < 1e-12
    outside = dev(np.array([[-0.5, 10.0], [10.0, GS.H_A + 0.5], [GS.W_A + 3.0, 5.0]]))
    assert bool(torch.isnan(geometry.lift_keypoints(outside, dev(depth), dev(GS.K_A))).all())
    both = geometry.lift_keypoints(torch.stack([dev(kpts), dev(kpts)]), torch.stack([dev(depth), dev(depth)]), dev(GS.K_A))
    assert both.shape == (2, len(kpts), 3) and torch.equal(both[1].nan_to_num(7.0), X.nan_to_num(7.0))
    R, t, mask = geometry.find_absolute_pose(X, dev(xb), dev(K), THR, 500, seed=0)
    _check_scene(R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy(), truth, R_true, t_true, "lift_keypoints -> find_absolute_pose", Xn, xb)


@pytest.mark.gpu
def test_estimate_absolute_pose_wraps_find_absolute_pose():
    from roma_amd import geometry
    Ks = GS.no_skew(K)                                                         # the PINHOLE camera has no skew
    assert np.array_equal(np.array(geometry._focal(CAMERA, "camera")[1]), Ks)
    X, x, truth, R_true, t_true = A.scene("backward_up", 0)
    xs = GS.project(X @ R_true.T + t_true, Ks)                                 # the same scene, its inliers projected without skew
    x = np.where(truth[:, None], xs + (x - GS.project(X @ R_true.T + t_true, K)), x)
    pose, info = geometry.estimate_absolute_pose(dev(x), dev(X), CAMERA, {"max_reproj_error": THR, "max_iterations": 500}, seed=4)
    R, t, mask = geometry.find_absolute_pose(dev(X), dev(x), dev(Ks), THR, 500, seed=4, refine_iters=15)
    assert isinstance(pose, geometry.CameraPose)
    assert torch.equal(pose.R, R) and torch.equal(pose.t, t) and torch.equal(info["inliers"], mask)
    assert pose.Rt.shape == (3, 4) and set(info) == {"inliers", "num_inliers", "model_score", "iterations", "refinements"}
    assert all(info[k].is_cuda for k in ("inliers", "num_inliers", "model_score", "refinements")) and info["iterations"] == 500
    assert int(info["num_inliers"]) == int(mask.sum())
    _check_scene(R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy(), truth, R_true, t_true, "estimate_absolute_pose", X, x)
