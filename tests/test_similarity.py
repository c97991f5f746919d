"""roma_amd.geometry, similarity registration: find_similarity / refine_similarity / similarity_hypotheses / register_depth_maps
(csrc/similarity.hip) and the torch helpers apply_similarity / transform_cameras / similarity_error, against the numpy restatement in
tests/similarity_ref.py.  CPU tests pin the restatement to a textbook SVD Umeyama and to ground truth, the C-ABI argument checks, the
Python surface and the kernels' resource report; GPU tests pin the kernels.

Scenes: similarity_ref.scene — N = 2000 points in a box (x in [-3,3], y in [-2,2], z in [4,12]) plus an offset, a rotation of 0.6 rad,
|t| = 2, sigma = 0.01 on X and s sigma on Y, 30 % outliers uniform in Y's bounding box; threshold 4 sqrt 2 s sigma.

Measured with the restatement (the CPU tests print the figures again, and fail if a constant is not what its rule gives):
  CLOSED_TOL       closed form (Horn's quaternion by Jacobi) against numpy-SVD Umeyama and against the truth on exact data: 3 points,
                   planar clouds, general clouds, weights, with and without scale, 400 cases: worst deviation 1.19e-11; 10 x that
  ROT_BOUND_DEG,   5 x the worst error of the truth-aware fit (closed form on the true inliers) over s in {0.05, 1, 20} x 5 seeds x offset
  LOGS_BOUND,      in {0, 1e4} and the rigid scenes: 0.0246 deg, 1.56e-4 in log-scale, 0.00104 X-units at the inliers' centroid;
  CENTRE_BOUND     rounded up
  SLOT_TOL         the minimal solver on exact data — the draws of the GPU test (seed 3, 64 samples, N = 2000 and N = 3) on the scenes
                   without noise and outliers — against the truth: worst deviation 1.18e-11; 10 x that
  REFINE_TOL       the refinement from the truth moved by 0.5 deg, 1 % and 0.05 units, summed over the rows in their order, in reverse
                   and in a shuffled order: the models differ by at most 5.83e-14; 10 x that
  COST_TOL         cost of a slot scored as the kernels do (fp32 errors, fp32 sums over a chunk) against fp64, N in {1023, 1024, 1025},
                   256 samples, both scorings: worst relative difference 9.95e-6; 10 x that
The deviation of two models is similarity_ref.model_deviation: max of |ds| / s, max |dR|, max |dt| / (1 + max |t|).
"""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import general_scenes as GS
from tests import geometry_ref as G
from tests import multiview_scenes as MV
from tests import similarity_ref as S
from tests.helpers import dev, kernel_resources

CLOSED_TOL = 1.2e-10
ROT_BOUND_DEG, LOGS_BOUND, CENTRE_BOUND = 0.13, 8e-4, 0.0052
SLOT_TOL = 1.2e-10
REFINE_TOL = 5.9e-13
COST_TOL = 1.0e-4
BOUNDARY_SAMPLES = 256                 # 1 % of the slots may be left out for a point at the threshold: 2 of 256
SCALES, OFFSETS = (0.05, 1.0, 20.0), (0.0, 1e4)
PERTURB_W = np.radians(0.5) * np.array([0.6, -0.48, 0.64])
PERTURB_T = 0.05 * np.array([0.48, 0.6, -0.64])


def _check_scene(model, mask, truth, gt, X, what):
    """the scene criteria: mask against the truth, proper rotation, model within the bounds at the true inliers' centroid"""
    s, R, t = model
    rec, prec = G.recall_precision(mask, truth)
    er, es, ec = S.model_errors(model, gt, X[truth & np.isfinite(X).all(-1)].mean(0))
    print(f"{what}: rotation {er:.4f} deg, log-scale {es:.2e}, centroid {ec:.5f}, recall {rec:.4f}, precision {prec:.4f}")
    assert rec >= 0.98 and prec >= 0.98, (rec, prec)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert er <= ROT_BOUND_DEG and es <= LOGS_BOUND and ec <= CENTRE_BOUND, (er, es, ec)


def _perturbed(gt):
    s, R, t = gt
    return 1.01 * s, G.rodrigues(PERTURB_W) @ R, t + s * PERTURB_T


def _exact_cases():
    """(x, y, w, with_scale, truth) on exact data: 3 points, planar and general clouds, unit and random weights"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = (3, 4, 10, 100)[trial % 4]
        x = rng.normal(size=(n, 3)) * rng.uniform(0.5, 3)
        if trial % 3 == 0:
            x[:, 2] = 0.3 * x[:, 0] - 0.2 * x[:, 1]
        R, s, t = G.rodrigues(rng.normal(size=3)), float(np.exp(rng.uniform(-3, 3))), 3 * rng.normal(size=3)
        w = np.ones(n) if trial % 2 else rng.uniform(0.1, 1, n)
        for with_scale in (True, False):
            sc = s if with_scale else 1.0
            yield x, sc * x @ R.T + t, w, with_scale, (sc, R, t)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_closed_form_matches_svd_umeyama_on_exact_data():
    worst, n = 0.0, 0
    for x, y, w, with_scale, truth in _exact_cases():
        got = S.closed_form(S.sums(x, y, w), with_scale, 0.0 if len(x) == 3 else S.GAP_TOL)
        assert got is not None and abs(np.linalg.det(got[1]) - 1) < 1e-12
        assert with_scale or got[0] == 1.0
        worst = max(worst, S.model_deviation(got, S.umeyama_svd(x, y, w, with_scale)), S.model_deviation(got, truth))
        n += 1
    print(f"closed form vs SVD Umeyama and the truth, {n} exact cases: worst deviation {worst:.2e}; tolerance {CLOSED_TOL:.1e}")
    assert 0 < 10 * worst <= CLOSED_TOL * 1.0001 and CLOSED_TOL <= 20 * worst, worst


def test_closed_form_rejects_what_does_not_fix_the_rotation():
    rng = np.random.default_rng(2)
    line = np.array([1.0, -2.0, 6.0]) + rng.uniform(-3, 3, (50, 1)) * np.array([0.3, 0.5, 0.8])
    R = G.rodrigues(np.array([0.2, -0.3, 0.4]))
    assert S.closed_form(S.sums(line, 2.0 * line @ R.T + 1.0, np.ones(50))) is None                  # a collinear cloud: no gap
    assert S.minimal(line[:3], 2.0 * line[:3] @ R.T) is None
    x = rng.normal(size=(20, 3))
    assert S.closed_form(S.sums(x, np.zeros_like(x), np.ones(20))) is None                           # Y a single point
    assert S.closed_form(S.sums(x, x, np.zeros(20))) is None                                         # no weight
    assert S.closed_form(S.sums(x, x @ R.T, np.ones(20))) is not None


@pytest.mark.parametrize("s", SCALES)
def test_numpy_restatement_meets_the_scene_criteria(s):
    for offset in OFFSETS:
        X, Y, truth, gt, thr = S.scene(0, s, offset)
        sm, R, t, mask = S.ransac(X, Y, thr, 300, seed=0)
        _check_scene((sm, R, t), mask, truth, gt, X, f"restatement RANSAC, s = {s}, offset {offset:g}")
        r = S.refine((sm, R, t), X, Y, thr)
        _check_scene(r["model"], r["mask"], truth, gt, X, f"restatement RANSAC + refinement, s = {s}, offset {offset:g}")
        assert r["cost"] <= r["cost0"]
    X, Y, truth, gt, thr = S.scene(1, 1.0)
    sm, R, t, mask = S.ransac(X, Y, thr, 300, seed=0, with_scale=False, scoring="magsac")
    assert sm == 1.0
    _check_scene((sm, R, t), mask, truth, gt, X, "restatement RANSAC, rigid, MAGSAC++")


def test_truth_aware_bounds_are_five_times_the_worst_fit():
    wr = ws = wc = 0.0
    for s in SCALES:
        for seed in range(5):
            for offset in OFFSETS:
                for with_scale in ((True, False) if s == 1.0 else (True,)):
                    X, Y, truth, gt, _ = S.scene(seed, s, offset)
                    er, es, ec = S.model_errors(S.truth_aware_fit(X, Y, truth, with_scale), gt, X[truth].mean(0))
                    wr, ws, wc = max(wr, er), max(ws, es), max(wc, ec)
    print(f"truth-aware fit over 40 scenes: worst rotation {wr:.4f} deg, log-scale {ws:.3e}, centroid {wc:.5f} X-units")
    assert 5 * wr <= ROT_BOUND_DEG <= 6 * wr and 5 * ws <= LOGS_BOUND <= 6 * ws and 5 * wc <= CENTRE_BOUND <= 6 * wc, (wr, ws, wc)


def _solver_cases(clean=False):
    """(X, Y, with_scale, truth model) of the solver test: scenes of N = 2000, and N = 3 (three true inliers of the first)"""
    a, b = S.scene(0, 1.0, clean=clean), S.scene(1, 20.0, clean=clean)
    three = np.nonzero(S.scene(0, 1.0)[2])[0][:3]
    return [(a[0], a[1], True, a[3]), (b[0], b[1], True, b[3]), (a[0], a[1], False, a[3]), (a[0][three], a[1][three], True, a[3])]


def test_slot_tolerance_is_ten_times_the_solver_on_exact_data():
    """the draws and rows of the GPU test (seed 3, 64 samples), on the scenes without noise and outliers"""
    worst, n = 0.0, 0
    for X, Y, with_scale, gt in _solver_cases(clean=True):
        _, hyp, nrm = S.hypotheses(X, Y, 64, 3, 0, with_scale)
        for m in hyp:
            if m is not None:
                worst, n = max(worst, S.model_deviation(S.to_caller(m, nrm), gt)), n + 1
    print(f"minimal solver on exact data, {n} samples: worst deviation from the truth {worst:.2e}; tolerance {SLOT_TOL:.1e}")
    assert n > 150 and 0 < 10 * worst <= SLOT_TOL * 1.0001 and SLOT_TOL <= 20 * worst, worst


def test_refinement_never_raises_the_cost_and_its_tolerance_is_ten_times_the_order_of_the_sums():
    worst = 0.0
    for s in SCALES:
        X, Y, truth, gt, thr = S.scene(0, s)
        start = _perturbed(gt)
        r = [S.refine(start, X, Y, thr, order=o) for o in (0, 1, 2)]
        assert all(q["steps"] >= 1 and q["cost"] <= q["cost0"] for q in r)
        assert abs(r[0]["cost0"] - S.cost_of(start, X, Y, thr)) <= 1e-9 * r[0]["cost0"]
        worst = max([worst] + [S.model_deviation(q["model"], r[0]["model"]) for q in r[1:]])
        _check_scene(r[0]["model"], r[0]["mask"], truth, gt, X, f"restatement refinement from the perturbed truth, s = {s}")
    print(f"refinement, three orders of the sums: models differ by at most {worst:.2e}; tolerance {REFINE_TOL:.1e}")
    assert 0 < 10 * worst <= REFINE_TOL * 1.0001 and REFINE_TOL <= 20 * worst, worst


def _boundary_scene(N):
    """the scene at twice its threshold: at 4 sqrt 2 sigma the tail of the inliers' noise puts a point within 1e-4 of the threshold in
    1.2 % of the slots (3 of 256 on average), more than the test may leave out; at 8 sqrt 2 sigma it is the outliers alone"""
    X, Y, _, _, thr = S.scene(2, 1.0, N=N)
    return X, Y, 2.0 * thr


def test_cost_tolerance_is_ten_times_fp32_scoring_against_fp64():
    worst = 0.0
    for N in (1023, 1024, 1025):
        X, Y, thr = _boundary_scene(N)
        for scoring in ("msac", "magsac"):
            v, c64, n64, near = S.slot_scores(X, Y, thr, BOUNDARY_SAMPLES, 1, scoring)
            _, c32, n32, _ = S.slot_scores(X, Y, thr, BOUNDARY_SAMPLES, 1, scoring, fp32=True)
            keep = v & (near > 1e-4)
            assert (v & ~keep).sum() <= 0.01 * BOUNDARY_SAMPLES and np.array_equal(n64[keep], n32[keep])
            worst = max(worst, np.abs(c32[keep] / c64[keep] - 1).max())
    print(f"fp32 scoring against fp64, slot costs: worst relative difference {worst:.2e}; tolerance {COST_TOL:.1e}")
    assert 0 < 10 * worst <= COST_TOL * 1.0001 and COST_TOL <= 20 * worst, worst


def test_similarity_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    rc = lib.roma_similarity_hypotheses(None, None, 1, 100, 10, 0.1, 0, 1, 0, 0, None, 0, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_similarity_hypotheses: null pointer" in lib.roma_last_error()
    rc = lib.roma_similarity_select(None, None, 1, 100, 10, 0.1, 0, 1, 3, None, 0, None, None, None, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_similarity_select: null pointer" in lib.roma_last_error()
    rc = lib.roma_refine_similarity(None, None, None, None, None, None, 1, 100, 0.1, 15, 1, None, None, None, None, None, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_refine_similarity: null pointer" in lib.roma_last_error()
    buf = (ctypes.c_double * 32)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    big = 1 << 40

    def hyp(X=a, Y=a, P=1, N=100, iters=10, thr=0.1, scoring=0, p0=0, ws=a, ws_bytes=big):
        return lib.roma_similarity_hypotheses(X, Y, P, N, iters, thr, scoring, 1, 0, p0, ws, ws_bytes, None)

    def sel(X=a, Y=a, P=1, N=100, iters=10, thr=0.1, scoring=0, lo=3, ws=a, ws_bytes=big, out=a):
        return lib.roma_similarity_select(X, Y, P, N, iters, thr, scoring, 1, lo, ws, ws_bytes, out, a, a, a, a, None)

    def ref(X=a, Y=a, P=1, N=100, thr=0.1, iters=15, out=a):
        return lib.roma_refine_similarity(X, Y, a, a, a, None, P, N, thr, iters, 1, out, a, a, a, a, a, a, None)

    for call in (hyp, sel, ref):
        assert call(N=2) == _lib.ROMA_E_SHAPE and b"need at least 3" in lib.roma_last_error()
        assert call(P=0) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
        for thr in (0.0, -1.0, float("nan")):
            assert call(thr=thr) == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
        assert call(X=odd) == _lib.ROMA_E_ALIGN and b"8-byte" in lib.roma_last_error()
    assert sel(out=None) == _lib.ROMA_E_ARG and b"null pointer" in lib.roma_last_error()
    assert ref(out=None) == _lib.ROMA_E_ARG and b"null pointer" in lib.roma_last_error()
    need = lib.roma_similarity_workspace(1, 100, 10, None)
    off = (ctypes.c_long * 12)()
    assert need > 0 and lib.roma_similarity_workspace(1, 100, 10, ctypes.cast(off, ctypes.c_void_p)) == need
    assert list(off) == sorted(off) and off[0] == 0 and len(set(off)) == 12 and off[11] + 100 * 48 <= need
    assert all(o % 256 == 0 for o in off)
    for call in (hyp, sel):
        assert call(iters=0) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
        assert call(ws_bytes=need - 1) == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
        for scoring in (-1, 2):
            assert call(scoring=scoring, ws_bytes=need) == _lib.ROMA_E_ARG and b"scoring" in lib.roma_last_error()
        assert call(ws=ctypes.c_void_p(ctypes.addressof(buf) + 8)) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()
    assert hyp(p0=-1) == _lib.ROMA_E_ARG and b"pair offset" in lib.roma_last_error()
    assert sel(lo=-1) == _lib.ROMA_E_ARG and b"lo_iters" in lib.roma_last_error()
    assert ref(iters=-1) == _lib.ROMA_E_ARG and b"iters" in lib.roma_last_error()
    assert lib.roma_similarity_workspace(0, 100, 10, None) < 0
    assert lib.roma_abi_version() == 5                                                                  # additive: the ABI stays


def test_similarity_workspace_is_monotone_in_the_batch():
    from roma_amd import geometry
    sizes = [geometry.similarity_workspace_layout(P, 777, 100)[0] for P in (1, 2, 3, 8, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 5
    for P in (2, 3):                                           # a narrower chunk's regions start no later: one workspace serves all
        wide, narrow = geometry.similarity_workspace_layout(P + 1, 777, 100)[1], geometry.similarity_workspace_layout(P, 777, 100)[1]
        assert all(n <= w for n, w in zip(narrow, wide))


def test_similarity_surface_validates_without_a_gpu():
    from roma_amd import geometry
    X, Y = torch.rand(100, 3), torch.rand(100, 3)
    s, I, z = torch.tensor(1.0, dtype=torch.float64), torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_similarity(X, Y, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.refine_similarity(s, I, z, X, Y, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.similarity_hypotheses(X, Y, 0.1, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.register_depth_maps(torch.rand(8, 8), torch.rand(8, 8), I, 0.1)
    with pytest.raises(ValueError, match="needs 3"):
        geometry.find_similarity(X[:2], Y[:2], 0.1)
    with pytest.raises(ValueError, match="one shape"):
        geometry.find_similarity(X, Y[:50], 0.1)
    with pytest.raises(ValueError, match="one shape"):
        geometry.find_similarity(X[:, :2], Y[:, :2], 0.1)
    with pytest.raises(ValueError, match="float32 or float64"):
        geometry.find_similarity(X.half(), Y.half(), 0.1)
    with pytest.raises(ValueError, match="threshold"):
        geometry.find_similarity(X, Y, 0.0)
    with pytest.raises(ValueError, match="max_iters"):
        geometry.find_similarity(X, Y, 0.1, 0)
    with pytest.raises(ValueError, match="scoring"):
        geometry.find_similarity(X, Y, 0.1, scoring="ransac")
    with pytest.raises(ValueError, match="refine_iters"):
        geometry.find_similarity(X, Y, 0.1, refine_iters=-1)
    with pytest.raises(TypeError, match="refine_iters"):
        geometry.find_similarity(X, Y, 0.1, 1000, None, 3, "magsac")
    with pytest.raises(ValueError, match="scoring"):
        geometry.similarity_hypotheses(X, Y, 0.1, scoring="ransac")


def test_similarity_helpers_agree_with_numpy_on_cpu_tensors():
    from roma_amd import geometry
    rng = np.random.default_rng(4)
    X = rng.normal(size=(50, 3)) + np.array([0.0, 0.0, 8.0])
    s, R, t = 1.7, G.rodrigues(np.array([0.3, -0.2, 0.5])), np.array([0.5, -1.0, 2.0])
    ts, tR, tt, tX = torch.tensor(s, dtype=torch.float64), torch.from_numpy(R), torch.from_numpy(t), torch.from_numpy(X)
    Y = geometry.apply_similarity(tX, ts, tR, tt)
    assert np.abs(Y.numpy() - (s * X @ R.T + t)).max() < 1e-13
    both = geometry.apply_similarity(torch.stack([tX, tX]), torch.stack([ts, ts]), torch.stack([tR, tR]), torch.stack([tt, tt]))
    assert both.shape == (2, 50, 3) and torch.equal(both[1], Y)
    # a camera of the source frame sees X where the transformed camera sees apply_similarity(X)
    Rc, tc = G.rodrigues(np.array([-0.1, 0.25, 0.05])), np.array([0.3, -0.2, 0.4])
    Rn, tn = geometry.transform_cameras(torch.from_numpy(Rc), torch.from_numpy(tc), ts, tR, tt)
    assert np.abs(Rn.numpy() - Rc @ R.T).max() < 1e-15 and np.abs(tn.numpy() - (s * tc - Rc @ R.T @ t)).max() < 1e-14
    px = GS.project(X @ Rc.T + tc, GS.K_A)
    assert np.abs(GS.project(Y.numpy() @ Rn.numpy().T + tn.numpy(), GS.K_A) - px).max() < 1e-9
    s2, R2, t2 = 1.02 * s, G.rodrigues(np.radians(0.7) * np.array([0.0, 0.6, 0.8])) @ R, t + np.array([0.01, 0.0, -0.02])
    e_R, e_s, d = geometry.similarity_error(torch.tensor(s2, dtype=torch.float64), torch.from_numpy(R2), torch.from_numpy(t2), ts, tR, tt, tX)
    assert abs(float(e_R) - 0.7) < 1e-9 and abs(float(e_s) - np.log(1.02)) < 1e-12 and d.shape == (50,)
    want = np.linalg.norm((s2 * X @ R2.T + t2) - (s * X @ R.T + t), axis=-1) / s
    assert np.abs(d.numpy() - want).max() < 1e-13
    assert abs(float(e_R) - S.model_errors((s2, R2, t2), (s, R, t), X[0])[0]) < 1e-9
    assert abs(float(d[0]) - S.model_errors((s2, R2, t2), (s, R, t), X[0])[2]) < 1e-13


def test_similarity_kernels_resource_report():
    res = kernel_resources("similarity.hip")
    seen = set()
    for name, r in res.items():
        for key in ("sim_prepare_kernel", "sim_solve_kernel", "sim_score_kernel", "sim_select_kernel", "refine_similarity_kernel"):
            if key in name:
                seen.add(key)
                print(f"{key} ({name[-12:]}): VGPRs {r['VGPRs']}, AGPRs {r.get('AGPRs', 0)}, scratch {r['ScratchSize']} bytes, "
                      f"LDS {r.get('LDS Size', 0)} bytes")
                if key == "sim_score_kernel":
                    assert r["ScratchSize"] == 0, (name, r)
    assert len(seen) == 5, seen
    assert sum("sim_score_kernel" in n for n in res) == 2 and sum("sim_select_kernel" in n for n in res) == 2      # MSAC and MAGSAC++


# ------------------------------------------------------------------------------------------------------------------ GPU
def _find(X, Y, thr, **kw):
    from roma_amd import geometry
    s, R, t, mask = geometry.find_similarity(dev(X), dev(Y), thr, **kw)
    return (float(s), R.cpu().numpy(), t.cpu().numpy()), mask.cpu().numpy()


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float64, device="cuda:0")


def _inliers(model, X, Y, thr):
    with np.errstate(invalid="ignore"):
        return S.errors(model, X, Y) < thr * thr


def _near(model, X, Y, thr):
    """rows whose distance is within 1e-3 relative of the threshold: where the fp32 mask may differ from a recount in fp64"""
    with np.errstate(invalid="ignore"):
        return np.abs(S.errors(model, X, Y) / (thr * thr) - 1) < 1e-3


@pytest.mark.gpu
def test_solver_samples_and_slots_match_the_restatement():
    from roma_amd import geometry
    worst, checked = 0.0, 0
    for X, Y, with_scale, _ in _solver_cases():
        thr = 0.0566
        r = geometry.similarity_hypotheses(dev(X), dev(Y), thr, 64, seed=3, with_scale=with_scale)
        samples, valid = r["samples"].cpu().numpy()[0], r["valid"].cpu().numpy()[0]
        ss, Rs, ts = (r[k].cpu().numpy()[0] for k in ("s", "R", "t"))
        idx, hyp, nrm = S.hypotheses(X, Y, 64, 3, 0, with_scale)
        assert samples.shape == (64, 3) and np.array_equal(samples, idx)
        if len(X) == 3:
            assert all(sorted(row) == [0, 1, 2] for row in samples[samples[:, 0] >= 0]) and (samples[:, 0] >= 0).sum() > 32
        got_nrm = [r[k].cpu().numpy()[0] for k in ("centroid_X", "scale_X", "centroid_Y", "scale_Y")]
        assert all(np.abs(a - b).max() <= 1e-12 * (1 + np.abs(b).max()) for a, b in zip(got_nrm, nrm))
        for h in range(64):
            assert valid[h] == (hyp[h] is not None), (h, valid[h])
            if not valid[h]:
                assert ss[h] == 0 and not Rs[h].any() and not ts[h].any() and np.isinf(r["cost"][0, h].item()) and r["count"][0, h].item() == 0
                continue
            d = S.model_deviation((ss[h], Rs[h], ts[h]), S.to_caller(hyp[h], nrm))
            worst, checked = max(worst, d), checked + 1
            assert d <= SLOT_TOL, (h, d)
            assert with_scale or ss[h] == 1.0
    print(f"solver vs numpy: {checked} slots compared, worst deviation {worst:.2e} (tolerance {SLOT_TOL:.1e})")
    assert checked > 150, checked


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["msac", "magsac"])
@pytest.mark.parametrize("N", [1023, 1024, 1025])
def test_chunk_boundary_costs_and_counts_match_the_restatement(N, scoring):
    from roma_amd import geometry
    X, Y, thr = _boundary_scene(N)
    r = geometry.similarity_hypotheses(dev(X), dev(Y), thr, BOUNDARY_SAMPLES, seed=1, scoring=scoring)
    valid, cost, count, near = S.slot_scores(X, Y, thr, BOUNDARY_SAMPLES, 1, scoring)
    assert np.array_equal(r["valid"].cpu().numpy()[0], valid)
    keep = valid & (near > 1e-4)
    assert (valid & ~keep).sum() <= 0.01 * BOUNDARY_SAMPLES and keep.sum() > 150
    assert np.array_equal(r["count"].cpu().numpy()[0][keep], count[keep])
    rel = np.abs(r["cost"].cpu().numpy()[0][keep] / cost[keep] - 1).max()
    print(f"N = {N}, {scoring}: {keep.sum()} slots, counts equal, costs within {rel:.2e} (tolerance {COST_TOL:.1e})")
    assert rel <= COST_TOL, rel


@pytest.mark.gpu
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("s", SCALES)
def test_find_similarity_meets_the_scene_criteria(s, offset):
    X, Y, truth, gt, thr = S.scene(0, s, offset)
    for scoring in (("msac", "magsac") if s == 1.0 else ("msac",)):
        model, mask = _find(X, Y, thr, max_iters=300, seed=0, scoring=scoring)
        _check_scene(model, mask, truth, gt, X, f"find_similarity, s = {s}, offset {offset:g}, {scoring}")
        assert not ((mask != _inliers(model, X, Y, thr)) & ~_near(model, X, Y, thr)).any()
        refined, rmask = _find(X, Y, thr, max_iters=300, seed=0, scoring=scoring, refine_iters=15)
        _check_scene(refined, rmask, truth, gt, X, f"find_similarity + refinement, s = {s}, offset {offset:g}, {scoring}")
        c0, c1 = S.cost_of(model, X, Y, thr), S.cost_of(refined, X, Y, thr)
        assert c1 <= c0 * (1 + 1e-9), (c0, c1)             # the kernel compares in the normalised frame: 1e-9 is the recount's rounding
    if s == 1.0:
        model, mask = _find(X, Y, thr, max_iters=300, seed=0, with_scale=False)
        assert model[0] == 1.0
        _check_scene(model, mask, truth, gt, X, f"find_similarity, rigid, offset {offset:g}")


@pytest.mark.gpu
def test_find_similarity_is_deterministic_and_chunking_changes_no_bit(monkeypatch):
    from roma_amd import geometry
    scenes = [S.scene(p, 1.0, N=600) for p in range(5)]
    X, Y, thr = dev(np.stack([q[0] for q in scenes])), dev(np.stack([q[1] for q in scenes])), scenes[0][4]

    def run(scoring):
        return geometry.find_similarity(X, Y, thr, 200, seed=11, refine_iters=5, scoring=scoring)

    whole = {scoring: run(scoring) for scoring in ("msac", "magsac")}
    assert all(torch.equal(a, b) for a, b in zip(whole["msac"], run("msac")))
    assert bool(whole["msac"][3].any(-1).all())                                  # every pair found a model
    single = geometry.find_similarity(X[0], Y[0], thr, 200, seed=11, refine_iters=5)
    assert all(torch.equal(a, b[0]) for a, b in zip(single, whole["msac"]))      # pair 0 alone draws what it draws in the batch
    per_pair, _ = geometry.similarity_workspace_layout(1, 600, 200)
    monkeypatch.setattr(geometry, "_WORKSPACE_LIMIT", 2 * per_pair + 1024)
    assert len(geometry._chunks(geometry._KIND_SIM, 5, 600, 200)) == 3
    for scoring in ("msac", "magsac"):
        assert all(torch.equal(a, b) for a, b in zip(whole[scoring], run(scoring))), scoring


@pytest.mark.gpu
def test_three_scenes_in_one_call_equal_three_calls_bit_for_bit():
    from roma_amd import geometry
    scenes = [S.scene(p, 1.0, N=500) for p in range(3)]
    thr = scenes[0][4]
    X, Y = dev(np.stack([q[0] for q in scenes])), dev(np.stack([q[1] for q in scenes]))
    lib = _lib.load()
    total, _ = geometry.similarity_workspace_layout(3, 500, 100)
    batch = geometry.find_similarity(X, Y, thr, 100, seed=5)
    for p in range(3):                                       # the single call with the draw of place p: the C entry points with p0 = p
        ws = torch.empty((total,), dtype=torch.uint8, device=X.device)
        s, R, t = (torch.empty(shape, dtype=torch.float64, device=X.device) for shape in ((1,), (1, 3, 3), (1, 3)))
        mask, valid = torch.empty((1, 500), dtype=torch.uint8, device=X.device), torch.empty((1,), dtype=torch.int32, device=X.device)
        Xp, Yp = X[p:p + 1].contiguous(), Y[p:p + 1].contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.roma_similarity_hypotheses(Xp.data_ptr(), Yp.data_ptr(), 1, 500, 100, thr, 0, 1, 5, p, ws.data_ptr(), total, stream), "h")
        _lib.check(lib.roma_similarity_select(Xp.data_ptr(), Yp.data_ptr(), 1, 500, 100, thr, 0, 1, 3, ws.data_ptr(), total, s.data_ptr(),
                                              R.data_ptr(), t.data_ptr(), mask.data_ptr(), valid.data_ptr(), stream), "s")
        assert int(valid[0]) == 1
        assert torch.equal(s[0], batch[0][p]) and torch.equal(R[0], batch[1][p]) and torch.equal(t[0], batch[2][p])
        assert torch.equal(mask[0].bool(), batch[3][p])
    single = geometry.find_similarity(X[0], Y[0], thr, 100, seed=5)
    assert all(torch.equal(a, b[0]) for a, b in zip(single, batch))


@pytest.mark.gpu
def test_rows_that_are_not_finite_are_never_inliers_and_change_nothing():
    X, Y, truth, gt, thr = S.scene(0, 1.0)
    rng = np.random.default_rng(7)
    bad = np.zeros(len(X), bool)
    bad[rng.permutation(len(X))[:200]] = True
    Xb, Yb = X.copy(), Y.copy()
    rows = np.nonzero(bad)[0]
    Xb[rows[:100], rng.integers(0, 3, 100)] = np.nan
    Yb[rows[100:], rng.integers(0, 3, 100)] = np.inf
    for kw in (dict(), dict(refine_iters=15), dict(scoring="magsac")):
        model, mask = _find(Xb, Yb, thr, max_iters=300, seed=0, **kw)
        assert not mask[bad].any()
        _check_scene(model, mask, truth & ~bad, gt, Xb, f"10 % NaN / inf rows, {kw}")
    # the compacted arrays: the same usable rows in the same order, so the same normalisation and the same sums.  The draw differs (it
    # depends on N), so the RANSAC starts elsewhere; behind the refinement both calls stand at the same fixed point: the same inlier
    # set, and models equal to what the order of the sums is worth (the restatement's two runs agree to the last bit)
    model, mask = _find(Xb, Yb, thr, max_iters=300, seed=0, refine_iters=15)
    cmodel, cmask = _find(Xb[~bad], Yb[~bad], thr, max_iters=300, seed=0, refine_iters=15)
    assert S.model_deviation(model, cmodel) <= REFINE_TOL and np.array_equal(mask[~bad], cmask)


@pytest.mark.gpu
def test_degenerate_pairs_give_no_model_and_leave_their_neighbours_alone():
    from roma_amd import geometry
    X, Y, truth, gt, thr = S.scene(0, 1.0, N=500)
    rng = np.random.default_rng(3)
    line = np.array([1.0, -2.0, 6.0]) + rng.uniform(-3, 3, (500, 1)) * np.array([0.3, 0.5, 0.8])
    nan = np.full_like(X, np.nan)
    two = nan.copy()
    two[:2] = X[:2]
    Xs = np.stack([X, nan, line, two, X])
    Ys = np.stack([Y, nan, 1.0 * line @ gt[1].T + gt[2], Y, Y])
    for scoring in ("msac", "magsac"):
        s, R, t, mask = geometry.find_similarity(dev(Xs), dev(Ys), thr, 100, seed=2, scoring=scoring)
        for p in (1, 2, 3):
            assert float(s[p]) == 0 and not bool(R[p].any()) and not bool(t[p].any()) and not bool(mask[p].any()), p
        alone = geometry.find_similarity(dev(Xs[:1]), dev(Ys[:1]), thr, 100, seed=2, scoring=scoring)
        assert all(torch.equal(a[0], b[0]) for a, b in zip((s, R, t, mask), alone))
        _check_scene((float(s[4]), R[4].cpu().numpy(), t[4].cpu().numpy()), mask[4].cpu().numpy(), truth, gt, X, f"behind three degenerate pairs, {scoring}")
        rs, rR, rt, rmask, info = geometry.refine_similarity(s, R, t, dev(Xs), dev(Ys), thr, 15, return_info=True)
        assert info["steps"][1:4].abs().sum().item() == 0
        assert torch.equal(rs[1:4], s[1:4]) and torch.equal(rR[1:4], R[1:4]) and torch.equal(rt[1:4], t[1:4])
    # the smallest budgets
    model, mask = _find(X, Y, thr, max_iters=1, seed=0, lo_iters=0)
    assert mask.shape == (500,) and (model[0] == 0 or abs(np.linalg.det(model[1]) - 1) < 1e-12)
    hyp = S.hypotheses(X, Y, 1, 0)[1][0]
    assert (model[0] != 0) == (hyp is not None)
    if hyp is not None:
        assert S.model_deviation(model, S.to_caller(hyp, S.normalisation(X, Y, S.usable(X, Y)))) <= 1e-9


@pytest.mark.gpu
def test_refine_similarity_matches_the_restatement():
    from roma_amd import geometry
    for s in SCALES:
        for with_scale in ((True, False) if s == 1.0 else (True,)):
            X, Y, truth, gt, thr = S.scene(0, s)
            start = _perturbed(gt)
            want = S.refine(start, X, Y, thr, with_scale=with_scale)
            rs, R, t, mask, info = geometry.refine_similarity(_scalar(start[0]), dev(start[1]), dev(start[2]), dev(X), dev(Y), thr, 15,
                                                              return_info=True, with_scale=with_scale)
            got, mask = (float(rs), R.cpu().numpy(), t.cpu().numpy()), mask.cpu().numpy()
            d = S.model_deviation(got, want["model"])
            print(f"refine_similarity, s = {s}, with_scale {with_scale}: {int(info['steps'])} steps (restatement {want['steps']}), cost "
                  f"{float(info['cost']):.6e} from {want['cost0']:.6e} (restatement {want['cost']:.6e}), model differs by {d:.2e} "
                  f"(tolerance {REFINE_TOL:.1e})")
            assert int(info["steps"]) == want["steps"] >= 1 and d <= REFINE_TOL
            assert float(info["cost"]) <= want["cost0"] and abs(float(info["cost"]) - want["cost"]) <= 1e-9 * want["cost"]
            assert int(info["count"]) == mask.sum() == want["count"] and np.array_equal(mask, want["mask"])
            assert with_scale or got[0] == 1.0
            _check_scene(got, mask, truth, gt, X, f"refined from the perturbed truth, s = {s}, with_scale {with_scale}")


@pytest.mark.gpu
def test_refine_similarity_returns_the_input_where_it_cannot_refine_and_mask_restricts_the_weights():
    from roma_amd import geometry
    X, Y, truth, gt, thr = S.scene(0, 1.0)
    start = _perturbed(gt)
    two = np.zeros(len(X), bool)
    two[np.nonzero(truth)[0][:2]] = True
    nanR = start[1].copy()
    nanR[1, 2] = np.nan
    Xtwo = np.full_like(X, np.nan)
    Xtwo[two] = X[two]
    for Rin, Xin, m, n in ((start[1], X, two, 2), (nanR, X, None, 0), (start[1], Xtwo, None, 2)):
        s, R, t, mask, info = geometry.refine_similarity(_scalar(start[0]), dev(Rin), dev(start[2]), dev(Xin), dev(Y), 1.0, 15,
                                                         mask=None if m is None else dev(m), return_info=True)
        assert float(s) == start[0] and R.cpu().numpy().tobytes() == Rin.tobytes() and t.cpu().numpy().tobytes() == start[2].tobytes()
        assert int(info["steps"]) == 0 and int(info["count"]) == int(mask.sum()) == n
    # the mask names the only rows that may carry weight: the first 600 true inliers alone give the restatement's fit of those rows
    some = np.zeros(len(X), bool)
    some[np.nonzero(truth)[0][:600]] = True
    want = S.refine(start, X, Y, thr, mask=some)
    s, R, t, mask, info = geometry.refine_similarity(_scalar(start[0]), dev(start[1]), dev(start[2]), dev(X), dev(Y), thr, 15, mask=dev(some),
                                                     return_info=True)
    assert S.model_deviation((float(s), R.cpu().numpy(), t.cpu().numpy()), want["model"]) <= REFINE_TOL
    assert not mask.cpu().numpy()[~some].any() and int(info["count"]) == want["count"] <= 600 and int(info["steps"]) == want["steps"] >= 1
    assert S.model_deviation(want["model"], S.refine(start, X, Y, thr)["model"]) > 100 * REFINE_TOL          # and that is another fit


@pytest.mark.gpu
def test_two_reconstructions_of_four_views_are_brought_into_one_frame():
    from roma_amd import geometry
    sc = MV.multiview_scene(4, 0)
    K, R, t, x = sc["K"], sc["R"], sc["t"], sc["x"].astype(np.float64)
    R_cd = R[3] @ R[2].T
    t_cd = t[3] - R_cd @ t[2]
    u_ab, u_cd = np.linalg.norm(t[1]), np.linalg.norm(t_cd)
    one = geometry.triangulate(dev(x[0]), dev(x[1]), dev(R[1]), dev(t[1] / u_ab), dev(K[0]), dev(K[1]))
    two = geometry.triangulate(dev(x[2]), dev(x[3]), dev(R_cd), dev(t_cd / u_cd), dev(K[2]), dev(K[3]))
    nan = torch.full((1,), float("nan"), dtype=torch.float64, device=one.points.device)
    X1 = torch.where(one.valid[:, None], one.points.double(), nan)
    X2 = torch.where(two.valid[:, None], two.points.double(), nan)
    gt = (u_ab / u_cd, R[2], t[2] / u_cd)                     # cloud 1 = X / u_ab in A's frame, cloud 2 = (R_c X + t_c) / u_cd
    thr = 0.1
    at = sc["X"].mean(0) / u_ab
    rs, rR, rt, rmask = S.ransac(X1.cpu().numpy(), X2.cpu().numpy(), thr, 300, 0)
    ref = S.refine((rs, rR, rt), X1.cpu().numpy(), X2.cpu().numpy(), thr)
    er_ref, es_ref, ec_ref = S.model_errors(ref["model"], gt, at)
    s, Rs, ts, mask = geometry.find_similarity(X1, X2, thr, 300, seed=0, refine_iters=15)
    e_R, e_s, d = geometry.similarity_error(s, Rs, ts, gt[0], dev(gt[1]), dev(gt[2]), dev(at[None]))
    er, es, ec = float(e_R), float(e_s), float(d[0])
    print(f"four views: rotation {er:.4f} deg, log-scale {es:.2e}, centroid {ec:.5f} (restatement on the same clouds: {er_ref:.4f}, "
          f"{es_ref:.2e}, {ec_ref:.5f}); {int(mask.sum())} inliers of {int((one.valid & two.valid).sum())} usable rows")
    assert er <= 5 * er_ref and es <= 5 * es_ref and ec <= 5 * ec_ref, (er, es, ec)
    assert int(mask.sum()) >= 0.98 * ref["count"] > 500
    # camera D, known in cloud 2's frame, expressed in cloud 1's by the inverse similarity: cloud 1 reprojects onto D's observations
    inv = (1.0 / s, Rs.T, -(Rs.T @ ts) / s)
    R_d, t_d = geometry.transform_cameras(dev(R_cd), dev(t_cd / u_cd), *inv)
    seen = mask.cpu().numpy() & sc["seen"].all(0) & ~sc["outlier"].any(0)
    px = GS.project(X1.cpu().numpy()[seen] @ R_d.cpu().numpy().T + t_d.cpu().numpy(), K[3])
    err = np.linalg.norm(px - x[3][seen], axis=-1)
    sg, Rg, tg = gt
    Rt, tt = R_cd @ Rg, (t_cd / u_cd + R_cd @ tg) / sg       # the same camera under the true similarity
    err_true = np.linalg.norm(GS.project(X1.cpu().numpy()[seen] @ Rt.T + tt, K[3]) - x[3][seen], axis=-1)
    print(f"cloud 1 in view D: median reprojection error {np.median(err):.3f} px over {seen.sum()} tracks (true similarity: "
          f"{np.median(err_true):.3f} px; sigma 0.5 px)")
    assert seen.sum() > 500 and np.median(err) <= 1.1 * np.median(err_true) and np.median(err) <= 3.0


@pytest.mark.gpu
def test_register_depth_maps_recovers_the_ratio_of_the_units():
    from roma_amd import geometry
    H, W, ratio = 48, 64, 1.7
    rng = np.random.default_rng(9)
    rows, cols = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    depth = 8.0 + 2.0 * np.sin(cols / 12.0) + 1.5 * np.cos(rows / 9.0)
    d1 = depth + rng.normal(0, S.SIGMA, depth.shape)
    d2 = ratio * (depth + rng.normal(0, S.SIGMA, depth.shape))
    wrong = rng.random(depth.shape) < 0.2
    d2[wrong] = ratio * rng.uniform(4, 12, wrong.sum())
    d1[10:16, 20:30], d2[30:34, 5:15], d1[0, 0], d2[47, 63] = 0.0, np.nan, -1.0, np.inf
    hole = ~(np.isfinite(d1) & np.isfinite(d2) & (np.nan_to_num(d1) > 0) & (np.nan_to_num(d2) > 0))
    Kd = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]])
    thr = 4.0 * np.sqrt(2.0) * ratio * S.SIGMA
    s, R, t, mask = geometry.register_depth_maps(dev(d1), dev(d2), dev(Kd), thr, max_iters=300, seed=0, refine_iters=15)
    assert mask.shape == (H, W) and mask.dtype == torch.bool and s.shape == () and R.shape == (3, 3) and t.shape == (3,)
    mask = mask.cpu().numpy()
    assert not mask[hole].any()
    rec, prec = G.recall_precision(mask, ~hole & ~wrong)
    rays = np.stack([cols, rows, np.ones_like(cols)], -1) @ np.linalg.inv(Kd).T
    at = (rays * depth[..., None])[~hole & ~wrong].mean(0)
    er, es, ec = S.model_errors((float(s), R.cpu().numpy(), t.cpu().numpy()), (ratio, np.eye(3), np.zeros(3)), at)
    print(f"register_depth_maps: s = {float(s):.5f} (ratio {ratio}), rotation {er:.4f} deg, |t| {float(t.norm()):.5f}, centroid {ec:.5f}, "
          f"recall {rec:.4f}, precision {prec:.4f}")
    assert rec >= 0.98 and prec >= 0.98            # a wrong cell is uniform along its ray: 1.4 % of them fall within the threshold
    assert es <= LOGS_BOUND and er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND
    # t is the centroid's error carried to the origin, |at| away: by the rotation and the scale bounds at most
    assert float(t.norm()) <= ratio * (CENTRE_BOUND + np.linalg.norm(at) * (np.radians(ROT_BOUND_DEG) + LOGS_BOUND))
