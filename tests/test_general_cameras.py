"""The two-view stack of roma_amd.geometry on two DIFFERENT, general cameras (fx != fy, skew, off-centre principal point, images of
1024 x 768 and 800 x 600) and four motion families — sideways, forward (epipole inside both images), backward and up, a 25 degree
turn —, against the numpy restatements (tests/pose_ref.py, pose_refine_ref.py, geometry_ref.py, fundamental_refine_ref.py,
homography_refine_ref.py) on the scenes of tests/general_scenes.py.  The other geometry modules run one camera, passed as (K, K), and
one sideways motion: K_A and K_B exchanged, K_B^T F K_A transposed, a wrong skew or fy term of K^-1, T_A and T_B exchanged in a
de-normalisation, one focal length where estimate_relative_pose documents the mean of two, or a solver that only copes with sideways
motion would pass them.  Here each of these fails.  CPU tests pin the restatements to ground truth on these scenes and recompute the
bounds the GPU tests use; GPU tests pin the kernels and wrappers.

Bounds, all from the restatements alone (test_yardsticks_come_from_the_restatement recomputes and prints them, and fails if a
recorded one is below what it finds):

Accuracy.  ROT_BOUND_DEG, TRANS_BOUND_DEG = 5 x the worst error of pose_ref.truth_aware_fit (least squares on the true inliers, no
RANSAC) over the 4 motions x seeds (0, 1), rounded up — the convention of tests/test_pose.py.  Worst: 0.0649 deg in R, 0.1943 deg in
t; bounds 0.35 deg, 1.0 deg.  A pose from F (estimate_pose_uncalibrated) gets 3 x that: F has two more degrees of freedom than E.

Refinement parity.  Device and restatement run the same fp64 algorithm from the same start and differ in the last bits of their
sums, sqrt and division.  How far such last bits move the result is measured on the restatement itself: pose_refine_ref.refine from
the restatement's RANSAC pose of each motion (seed 0), and again four times with every coordinate of xa, xb moved to a neighbouring
fp64 value (np.nextafter, direction by a seeded coin).  Largest movement: 2.13e-14 deg in R, 5.78e-14 deg in t, 3.58e-15 relative in
the final cost, 1.49e-10 thr^2 in any match's r^2 (REF_*, rounded up); the bounds are 10 x these.  No match crossed thr^2 in
these runs; the masks were equal.

F and H.  The criteria of tests/test_geometry.py (_check_two_view, _check_planar: recall and precision >= 0.98, median Sampson
distance of the clean inliers <= 0.2 px, rank 2; corner error <= 1 px) hold for geometry_ref.ransac on these scenes at 1.5 px (F) and
3 px (H) — test_restatements_meet_the_f_and_h_criteria —, so all of them are used.  The refinement parity cases (F on the turn, H
on the planar scene) use the bounds of tests/test_fundamental_refine.py and tests/test_homography_refine.py as they stand.

F refinement on the forward scene.  The model and cost bounds of tests/test_fundamental_refine.py (1.51e-15 in |F_dev - F_np|_F,
3.49e-15 relative in the cost: 10 x what the device showed on four sideways scenes) do not hold there for the restatement against
ITSELF: with its input points moved by one ulp, fundamental_refine_ref.refine moves by 8.44e-14 in |dF|_F and 1.04e-14 relative in
the cost (on the turn: 3.3e-18 and 1.7e-15; on two_view_scene(11..14): at most 2.1e-15 and 2.6e-15).  An MI355X differed from the
restatement by 4.04e-14 and 1.20e-14 on that scene, with the same 4 kept steps, 1402 inliers and mask: inside the restatement's own
noise, outside those two bounds.  So the forward scene is a second parity case whose model and cost bounds are made like the
pose bounds above, 10 x the restatement's own movement (REF_F_*, recomputed by test_yardsticks_come_from_the_restatement), under
the hard ceilings of that module (1e-9, 1e-10); steps, counts, masks and the r^2 band are checked as there."""
import functools

import numpy as np
import pytest
import torch

from tests import fundamental_refine_ref as FR
from tests import general_scenes as GS
from tests import geometry_ref as G
from tests import homography_refine_ref as HR
from tests import pose_ref as PR
from tests import pose_refine_ref as RR
from tests import test_fundamental_refine as TF
from tests import test_geometry as TG
from tests import test_homography_refine as TH
from tests.helpers import dev, to_np

DEV = "cuda:0"
KA, KB, THR_G = GS.K_A, GS.K_B, GS.THR_G
MOTIONS = list(GS.MOTIONS)
ROT_BOUND_DEG, TRANS_BOUND_DEG = 0.35, 1.0                   # 5 x the worst truth-aware error, rounded up (header)
F_POSE_FACTOR = 3.0
# largest movement of pose_refine_ref.refine under a one-ulp change of its input points (header), rounded up
REF_ROT_DEG, REF_TRANS_DEG, REF_COST_REL, REF_R2_REL = 2.5e-14, 6e-14, 4e-15, 2e-10
# the same for fundamental_refine_ref.refine on the forward scene: |dF|_F and relative cost (header), rounded up
REF_F_MODEL, REF_F_COST_REL = 9e-14, 1.1e-14
PARITY_ROT_DEG, PARITY_TRANS_DEG, PARITY_COST_REL, PARITY_R2_REL = 10 * REF_ROT_DEG, 10 * REF_TRANS_DEG, 10 * REF_COST_REL, 10 * REF_R2_REL


def _angle_deg(a, b):
    """angle between two unit vectors by the chord (arccos of the dot product resolves nothing below 1e-6 deg)"""
    return float(np.rad2deg(2.0 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(a - b)))))


def _rot_deg(Ra, Rb):
    return float(np.rad2deg(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))))


def _cost(R, t, xa, xb, Ka, Kb, thr):
    xh, xh2 = PR.calibrate(xa, Ka), PR.calibrate(xb, Kb)
    return RR.truncated_cost(R, t, xh, xh2, thr, RR.usable(xh, xh2))


def _assert_pose(R, t):
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.norm(t) - 1) < 1e-12


def _check_pose(R_true, t_true, emask, R, t, mask, truth, what, factor=1.0):
    """_check_pose_scene of tests/test_pose.py with the scene's pose as an argument"""
    rec, prec = G.recall_precision(emask, truth)
    assert rec >= 0.98 and prec >= 0.98, (what, rec, prec)
    _assert_pose(R, t)
    assert not (mask & ~emask).any()
    assert (mask & truth).sum() >= 0.98 * truth.sum(), (what, (mask & truth).sum(), truth.sum())
    er, et = PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)
    print(f"{what}: rotation error {er:.4f} deg, translation error {et:.4f} deg, model mask recall {rec:.4f} precision {prec:.4f}, "
          f"{int(mask.sum())} of {int(emask.sum())} pass cheirality")
    assert er <= factor * ROT_BOUND_DEG and et <= factor * TRANS_BOUND_DEG, (what, er, et)
    assert np.dot(t, t_true) > 0, what                       # the cheirality vote picks the sign, not only the axis


@functools.lru_cache(maxsize=None)
def _np_start(motion, seed=0):
    """the restatement's RANSAC pose of general_scene(motion, seed): scene, E, its mask, recover_pose's output.  Read only."""
    scene = GS.general_scene(motion, seed)
    xa, xb = scene[:2]
    E, emask = PR.ransac_essential(xa, xb, KA, KB, THR_G, 300, seed=seed)
    return scene, E, emask, PR.recover_pose(E, xa, xb, KA, KB, emask)


def _neighbour(x, rng):
    return np.nextafter(x, np.where(rng.integers(0, 2, x.shape) == 1, np.inf, -np.inf))


def _refine_movement(motion):
    """(rotation deg, translation deg, relative cost, r^2 / thr^2) by which four one-ulp changes of the points move RR.refine, and
    whether any mask entry changed"""
    (xa, xb, _, _, _), _, _, (R0, t0, _, _) = _np_start(motion)
    o = RR.refine(R0, t0, xa, xb, KA, KB, THR_G)
    r2 = RR.residuals(o["R"], o["t"], PR.calibrate(xa, KA), PR.calibrate(xb, KB)) ** 2
    rng = np.random.default_rng(7)
    worst, crossed = np.zeros(4), 0
    for _ in range(4):
        xa2, xb2 = _neighbour(xa, rng), _neighbour(xb, rng)
        o2 = RR.refine(R0, t0, xa2, xb2, KA, KB, THR_G)
        r2b = RR.residuals(o2["R"], o2["t"], PR.calibrate(xa2, KA), PR.calibrate(xb2, KB)) ** 2
        worst = np.maximum(worst, [_rot_deg(o["R"], o2["R"]), _angle_deg(o["t"], o2["t"]), abs(o["cost"] - o2["cost"]) / o["cost"],
                                   np.abs(r2 - r2b).max() / THR_G ** 2])
        crossed += int((o["mask"] != o2["mask"]).sum())
    return worst, crossed, o


@functools.lru_cache(maxsize=None)
def _np_fundamental(motion):
    """the restatement's RANSAC F of general_scene(motion, 0) at the settings of tests/test_fundamental_refine.py.  Read only."""
    xa, xb = GS.general_scene(motion, 0)[:2]
    return xa, xb, G.ransac("fundamental", xa, xb, TF.THR, TF.SAMPLES, seed=0)[0]


def _f_refine_movement(motion):
    """(|dF|_F, relative cost) by which four one-ulp changes of the points move FR.refine, and the mask entries that changed"""
    xa, xb, F0 = _np_fundamental(motion)
    o = FR.refine(F0, xa, xb, TF.THR)
    rng = np.random.default_rng(7)
    worst, crossed = np.zeros(2), 0
    for _ in range(4):
        o2 = FR.refine(F0, _neighbour(xa, rng), _neighbour(xb, rng), TF.THR)
        worst = np.maximum(worst, [np.linalg.norm(o["F"] - o2["F"]), abs(o["cost"] - o2["cost"]) / o["cost"]])
        crossed += int((o["mask"] != o2["mask"]).sum())
    return worst, crossed, o


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_scenes_are_what_they_say():
    for motion in MOTIONS:
        xa, xb, truth, R, t = GS.general_scene(motion, 0)
        ca, cb = GS.general_scene(motion, 0, sigma=0.0)[:2]
        assert xa.shape == xb.shape == (2000, 2) and truth.sum() == 1400
        assert (xa >= -3).all() and (xa[:, 0] < GS.W_A + 3).all() and (xa[:, 1] < GS.H_A + 3).all()
        assert (xb >= -3).all() and (xb[:, 0] < GS.W_B + 3).all() and (xb[:, 1] < GS.H_B + 3).all()
        assert xb[:, 0].max() > GS.W_B - 20 and xa[:, 0].max() > GS.W_A - 20
        assert np.array_equal(ca[~truth], xa[~truth]) and np.abs(ca[truth] - xa[truth]).max() < 3.0
        Rp, tp = GS.scene_pose(motion, 0)
        assert np.array_equal(Rp, R) and np.array_equal(tp, t) and abs(np.linalg.norm(t) - 1) < 1e-15
        F = GS.fundamental_from_pose(R, t)
        assert np.sqrt(G.errors("fundamental", F, ca[truth], cb[truth])).max() < 1e-9
        # the generality is not decoration: the same clean matches are off the model under exchanged cameras (by more than the 1.5 px
        # threshold) and without the skew (by a fraction of a pixel: what the parity tests resolve, not the accuracy ones)
        d = np.sqrt(G.errors("fundamental", GS.fundamental_from_pose(R, t, KB, KA), ca[truth], cb[truth]))
        assert np.median(d) > 1.5, (motion, np.median(d))
        d = np.sqrt(G.errors("fundamental", GS.fundamental_from_pose(R, t, GS.no_skew(KA), GS.no_skew(KB)), ca[truth], cb[truth]))
        assert d.max() > 0.05, (motion, d.max())
        # the epipole of the forward motion lies inside both images, that of the sideways one far outside
        e = KB @ t
        inside = 0 <= e[0] / e[2] < GS.W_B and 0 <= e[1] / e[2] < GS.H_B
        assert inside == (motion == "forward"), (motion, e / e[2])
    assert abs(THR_G - GS.calibrated_threshold(1.5, KA, KB)) < 1e-18
    xa, xb, truth, H = GS.general_planar_scene(0)
    hb = np.concatenate([xa, np.ones((len(xa), 1))], -1) @ H.T
    assert np.abs(hb[truth, :2] / hb[truth, 2:3] - xb[truth]).max() < 3.0 and truth.sum() == 1200
    c = np.array([[0, 0, 1], [GS.W_A, GS.H_A, 1.0]]) @ H.T
    assert np.abs(c[:, :2] / c[:, 2:3] - [[0, 0], [GS.W_B, GS.H_B]]).max() <= 60 + 1e-9


def test_numpy_five_point_and_recover_pose_on_exact_general_data():
    for motion in MOTIONS:
        xa, xb, R, t = GS.exact_scene(motion, 0)
        xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
        models, w, cond = PR.five_point(xh[:5], xh2[:5])
        assert 1 <= len(models) <= 10
        E = PR.essential_from_pose(R, t)
        errs = [np.abs(G.sign_fixed(m) - E).max() for m in models]
        assert min(errs) < 1e-7, (motion, errs)
        Rr, tr, mask, count = PR.recover_pose(E, xa, xb, KA, KB)
        assert np.abs(Rr - R).max() < 1e-9 and np.abs(tr - t).max() < 1e-9, motion
        assert mask.all() and count == len(xa)
        Rs, ts, ms, _ = PR.recover_pose(E, xa, xb, KB, KA)        # exchanged cameras: the vote is no longer unanimous
        assert not ms.all()


def test_yardsticks_come_from_the_restatement():
    worst = np.zeros(2)
    for motion in MOTIONS:
        for seed in (0, 1):
            xa, xb, truth, R_true, t_true = GS.general_scene(motion, seed)
            R, t = PR.truth_aware_fit(xa, xb, truth, KA, KB)
            e = PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)
            print(f"truth-aware fit, {motion} {seed}: rotation error {e[0]:.4f} deg, translation error {e[1]:.4f} deg")
            worst = np.maximum(worst, e)
    print(f"accuracy: 5 x worst = {5 * worst[0]:.4f} deg, {5 * worst[1]:.4f} deg; recorded {ROT_BOUND_DEG} deg, {TRANS_BOUND_DEG} deg")
    assert 5 * worst[0] <= ROT_BOUND_DEG <= 10 * worst[0] and 5 * worst[1] <= TRANS_BOUND_DEG <= 10 * worst[1]
    moved = np.zeros(4)
    for motion in MOTIONS:
        m, crossed, o = _refine_movement(motion)
        print(f"refine, {motion}: one-ulp inputs move the result by {m[0]:.3e} deg, {m[1]:.3e} deg, cost {m[2]:.3e} relative, r^2 {m[3]:.3e} "
              f"thr^2; {crossed} mask entries change; {o['steps']} kept steps, cost {o['cost0']:.6e} -> {o['cost']:.6e}")
        assert o["steps"] >= 1 and crossed == 0
        moved = np.maximum(moved, m)
    rec = np.array([REF_ROT_DEG, REF_TRANS_DEG, REF_COST_REL, REF_R2_REL])
    print(f"refinement parity: largest movement {moved}, recorded {rec}, bounds {10 * rec}")
    assert (moved <= rec).all(), (moved, rec)
    # F refinement: the turn keeps the bounds of tests/test_fundamental_refine.py, the forward scene cannot (header)
    mt, crossed_t, ot = _f_refine_movement("turn")
    mf, crossed_f, of = _f_refine_movement("forward")
    print(f"F refine: one-ulp inputs move the result by |dF| {mt[0]:.3e}, cost {mt[1]:.3e} relative on the turn ({ot['steps']} steps) and by "
          f"|dF| {mf[0]:.3e}, cost {mf[1]:.3e} on the forward scene ({of['steps']} steps); bounds of test_fundamental_refine.py "
          f"{TF.PARITY_MODEL:.3e}, {TF.PARITY_COST_REL:.3e}; recorded for the forward scene {REF_F_MODEL}, {REF_F_COST_REL}")
    assert ot["steps"] >= 1 and of["steps"] >= 1 and crossed_t == 0 and crossed_f == 0
    assert mt[0] <= TF.PARITY_MODEL                            # by a factor of hundreds; the cost's movement is printed above
    assert mf[0] > TF.PARITY_MODEL and mf[1] > TF.PARITY_COST_REL          # why the forward scene has bounds of its own
    assert mf[0] <= REF_F_MODEL and mf[1] <= REF_F_COST_REL
    assert 10 * REF_F_MODEL <= TF.CEILING_MODEL and 10 * REF_F_COST_REL <= TF.CEILING_COST_REL


def test_restatement_meets_the_pose_criteria_on_every_motion():
    for motion in MOTIONS:
        (xa, xb, truth, R_true, t_true), E, emask, (R, t, mask, count) = _np_start(motion)
        s = np.linalg.svd(E, compute_uv=False)
        assert abs(s[0] - s[1]) / s[0] < 1e-9 and s[2] / s[0] < 1e-12 and count == mask.sum()
        _check_pose(R_true, t_true, emask, R, t, mask, truth, f"restatement, {motion}")
        o = RR.refine(R, t, xa, xb, KA, KB, THR_G)
        assert PR.rotation_error_deg(o["R"], R_true) <= ROT_BOUND_DEG and PR.translation_error_deg(o["t"], t_true) <= TRANS_BOUND_DEG
        # exchanged cameras leave the restatement without a model worth the name
        rec = G.recall_precision(G.errors("fundamental", E, PR.calibrate(xa, KB), PR.calibrate(xb, KA)) < THR_G ** 2, truth)[0]
        assert rec < 0.5, (motion, rec)


def test_restatements_meet_the_f_and_h_criteria():
    """what the header says of _check_two_view and _check_planar on these scenes; and the pose of F, with the transposed product"""
    for motion in ("forward", "turn"):
        xa, xb, truth, R_true, t_true = GS.general_scene(motion, 0)
        ca, cb = GS.general_scene(motion, 0, sigma=0.0)[:2]
        F, mask = G.ransac("fundamental", xa, xb, 1.5, 300, seed=1)
        TG._check_two_view(F, mask, truth, ca, cb)
        R, t, pmask, _ = PR.recover_pose(KB.T @ F @ KA, xa, xb, KA, KB, mask)
        _check_pose(R_true, t_true, mask, R, t, pmask, truth, f"restatement F pose, {motion}", F_POSE_FACTOR)
        Rw, tw = PR.recover_pose(KA.T @ F @ KB, xa, xb, KA, KB, mask)[:2]
        assert PR.rotation_error_deg(Rw, R_true) > 4.0, motion
        o = FR.refine(F, xa, xb, 1.5)
        assert o["steps"] >= 1
    xa, xb, truth, H_true = GS.general_planar_scene(0)
    H, mask = G.ransac("homography", xa, xb, 3.0, 300, seed=2)
    TG._check_planar(H, mask, truth, H_true)
    assert HR.refine(H, xa, xb, 1.5)["steps"] >= 1


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("motion", ["forward", "turn"])
def test_calibration_and_five_point_models_match_numpy(motion):
    from roma_amd import geometry
    xa, xb = GS.general_scene(motion, 5, N=600)[:2]
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "essential", THR_G, max_iters=200, seed=7, K_A=dev(KA), K_B=dev(KB))
    for got, K in ((r["T_A"], KA), (r["T_B"], KB)):
        want = np.linalg.inv(K)
        assert np.abs(got[0].cpu().numpy() - want).max() <= 1e-15 * np.abs(want).max(), (got, want)
    xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    models, valid, samples = to_np(r["models"][0], r["valid"][0], r["samples"][0])
    assert models.shape == (200, 10, 3, 3) and np.array_equal(samples, PR.minimal_samples(xa[None], xb[None], 200, 7)[0])
    usable, skipped, checked, worst = 0, 0, 0, 0.0
    for h in range(200):
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
    print(f"{motion}: 5-point vs numpy: {checked} slots of {usable - skipped} samples compared, worst max-abs difference {worst:.2e}; "
          f"{skipped} of {usable} valid samples left out as ill-conditioned")
    assert skipped <= 0.05 * usable, (skipped, usable)
    assert checked >= 300, checked


def _msac(E, xh, xh2, t2):
    e = G.errors("fundamental", E, xh, xh2)
    return np.where(e < t2, e, t2).sum()


@pytest.mark.gpu
def test_essential_inlier_counts_equal_an_fp64_recount_on_calibrated_points():
    from roma_amd import geometry
    xa, xb = GS.general_scene("forward", 6)[:2]
    xa[17] = np.nan
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "essential", THR_G, max_iters=100, seed=9, K_A=KA, K_B=KB)
    xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    models, valid, count = to_np(r["models"][0], r["valid"][0], r["count"][0])
    assert valid.sum() > 200
    t2 = THR_G * THR_G
    for h, s in zip(*np.nonzero(valid)):
        e = G.errors("fundamental", models[h, s], xh, xh2)
        lo, hi = (e < t2 * (1 - 1e-3)).sum(), (e < t2 * (1 + 1e-3)).sum()
        assert lo <= count[h, s] <= hi, (h, s, lo, count[h, s], hi)
    assert count.max() > 1300                                 # of 1400 true inliers: some slot is the scene's model
    assert (count[~valid] == 0).all() and np.isinf(r["cost"][0].cpu().numpy()[~valid]).all()


@pytest.mark.gpu
def test_essential_selection_and_local_optimisation():
    from roma_amd import geometry
    xa, xb = GS.general_scene("turn", 13)[:2]
    xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    r = geometry.score_hypotheses(dev(xa), dev(xb), "essential", THR_G, max_iters=500, seed=21, K_A=KA, K_B=KB)
    best = int(np.argmin(r["cost"][0].cpu().numpy().reshape(-1)))
    want = G.sign_fixed(r["models"][0].cpu().numpy().reshape(-1, 3, 3)[best])
    E0, mask0 = geometry.find_essential(dev(xa), dev(xb), KA, KB, THR_G, max_iters=500, seed=21, lo_iters=0)
    E0 = E0.cpu().numpy()
    assert np.abs(E0 - want).max() <= 1e-9, (E0, want)
    E3, mask3 = geometry.find_essential(dev(xa), dev(xb), KA, KB, THR_G, max_iters=500, seed=21, lo_iters=3)
    E3 = E3.cpu().numpy()
    t2 = THR_G * THR_G
    assert _msac(E3, xh, xh2, t2) < _msac(E0, xh, xh2, t2), (_msac(E3, xh, xh2, t2), _msac(E0, xh, xh2, t2))
    for E in (E0, E3):
        s = np.linalg.svd(E, compute_uv=False)
        assert abs(np.linalg.norm(E) - 1) < 1e-12 and abs(s[0] - s[1]) / s[0] < 1e-9 and s[2] / s[0] < 1e-12, s
        assert E.reshape(-1)[np.abs(E).argmax()] > 0
    e = G.errors("fundamental", E3, xh, xh2)
    m = mask3.cpu().numpy()
    assert ((e < t2 * (1 - 1e-3)) <= m).all() and (m <= (e < t2 * (1 + 1e-3))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("motion", MOTIONS)
def test_pose_of_every_motion(motion, seed):
    from roma_amd import geometry
    xa, xb, truth, R_true, t_true = GS.general_scene(motion, seed)
    a, b = dev(xa).float(), dev(xb).float()
    E, emask = geometry.find_essential(a, b, KA, KB, THR_G, max_iters=500, seed=seed)
    R, t, mask = geometry.estimate_pose(a, b, KA, KB, THR_G, max_iters=500, seed=seed)
    assert R.shape == (3, 3) and R.dtype == torch.float64 and t.shape == (3,) and mask.shape == (2000,) and mask.dtype == torch.bool
    _check_pose(R_true, t_true, *to_np(emask, R, t, mask), truth, f"device, {motion} {seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("esign", [1.0, -1.0])
def test_recover_pose_picks_the_true_candidate(sign, esign):
    """test_recover_pose_picks_the_true_candidate of tests/test_pose.py with two cameras, forward motion and the turn"""
    from roma_amd import geometry
    for motion in ("forward", "turn"):
        xa, xb, R_true, t_true = GS.exact_scene(motion, 0, N=2000, sign=sign)
        rng = np.random.default_rng(3)
        truth = rng.uniform(size=2000) >= 0.25
        xb[~truth] = np.stack([rng.uniform(0, GS.W_B, 2000), rng.uniform(0, GS.H_B, 2000)], -1)[~truth]
        E = esign * 0.37 * G.skew(t_true) @ R_true
        xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
        for Rc, tc in PR.decompose(E):
            la, lb = PR.depths(Rc, tc, xh[truth], xh2[truth])
            assert np.isfinite(la).all() and np.isfinite(lb).all() and min(np.abs(la).min(), np.abs(lb).min()) > 1e-6
        Rw, tw, mw, cw = PR.recover_pose(E, xa, xb, KA, KB, truth)
        assert cw == truth.sum() and np.abs(Rw - R_true).max() < 1e-9 and np.abs(tw - t_true).max() < 1e-9
        R, t, mask = geometry.recover_pose(dev(E), dev(xa), dev(xb), KA, KB, dev(truth))
        assert np.abs(R.cpu().numpy() - R_true).max() < 1e-9 and np.abs(t.cpu().numpy() - t_true).max() < 1e-9, motion
        assert np.array_equal(mask.cpu().numpy(), mw) and int(mask.sum()) == cw, motion


@pytest.mark.gpu
@pytest.mark.parametrize("motion", ["forward", "turn"])
def test_estimate_pose_uncalibrated_is_find_fundamental_then_recover_pose_of_kb_f_ka(motion):
    from roma_amd import geometry
    xa, xb, truth, R_true, t_true = GS.general_scene(motion, 0)
    a, b, Ka, Kb = dev(xa).float(), dev(xb).float(), dev(KA), dev(KB)
    R, t, mask = geometry.estimate_pose_uncalibrated(a, b, Ka, Kb, 1.5, max_iters=2000, seed=17)
    F, fmask = geometry.find_fundamental(a, b, threshold=1.5, max_iters=2000, seed=17)
    R2, t2, mask2 = geometry.recover_pose(Kb.transpose(-1, -2) @ F @ Ka, a, b, Ka, Kb, fmask)
    assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(mask, mask2)
    _check_pose(R_true, t_true, *to_np(fmask, R, t, mask), truth, f"device F pose, {motion}", F_POSE_FACTOR)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", MOTIONS)
def test_refine_parity_with_the_restatement(motion):
    from roma_amd import geometry
    seed = 0
    xa, xb, truth, R_true, t_true = GS.general_scene(motion, seed)
    R0, t0, _ = geometry.estimate_pose(dev(xa), dev(xb), KA, KB, THR_G, max_iters=500, seed=seed)
    R, t, mask, info = geometry.refine_pose(R0, t0, dev(xa), dev(xb), KA, KB, THR_G, return_info=True)
    assert R.shape == (3, 3) and R.dtype == torch.float64 and t.shape == (3,) and mask.shape == (2000,) and mask.dtype == torch.bool
    R0, t0, R, t, mask = to_np(R0, t0, R, t, mask)
    o = RR.refine(R0, t0, xa, xb, KA, KB, THR_G)
    c0, c1 = _cost(R0, t0, xa, xb, KA, KB, THR_G), _cost(R, t, xa, xb, KA, KB, THR_G)
    assert c1 <= c0, (c0, c1)
    _assert_pose(R, t)
    assert int(info["count"]) == int(mask.sum())
    xh, xh2 = PR.calibrate(xa, KA), PR.calibrate(xb, KB)
    r2d, r2n = RR.residuals(R, t, xh, xh2) ** 2, RR.residuals(o["R"], o["t"], xh, xh2) ** 2
    fig = np.array([_rot_deg(R, o["R"]), _angle_deg(t, o["t"]), abs(float(info["cost"]) - o["cost"]) / o["cost"],
                    np.abs(r2d - r2n).max() / THR_G ** 2])
    differ = mask != o["mask"]
    band = np.abs(r2n - THR_G ** 2) <= PARITY_R2_REL * THR_G ** 2
    print(f"{motion} {seed}: device vs restatement: rotation {fig[0]:.3e} deg, translation {fig[1]:.3e} deg, cost {fig[2]:.3e} relative, "
          f"r^2 {fig[3]:.3e} thr^2; steps {int(info['steps'])} / {o['steps']}, inliers {int(info['count'])} / {o['count']}, "
          f"{int(differ.sum())} mask entries differ, {int(band.sum())} matches within the band of thr^2; the start was "
          f"{_rot_deg(R0, o['R']):.4f} / {_angle_deg(t0, o['t']):.4f} deg away")
    assert int(info["steps"]) >= 1 and o["steps"] >= 1
    assert fig[0] <= PARITY_ROT_DEG and fig[1] <= PARITY_TRANS_DEG and fig[2] <= PARITY_COST_REL and fig[3] <= PARITY_R2_REL, fig
    assert not (differ & ~band).any()                        # masks differ only where r^2 is within the tolerance of thr^2
    assert abs(int(info["count"]) - o["count"]) <= int(band.sum())
    assert PR.rotation_error_deg(R, R_true) <= ROT_BOUND_DEG and PR.translation_error_deg(t, t_true) <= TRANS_BOUND_DEG


@pytest.mark.gpu
@pytest.mark.parametrize("motion", MOTIONS)
def test_estimate_relative_pose_with_two_cameras(motion):
    """estimate_relative_pose takes fx, fy, cx, cy per camera, no skew: the scene is made with the skew of both K set to 0"""
    from roma_amd import geometry
    Ka, Kb = GS.no_skew(KA), GS.no_skew(KB)
    cam0 = {"model": "PINHOLE", "width": GS.W_A, "height": GS.H_A, "params": [Ka[0, 0], Ka[1, 1], Ka[0, 2], Ka[1, 2]]}
    cam1 = {"model": "PINHOLE", "width": GS.W_B, "height": GS.H_B, "params": [Kb[0, 0], Kb[1, 1], Kb[0, 2], Kb[1, 2]]}
    thr = RR.calibrated_threshold(1.5, cam0, cam1)
    assert abs(thr - THR_G) < 1e-18 and abs(thr - 1.5 / 805) > 1e-4 and abs(thr - 1.5 / 632.5) > 1e-4
    xa, xb, truth, R_true, t_true = GS.general_scene(motion, 0, KA=Ka, KB=Kb)
    a, b = dev(xa).float(), dev(xb).float()
    pose, info = geometry.estimate_relative_pose(a, b, cam0, cam1, {"max_epipolar_error": 1.5, "max_iterations": 500}, seed=4)
    R0, t0, _ = geometry.estimate_pose(a, b, Ka, Kb, thr, max_iters=500, seed=4)
    R1, t1, mask1, info1 = geometry.refine_pose(R0, t0, a, b, Ka, Kb, thr, return_info=True)
    assert torch.equal(info["inliers"], mask1) and torch.equal(pose.R, R1) and torch.equal(pose.t, t1)
    assert int(info["num_inliers"]) == int(mask1.sum()) and torch.equal(info["model_score"], info1["cost"])
    R0, t0, R, t, mask = to_np(R0, t0, pose.R, pose.t, info["inliers"])
    xa32, xb32 = xa.astype(np.float32).astype(np.float64), xb.astype(np.float32).astype(np.float64)
    c0, c1 = _cost(R0, t0, xa32, xb32, Ka, Kb, thr), _cost(R, t, xa32, xb32, Ka, Kb, thr)
    assert c1 <= c0, (c0, c1)
    _assert_pose(R, t)
    er, et = PR.rotation_error_deg(R, R_true), PR.translation_error_deg(t, t_true)
    rec, prec = G.recall_precision(mask, truth)
    print(f"{motion}: estimate_relative_pose {er:.4f} / {et:.4f} deg (rotation / translation), {int(info['refinements'])} steps, "
          f"cost {c0:.6e} -> {c1:.6e}, inliers recall {rec:.4f} precision {prec:.4f}")
    assert er <= ROT_BOUND_DEG and et <= TRANS_BOUND_DEG and np.dot(t, t_true) > 0
    assert rec >= 0.98 and prec >= 0.98


BATCH = [(m, 0) for m in MOTIONS] + [("forward", 1), ("turn", 1)]


def _batch_cameras():
    """pair p: K_A scaled by 1 + 0.03 p, K_B by 1 - 0.03 p (last row kept)"""
    s = np.ones((3, 1))
    Kas, Kbs = [], []
    for p in range(len(BATCH)):
        s[:2, 0] = 1 + 0.03 * p
        Kas.append(KA * s)
        s[:2, 0] = 1 - 0.03 * p
        Kbs.append(KB * s)
    return np.stack(Kas), np.stack(Kbs)


@functools.lru_cache(maxsize=None)
def _batch_scenes():
    Kas, Kbs = _batch_cameras()
    return [GS.general_scene(m, s, KA=Kas[p], KB=Kbs[p]) for p, (m, s) in enumerate(BATCH)], Kas, Kbs


@pytest.mark.gpu
def test_batch_with_intrinsics_of_its_own_per_pair():
    from roma_amd import geometry
    scenes, Kas, Kbs = _batch_scenes()
    a, b = dev(np.stack([s[0] for s in scenes])).float(), dev(np.stack([s[1] for s in scenes])).float()
    E, emask = geometry.find_essential(a, b, dev(Kas), dev(Kbs), THR_G, max_iters=500, seed=5)
    R, t, mask = geometry.estimate_pose(a, b, dev(Kas), dev(Kbs), THR_G, max_iters=500, seed=5)
    assert R.shape == (6, 3, 3) and t.shape == (6, 3) and mask.shape == (6, 2000)
    for p, (motion, seed) in enumerate(BATCH):
        _check_pose(scenes[p][3], scenes[p][4], *to_np(emask[p], R[p], t[p], mask[p]), scenes[p][2], f"pair {p} ({motion} {seed})")
    # pair 0 alone, with its own cameras, is what it is in the batch (a later pair draws other samples: the draw counts pairs)
    E1, m1 = geometry.find_essential(a[0], b[0], Kas[0], Kbs[0], THR_G, max_iters=500, seed=5)
    assert torch.equal(E1, E[0]) and torch.equal(m1, emask[0])
    R2, t2, mask2 = geometry.refine_pose(R, t, a, b, dev(Kas), dev(Kbs), THR_G)
    for p in range(6):
        xa32, xb32 = a[p].double().cpu().numpy(), b[p].double().cpu().numpy()
        c0 = _cost(*to_np(R[p], t[p]), xa32, xb32, Kas[p], Kbs[p], THR_G)
        c1 = _cost(*to_np(R2[p], t2[p]), xa32, xb32, Kas[p], Kbs[p], THR_G)
        assert c1 <= c0, (p, c0, c1)
        assert PR.rotation_error_deg(R2[p].cpu().numpy(), scenes[p][3]) <= ROT_BOUND_DEG
        assert PR.translation_error_deg(t2[p].cpu().numpy(), scenes[p][4]) <= TRANS_BOUND_DEG


@pytest.mark.gpu
def test_three_chunks_return_what_one_chunk_returns(monkeypatch):
    from roma_amd import geometry
    scenes, Kas, Kbs = _batch_scenes()
    a, b = dev(np.stack([s[0] for s in scenes])).float(), dev(np.stack([s[1] for s in scenes])).float()
    planar = [GS.general_planar_scene(s) for s in range(6)]
    ha, hb = dev(np.stack([s[0] for s in planar])), dev(np.stack([s[1] for s in planar]))
    Ka, Kb = dev(Kas), dev(Kbs)
    calls = [(geometry.KIND_E, lambda: geometry.find_essential(a, b, Ka, Kb, THR_G, max_iters=500, seed=5)),
             (geometry.KIND_F, lambda: geometry.find_fundamental(a, b, threshold=1.5, max_iters=500, seed=5)),
             (geometry.KIND_H, lambda: geometry.find_homography(ha, hb, threshold=3.0, max_iters=500, seed=5))]
    for kind, call in calls:
        assert geometry._chunks(kind, 6, 2000, 500) == [(0, 6)]
        one = call()
        per_pair, _ = geometry.workspace_layout(kind, 1, 2000, 500)
        with monkeypatch.context() as mp:
            mp.setattr(geometry, "_WORKSPACE_LIMIT", 2 * per_pair + per_pair // 2)
            assert geometry._chunks(kind, 6, 2000, 500) == [(0, 2), (2, 4), (4, 6)]
            three = call()
        assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1]), kind
        assert bool(one[0].flatten(1).any(1).all()) and int(one[1].sum(1).min()) > 1000, kind    # and every pair has a model
    for p in range(6):
        assert G.corner_error(one[0][p].cpu().numpy(), planar[p][3]) <= 1.0, p


@pytest.mark.gpu
def test_a_singular_k_b_gives_the_identity_pose():
    from roma_amd import geometry
    eye, zero = torch.eye(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    xa, xb = GS.general_scene("sideways", 3, N=500)[:2]
    singular = dev(KB).clone()
    singular[1, 1] = 0.0
    E, emask = geometry.find_essential(dev(xa), dev(xb), dev(KA), singular, THR_G, max_iters=100, seed=0)
    assert torch.equal(E, torch.zeros_like(E)) and not bool(emask.any())
    R, t, mask = geometry.estimate_pose(dev(xa), dev(xb), dev(KA), singular, THR_G, max_iters=100, seed=0)
    assert torch.equal(R, eye) and torch.equal(t, zero) and not bool(mask.any())
    r = geometry.score_hypotheses(dev(xa), dev(xb), "essential", THR_G, 100, 0, dev(KA), singular)
    assert not bool(r["valid"].any()) and bool((r["samples"] == -1).all())
    E, emask = geometry.find_essential(dev(xa), dev(xb), dev(KA), dev(KB), THR_G, max_iters=100, seed=0)   # and the regular pair has one
    assert bool(E.any()) and int(emask.sum()) > 300


def _assert_transforms(r, xa, xb):
    """T_A, T_B of score_hypotheses are the Hartley transforms of image A and of image B (which differ here)"""
    ok = G.usable(xa, xb)
    for key, x in (("T_A", xa), ("T_B", xb)):
        want = G.transform(G.normalisation(x, ok))
        assert np.abs(r[key][0].cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max(), key
    assert G.normalisation(xb, ok)[2] > 1.2 * G.normalisation(xa, ok)[2]      # image B is smaller: exchanged transforms would show


@pytest.mark.gpu
def test_minimal_f_and_h_models_match_numpy_with_unequal_images():
    """test_minimal_models_match_numpy_fp64 of tests/test_geometry.py on the forward scene and the planar one"""
    from roma_amd import geometry
    xa, xb = GS.general_scene("forward", 5, N=600)[:2]
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "fundamental", 1.5, max_iters=400, seed=7)
    _assert_transforms(r, xa, xb)
    TA, TB = to_np(r["T_A"][0], r["T_B"][0])
    xh, xh2 = TG._normalised(xa, xb, TA, TB)
    models, valid, samples = to_np(r["models"][0], r["valid"][0], r["samples"][0])
    checked = 0
    for h in range(400):
        if samples[h, 0] < 0:
            assert not valid[h].any()
            continue
        want, co, cond = G.seven_point(xh[samples[h]], xh2[samples[h]])
        if cond > 1e6:
            continue
        if G.cubic_discriminant_rel(*co) > 1e-9:          # a well-conditioned sample is never rejected, and no root is lost
            assert valid[h].sum() == len(want), (h, valid[h], len(want))
        for r_ in range(3):
            if valid[h, r_]:
                d = min(np.abs(G.sign_fixed(models[h, r_]) - G.sign_fixed(w)).max() for w in want)
                assert d < 1e-6, (h, r_, d)
                checked += 1
    assert checked > 300
    xa, xb = GS.general_planar_scene(5, N=600)[:2]
    rh = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "homography", 3.0, max_iters=400, seed=8)
    _assert_transforms(rh, xa, xb)
    TA, TB = to_np(rh["T_A"][0], rh["T_B"][0])
    xh, xh2 = TG._normalised(xa, xb, TA, TB)
    models, valid, samples = to_np(rh["models"][0], rh["valid"][0], rh["samples"][0])
    checked = 0
    for h in range(400):
        if samples[h, 0] < 0:
            continue
        s = samples[h]
        if G.collinear(xh[s]) or G.collinear(xh2[s]):
            assert not valid[h, 0]
            continue
        want, cond = G.four_point(xh[s], xh2[s])
        if cond > 1e6:
            continue
        assert valid[h, 0], h                              # a well-conditioned, non-collinear sample is never rejected
        assert np.abs(G.sign_fixed(models[h, 0]) - G.sign_fixed(want)).max() < 1e-6, h
        checked += 1
    assert checked > 300


@pytest.mark.gpu
@pytest.mark.parametrize("model,thr", [("fundamental", 1.5), ("homography", 3.0)])
def test_f_and_h_selection_and_local_optimisation_with_unequal_images(model, thr):
    """test_selection_and_local_optimisation of tests/test_geometry.py: the de-normalisation is T_B^T F T_A / T_B^-1 H T_A"""
    from roma_amd import geometry
    xa, xb = (GS.general_scene("turn", 13) if model == "fundamental" else GS.general_planar_scene(13))[:2]
    fn = geometry.find_fundamental if model == "fundamental" else geometry.find_homography
    r = geometry.score_hypotheses(dev(xa), dev(xb), model, thr, max_iters=500, seed=21)
    _assert_transforms(r, xa, xb)
    best = int(np.argmin(r["cost"][0].cpu().numpy().reshape(-1)))
    slot = r["models"][0].cpu().numpy().reshape(-1, 3, 3)[best]
    ok = G.usable(xa, xb)
    want = G.finish(model, G.denormalise(model, slot, G.transform(G.normalisation(xa, ok)), G.transform(G.normalisation(xb, ok))))
    M0, mask0 = fn(dev(xa), dev(xb), threshold=thr, max_iters=500, seed=21, lo_iters=0)
    M0 = M0.cpu().numpy()
    assert np.abs(M0 - want).max() <= 1e-9 * np.abs(want).max(), (M0, want)
    t2 = thr * thr

    def msac(M):
        e = G.errors(model, M, xa, xb)
        return np.where(e < t2, e, t2).sum()
    M3, _ = fn(dev(xa), dev(xb), threshold=thr, max_iters=500, seed=21, lo_iters=3)
    assert msac(M3.cpu().numpy()) < msac(M0), (msac(M3.cpu().numpy()), msac(M0))


@pytest.mark.gpu
@pytest.mark.parametrize("motion", ["forward", "turn"])
def test_fundamental_of_two_cameras(motion):
    from roma_amd import geometry
    xa, xb, truth = GS.general_scene(motion, 0)[:3]
    ca, cb = GS.general_scene(motion, 0, sigma=0.0)[:2]
    M, mask = geometry.find_fundamental(dev(xa).float(), dev(xb).float(), threshold=1.5, max_iters=500, seed=1)
    assert M.shape == (3, 3) and M.dtype == torch.float64 and mask.shape == (2000,) and mask.dtype == torch.bool
    TG._check_two_view(M.cpu().numpy(), mask.cpu().numpy(), truth, ca, cb)


@pytest.mark.gpu
def test_homography_between_unequal_images():
    from roma_amd import geometry
    xa, xb, truth, H = GS.general_planar_scene(0)
    M, mask = geometry.find_homography(dev(xa), dev(xb), threshold=3.0, max_iters=500, seed=2)
    assert M.shape == (3, 3) and M.dtype == torch.float64 and float(M[2, 2]) == 1.0
    TG._check_planar(M.cpu().numpy(), mask.cpu().numpy(), truth, H)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", ["turn", "forward"])
def test_fundamental_refine_parity_with_unequal_images(motion):
    """test_refine_parity_with_the_restatement of tests/test_fundamental_refine.py: on the turn with its bounds as they stand, on the
    forward scene with model and cost bounds from the restatement's own movement (header)"""
    from roma_amd import geometry
    bound_model, bound_cost = (TF.PARITY_MODEL, TF.PARITY_COST_REL) if motion == "turn" else (10 * REF_F_MODEL, 10 * REF_F_COST_REL)
    xa, xb = GS.general_scene(motion, 0)[:2]
    F0, _ = geometry.find_fundamental(dev(xa), dev(xb), threshold=TF.THR, max_iters=TF.SAMPLES, seed=0)
    F, mask, info = geometry.refine_fundamental(F0, dev(xa), dev(xb), TF.THR, return_info=True)
    F0, F, mask = to_np(F0, F, mask)
    o = FR.refine(F0, xa, xb, TF.THR)
    TF._assert_output(F0, F, mask, info, xa, xb)
    r2d, r2n = FR.residuals(F, xa, xb) ** 2, FR.residuals(o["F"], xa, xb) ** 2
    fig = np.array([np.linalg.norm(F - o["F"]), abs(float(info["cost"]) - o["cost"]) / o["cost"], np.abs(r2d - r2n).max() / TF.THR ** 2])
    differ = mask != o["mask"]
    print(f"{motion}: device vs restatement: |dF| {fig[0]:.3e}, cost {fig[1]:.3e} relative, r^2 {fig[2]:.3e} thr^2; steps {int(info['steps'])} / "
          f"{o['steps']}, inliers {int(info['count'])} / {o['count']}, {int(differ.sum())} mask entries differ; cost {o['cost0']:.4f} -> "
          f"{o['cost']:.4f}")
    assert fig[0] <= bound_model and fig[1] <= bound_cost and fig[2] <= TF.PARITY_R2_REL, fig
    assert int(info["steps"]) == o["steps"] >= 1 and int(info["count"]) == o["count"]
    assert not (differ & ~(np.abs(r2n - TF.THR ** 2) <= TF.PARITY_R2_REL * TF.THR ** 2)).any()


@pytest.mark.gpu
def test_homography_refine_parity_with_unequal_images():
    """one case of test_refine_parity_with_the_restatement of tests/test_homography_refine.py, its bounds as they stand"""
    from roma_amd import geometry
    xa, xb = GS.general_planar_scene(0)[:2]
    H0, _ = geometry.find_homography(dev(xa), dev(xb), threshold=TH.THR, max_iters=TH.SAMPLES, seed=0)
    H, mask, info = geometry.refine_homography(H0, dev(xa), dev(xb), TH.THR, return_info=True)
    H0, H, mask = to_np(H0, H, mask)
    o = HR.refine(H0, xa, xb, TH.THR)
    TH._assert_output(H0, H, mask, info, xa, xb)
    ed, en = (HR.residuals(H, xa, xb) ** 2).sum(-1), (HR.residuals(o["H"], xa, xb) ** 2).sum(-1)
    fig = np.array([np.linalg.norm(H - o["H"]) / np.linalg.norm(o["H"]), abs(float(info["cost"]) - o["cost"]) / o["cost"],
                    np.abs(ed - en).max() / TH.THR ** 2])
    differ = mask != o["mask"]
    print(f"device vs restatement: |dH| / |H| {fig[0]:.3e}, cost {fig[1]:.3e} relative, e {fig[2]:.3e} thr^2; steps {int(info['steps'])} / "
          f"{o['steps']}, inliers {int(info['count'])} / {o['count']}, {int(differ.sum())} mask entries differ; cost {o['cost0']:.4f} -> "
          f"{o['cost']:.4f}")
    assert fig[0] <= TH.PARITY_MODEL and fig[1] <= TH.PARITY_COST_REL and fig[2] <= TH.PARITY_E_REL, fig
    assert int(info["steps"]) == o["steps"] >= 1 and int(info["count"]) == o["count"]
    assert not (differ & ~(np.abs(en - TH.THR ** 2) <= TH.PARITY_E_REL * TH.THR ** 2)).any()
