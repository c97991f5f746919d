"""MAGSAC++ scoring of roma_amd.geometry (scoring="magsac"; csrc/ransac_common.h) against the numpy restatement in
tests/magsac_ref.py.  CPU tests pin the tables, the argument checks, the restatement's accuracy criteria and the compiler's resource
report of the new kernel instantiations; GPU tests pin the kernels.

The accuracy cases (MR.CASES: N = 2000, generous thresholds) and their criterion — MAGSAC++ better than MSAC on at least 5 of the 6
scenes of a row — are those of DESIGN.md §3.4; the restatement gets 6 of 6 in every row."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import geometry_ref as G
from tests import magsac_ref as MR
from tests import pose_ref as PR
from tests.helpers import dev, kernel_resources

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = {"F": "fundamental", "H": "homography", "E": "essential"}
K = PR.K_SCENE


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_tables_equal_the_closed_forms():
    lib = _lib.load()
    loss, weight = np.zeros(1025, np.float32), np.zeros(1025, np.float32)
    assert lib.roma_magsac_table(loss.ctypes.data, weight.ctypes.data) == 0
    for got, closed in ((loss, MR.loss_closed), (weight, MR.weight_closed)):
        want = np.array([closed(j / 1024) for j in range(1025)])
        w32 = want.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(w32)).astype(np.float64)).all()      # 1 fp32 ulp
    assert loss[0] == 0.0 and loss[1024] == 1.0 and weight[0] == 1.0 and weight[1024] == 0.0
    assert (np.diff(loss) >= 0).all() and (np.diff(weight) <= 0).all()
    assert np.array_equal(loss.astype(np.float64), MR.LOSS_NODES) and np.array_equal(weight.astype(np.float64), MR.WEIGHT_NODES)
    assert lib.roma_magsac_table(None, weight.ctypes.data) == _lib.ROMA_E_ARG and b"roma_magsac_table: null pointer" in lib.roma_last_error()


def test_committed_table_header_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("gen_magsac_table", os.path.join(ROOT, "tools", "gen_magsac_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.OUT).read() == gen.render()


def test_ex_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 16)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    calls = {
        "roma_ransac_hypotheses_ex": lambda p, sc: lib.roma_ransac_hypotheses_ex(0, p, p, 1, 100, 10, 3.0, sc, 0, 0, p, big, None),
        "roma_ransac_select_ex": lambda p, sc: lib.roma_ransac_select_ex(1, p, p, 1, 100, 10, 3.0, sc, 3, p, big, p, p, None),
        "roma_essential_hypotheses_ex": lambda p, sc: lib.roma_essential_hypotheses_ex(p, p, p, p, 1, 100, 10, 1e-3, sc, 0, 0, p, big, None),
        "roma_essential_select_ex": lambda p, sc: lib.roma_essential_select_ex(p, p, p, p, 1, 100, 10, 1e-3, sc, 3, p, big, p, p, None),
    }
    for name, call in calls.items():
        for sc in (0, 1):
            assert call(None, sc) == _lib.ROMA_E_ARG and (name + ": null pointer").encode() in lib.roma_last_error(), name
        for bad in (2, -1):
            assert call(a, bad) == _lib.ROMA_E_ARG, name
            msg = lib.roma_last_error()
            assert (name + ": scoring").encode() in msg and f"got {bad}".encode() in msg, msg
    # the old entry points still name themselves
    assert lib.roma_ransac_hypotheses(0, None, None, 1, 100, 10, 3.0, 0, 0, None, 0, None) == _lib.ROMA_E_ARG
    assert b"roma_ransac_hypotheses: null pointer" in lib.roma_last_error()
    assert lib.roma_essential_select(None, None, None, None, 1, 100, 10, 1e-3, 3, None, 0, None, None, None) == _lib.ROMA_E_ARG
    assert b"roma_essential_select: null pointer" in lib.roma_last_error()


def test_unknown_scoring_raises_before_the_device_check():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500                                  # CPU tensors: "magsac" gets as far as the device check, "bogus" does not
    Kt = torch.from_numpy(K)
    cam = {"model": "PINHOLE", "params": [800.0, 800.0, 512.0, 384.0]}
    calls = [lambda s: geometry.find_fundamental(x, x, scoring=s), lambda s: geometry.find_homography(x, x, scoring=s),
             lambda s: geometry.find_essential(x, x, Kt, Kt, 1e-3, scoring=s), lambda s: geometry.estimate_pose(x, x, Kt, Kt, 1e-3, scoring=s),
             lambda s: geometry.estimate_pose_uncalibrated(x, x, Kt, Kt, 1.5, scoring=s),
             lambda s: geometry.estimate_relative_pose(x, x, cam, cam, scoring=s), lambda s: geometry.score_hypotheses(x, x, scoring=s)]
    for call in calls:
        with pytest.raises(ValueError, match="unknown scoring 'bogus'"):
            call("bogus")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call("magsac")
    with pytest.raises(TypeError):
        geometry.find_homography(x, x, 3.0, 2000, None, 3, "magsac")      # keyword-only


def _restatement(row, scene, threshold, scoring, hyp):
    xa, xb, _ = MR.case_scene(row, scene)
    _, iters, seed = MR.CASES[row]
    if row == "E":
        return MR.ransac_essential(xa, xb, K, K, threshold, iters, seed, scoring=scoring, hyp=hyp)
    return MR.ransac(MODEL[row], xa, xb, threshold, iters, seed, scoring=scoring, hyp=hyp)


def _wins(row, results):
    """results: scene -> {scoring: criteria}; asserts MAGSAC++ better on >= 5 of the 6 scenes for each criterion of the row"""
    for c in range(len(next(iter(results.values()))["msac"])):
        ms, mg = [r["msac"][c] for r in results.values()], [r["magsac"][c] for r in results.values()]
        print(f"{row} criterion {c}: MSAC " + " ".join(f"{v:.3f}" for v in ms) + " | MAGSAC++ " + " ".join(f"{v:.3f}" for v in mg))
        assert sum(g < m for g, m in zip(mg, ms)) >= 5, (row, c, ms, mg)


@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_restatement_meets_the_accuracy_criteria(row):
    thr, iters, seed = MR.CASES[row]
    results = {}
    for scene in MR.SCENES[row]:
        xa, xb, truth = MR.case_scene(row, scene)
        hyp = MR.hypotheses_essential(xa, xb, K, K, iters, seed) if row == "E" else MR.hypotheses(MODEL[row], xa, xb, iters, seed)
        results[scene] = {}
        for scoring in ("msac", "magsac"):
            M, mask = _restatement(row, scene, thr, scoring, hyp)
            results[scene][scoring] = MR.criteria(row, M, mask, xa, xb, truth)
            if scoring == "msac" and scene == MR.SCENES[row][0]:            # the restatement's MSAC is the existing reference
                want = PR.ransac_essential(xa, xb, K, K, thr, iters, seed) if row == "E" else G.ransac(MODEL[row], xa, xb, thr, iters, seed)
                assert np.abs(M - want[0]).max() < 1e-9 and np.array_equal(mask, want[1])      # to the rounding of the 9 x 9 product
    _wins(row, results)


def test_magsac_instantiations_use_no_scratch_and_spill_nothing():
    """The compiler's resource report of the MAGSAC++ instantiations (last template argument 1): no scratch, no spills, and the scoring
    kernel — its loss nodes in LDS beside the points — keeps the occupancy of its MSAC counterpart."""
    g, e = kernel_resources("geometry.hip"), kernel_resources("essential.hip")

    def one(kernels, pattern):
        hit = [k for k in kernels if re.search(pattern, k)]
        assert len(hit) == 1, (pattern, sorted(kernels))
        return kernels[hit[0]]
    new = {"score F": one(g, r"score_kernelILi0ELi1EE"), "score H": one(g, r"score_kernelILi1ELi1EE"),
           "select F": one(g, r"\d+select_kernelILi0ELi1EE"), "select H": one(g, r"\d+select_kernelILi1ELi1EE"),
           "score E": one(e, r"score_kernelILi0ELi1EE"), "select E": one(e, r"essential_select_kernelILi1EE")}
    for name, k in new.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
    for kind in (0, 1):
        msac, magsac = one(g, rf"score_kernelILi{kind}ELi0EE"), one(g, rf"score_kernelILi{kind}ELi1EE")
        assert magsac["Occupancy"] >= msac["Occupancy"], (kind, msac, magsac)
        assert magsac["LDS Size"] == msac["LDS Size"] + 4096, (msac, magsac)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _scene(row, seed, N):
    return (G.planar_scene(seed, N=N) if row == "H" else G.two_view_scene(seed, N=N))[:2]


_K_DEV = []


def _Kd():
    if not _K_DEV:                                            # once: no copy from the host inside a graph capture
        _K_DEV.append(dev(K))
    return _K_DEV[0]


def _kw(row):
    return {"K_A": _Kd(), "K_B": _Kd()} if row == "E" else {}


def _find(row, xa, xb, thr, iters, seed, **kw):
    from roma_amd import geometry
    if row == "E":
        return geometry.find_essential(xa, xb, _Kd(), _Kd(), thr, max_iters=iters, seed=seed, **kw)
    fn = geometry.find_fundamental if row == "F" else geometry.find_homography
    return fn(xa, xb, threshold=thr, max_iters=iters, seed=seed, **kw)


def _pixel_errors(row, r, models, xa, xb):
    """fp64 squared errors (..., N) of normalised / calibrated models (..., 3, 3) of a score_hypotheses result"""
    if row == "E":
        return G.errors("fundamental", models, PR.calibrate(xa, K), PR.calibrate(xb, K))
    TA, TB = r["T_A"][0].cpu().numpy(), r["T_B"][0].cpu().numpy()
    Ms = TB.T @ models @ TA if row == "F" else np.linalg.inv(TB) @ models @ TA
    return G.errors(MODEL[row], Ms, xa, xb)


@pytest.mark.gpu
@pytest.mark.parametrize("row,N", [("F", 8), ("F", 1025), ("F", 3000), ("H", 3000), ("E", 3000)])
def test_slot_costs_equal_an_fp64_recount(row, N):
    """cost64(e (1 - 1e-3)) (1 - 1e-5) <= cost <= cost64(e (1 + 1e-3)) (1 + 1e-5) for every valid slot: L is monotone, so this is the
    band test_inlier_counts_equal_an_fp64_recount grants the fp32 errors, plus the fp32 sum of a chunk.  N = 1025 leaves a chunk of one
    point, 3000 a ragged last chunk, 8 a single short one."""
    from roma_amd import geometry
    thr = MR.CASES[row][0]
    xa, xb = _scene(row, 6, N)
    bad = 17 if N > 17 else 3
    xa[bad] = np.nan                                          # a non-finite match: L = 1, never an inlier
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), MODEL[row], thr, max_iters=200, seed=9, scoring="magsac", **_kw(row))
    valid, count, cost = r["valid"][0].cpu().numpy(), r["count"][0].cpu().numpy(), r["cost"][0].cpu().numpy()
    assert valid.sum() > 100
    t2 = thr * thr
    e = _pixel_errors(row, r, r["models"][0].cpu().numpy()[valid], xa, xb)
    assert np.isnan(e[:, bad]).all()
    with np.errstate(invalid="ignore"):
        lo_n, hi_n = (e < t2 * (1 - 1e-3)).sum(-1), (e < t2 * (1 + 1e-3)).sum(-1)
    lo_c, hi_c = MR.cost(e * (1 - 1e-3), t2) * (1 - 1e-5), MR.cost(e * (1 + 1e-3), t2) * (1 + 1e-5)
    print(f"{row} N={N}: {valid.sum()} slots, worst (cost - lo) / cost {((cost[valid] - lo_c) / cost[valid]).min():.2e}, "
          f"worst (hi - cost) / cost {((hi_c - cost[valid]) / cost[valid]).min():.2e}")
    assert ((lo_n <= count[valid]) & (count[valid] <= hi_n)).all()
    assert ((lo_c <= cost[valid]) & (cost[valid] <= hi_c)).all()
    assert (count[~valid] == 0).all() and np.isinf(cost[~valid]).all()
    if N == 3000:                                             # the costs differ from the MSAC costs of the same slots
        r0 = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), MODEL[row], thr, max_iters=200, seed=9, **_kw(row))
        assert torch.equal(r0["count"], r["count"]) and torch.equal(r0["models"], r["models"])
        assert not torch.equal(r0["cost"], r["cost"])


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_selection_and_reweighted_local_optimisation(row):
    """lo_iters = 0 returns the de-normalised arg-min slot of the MAGSAC++ costs (lowest slot on ties, as np.argmin); lo_iters = 3
    returns a model whose fp64 MAGSAC++ cost is not higher — strictly lower where the restatement's re-weighted refit from that same
    slot is strictly lower.  F stays rank 2, E on the essential manifold."""
    from roma_amd import geometry
    thr, iters, _ = MR.CASES[row]
    xa, xb = _scene(row, 13, 2000)
    r = geometry.score_hypotheses(dev(xa), dev(xb), MODEL[row], thr, max_iters=iters, seed=21, scoring="magsac", **_kw(row))
    best = int(np.argmin(r["cost"][0].cpu().numpy().reshape(-1)))
    slot = r["models"][0].cpu().numpy().reshape(-1, 3, 3)[best]
    t2 = thr * thr
    if row == "E":
        xh, xh2 = PR.calibrate(xa, K), PR.calibrate(xb, K)
        want = G.sign_fixed(slot)
        ref, _ = MR.ransac_essential(xa, xb, K, K, thr, iters, 21, hyp=([slot], xh, xh2))

        def cost64(M):
            return MR.cost(G.errors("fundamental", M, xh, xh2), t2)
    else:
        TA, TB = r["T_A"][0].cpu().numpy(), r["T_B"][0].cpu().numpy()
        want = G.finish(MODEL[row], G.denormalise(MODEL[row], slot, TA, TB))
        ha = np.concatenate([xa, np.ones((len(xa), 1))], -1)
        hb = np.concatenate([xb, np.ones((len(xb), 1))], -1)
        ref, _ = MR.ransac(MODEL[row], xa, xb, thr, iters, 21, hyp=([slot], (ha @ TA.T)[:, :2], (hb @ TB.T)[:, :2], TA, TB))

        def cost64(M):
            return MR.cost(G.errors(MODEL[row], M, xa, xb), t2)
    M0, _ = _find(row, dev(xa), dev(xb), thr, iters, 21, lo_iters=0, scoring="magsac")
    M3, mask3 = _find(row, dev(xa), dev(xb), thr, iters, 21, lo_iters=3, scoring="magsac")
    M0, M3 = M0.cpu().numpy(), M3.cpu().numpy()
    assert np.abs(M0 - want).max() <= 1e-9 * np.abs(want).max(), (M0, want)
    print(f"{row}: MAGSAC++ cost of the best slot {cost64(M0):.6f}, after 3 rounds {cost64(M3):.6f}, restatement {cost64(ref):.6f}")
    assert cost64(M3) <= cost64(M0)
    if cost64(ref) < cost64(M0):
        assert cost64(M3) < cost64(M0)
    for M in (M0, M3):
        s = np.linalg.svd(M / np.linalg.norm(M), compute_uv=False)
        if row == "F":
            assert s[2] / s[0] < 1e-12, s
        if row == "E":
            assert abs(np.linalg.norm(M) - 1) < 1e-12 and abs(s[0] - s[1]) / s[0] < 1e-9 and s[2] / s[0] < 1e-12, s
            assert M.reshape(-1)[np.abs(M).argmax()] > 0
    e = G.errors("fundamental", M3, xh, xh2) if row == "E" else G.errors(MODEL[row], M3, xa, xb)
    m = mask3.cpu().numpy()
    assert ((e < t2 * (1 - 1e-3)) <= m).all() and (m <= (e < t2 * (1 + 1e-3))).all()          # mask = e < threshold^2, unchanged


def _batch(row, seeds, N=2000):
    scenes = [_scene(row, s, N) for s in seeds]
    return dev(np.stack([s[0] for s in scenes])), dev(np.stack([s[1] for s in scenes]))


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_msac_by_name_is_the_default_bit_for_bit(row):
    thr = MR.TIGHT[row]
    xa, xb = _batch(row, (20, 21, 22))
    M1, m1 = _find(row, xa, xb, thr, 300, 5)
    M2, m2 = _find(row, xa, xb, thr, 300, 5, scoring="msac")
    assert torch.equal(M1, M2) and torch.equal(m1, m2)
    M3, m3 = _find(row, xa, xb, thr, 300, 5, scoring="magsac")
    assert not torch.equal(M1, M3)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_device_meets_the_accuracy_criteria(row):
    """the cases of test_restatement_meets_the_accuracy_criteria on the device (a single pair draws what the restatement draws),
    against the device's own MSAC at the same arguments"""
    thr, iters, seed = MR.CASES[row]
    results = {}
    for scene in MR.SCENES[row]:
        xa, xb, truth = MR.case_scene(row, scene)
        results[scene] = {}
        for scoring in ("msac", "magsac"):
            M, mask = _find(row, dev(xa), dev(xb), thr, iters, seed, scoring=scoring)
            results[scene][scoring] = MR.criteria(row, M.cpu().numpy(), mask.cpu().numpy(), xa, xb, truth)
    _wins(row, results)


def _alone(row, xa, xb, p0, thr, iters, seed, lo_iters=3):
    """pair p0 of a batch through the *_ex entry points on its own: P = 1 with the pair offset p0"""
    from roma_amd import geometry
    from roma_amd.ops import _stream
    lib = _lib.load()
    N = xa.shape[0]
    kind = {"F": geometry.KIND_F, "H": geometry.KIND_H, "E": geometry.KIND_E}[row]
    total, _ = geometry.workspace_layout(kind, 1, N, iters)
    ws = torch.empty((total,), dtype=torch.uint8, device=DEV)
    M = torch.empty((3, 3), dtype=torch.float64, device=DEV)
    mask = torch.empty((N,), dtype=torch.uint8, device=DEV)
    a, b, k = xa.contiguous(), xb.contiguous(), _Kd()
    if row == "E":
        rc = lib.roma_essential_hypotheses_ex(a.data_ptr(), b.data_ptr(), k.data_ptr(), k.data_ptr(), 1, N, iters, thr, 1, seed, p0,
                                              ws.data_ptr(), total, _stream())
        assert rc == 0, lib.roma_last_error()
        rc = lib.roma_essential_select_ex(a.data_ptr(), b.data_ptr(), k.data_ptr(), k.data_ptr(), 1, N, iters, thr, 1, lo_iters,
                                          ws.data_ptr(), total, M.data_ptr(), mask.data_ptr(), _stream())
    else:
        rc = lib.roma_ransac_hypotheses_ex(kind, a.data_ptr(), b.data_ptr(), 1, N, iters, thr, 1, seed, p0, ws.data_ptr(), total, _stream())
        assert rc == 0, lib.roma_last_error()
        rc = lib.roma_ransac_select_ex(kind, a.data_ptr(), b.data_ptr(), 1, N, iters, thr, 1, lo_iters, ws.data_ptr(), total, M.data_ptr(),
                                       mask.data_ptr(), _stream())
    assert rc == 0, lib.roma_last_error()
    return M, mask.bool()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_magsac_determinism_and_batch_independence(row):
    thr = MR.CASES[row][0]
    xa, xb = _batch(row, (20, 21, 22))
    M1, m1 = _find(row, xa, xb, thr, 300, 5, scoring="magsac")
    M2, m2 = _find(row, xa, xb, thr, 300, 5, scoring="magsac")
    assert torch.equal(M1, M2) and torch.equal(m1, m2)
    for p in range(3):
        Mp, mp = _alone(row, xa[p], xb[p], p, thr, 300, 5)
        assert torch.equal(Mp, M1[p]) and torch.equal(mp, m1[p]), p
        assert bool(m1[p].any())


@pytest.mark.gpu
def test_magsac_degenerate_input_gives_a_zero_model():
    x = torch.full((500, 2), 123.5, device=DEV)
    bad = torch.full((500, 2), float("nan"), device=DEV)
    for row in ("F", "H", "E"):
        for a in (x, bad):
            M, mask = _find(row, a, a.clone(), MR.CASES[row][0], 100, 0, scoring="magsac")
            assert torch.equal(M, torch.zeros_like(M)) and not bool(mask.any())


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["F", "H", "E"])
def test_magsac_graph_capture_replays_the_eager_result(row):
    thr, iters, _ = MR.CASES[row]
    xa, xb = _scene(row, 30, 2000)
    xa, xb = dev(xa).float(), dev(xb).float()
    eager = _find(row, xa, xb, thr, iters, 11, scoring="magsac")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _find(row, xa, xb, thr, iters, 11, scoring="magsac")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _find(row, xa, xb, thr, iters, 11, scoring="magsac")
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert bool(out[1].any())


@pytest.mark.gpu
def test_pose_entry_points_pass_the_scoring_on():
    """estimate_pose / estimate_pose_uncalibrated / estimate_relative_pose with scoring="magsac" are their chains on find_essential /
    find_fundamental with that scoring (refine_iters and refine_pose compose unchanged behind it)."""
    from roma_amd import geometry
    xa, xb = G.two_view_scene(13, N=2000)[:2]
    xa, xb, k = dev(xa), dev(xb), _Kd()
    thr = MR.CASES["E"][0]
    E, emask = geometry.find_essential(xa, xb, k, k, thr, max_iters=200, seed=3, scoring="magsac")
    want = geometry.recover_pose(E, xa, xb, k, k, emask)
    got = geometry.estimate_pose(xa, xb, k, k, thr, max_iters=200, seed=3, scoring="magsac")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], geometry.estimate_pose(xa, xb, k, k, thr, max_iters=200, seed=3)[0])
    F, fmask = geometry.find_fundamental(xa, xb, threshold=6.0, max_iters=300, seed=3, refine_iters=5, scoring="magsac")
    want = geometry.recover_pose(k.T @ F @ k, xa, xb, k, k, fmask)
    got = geometry.estimate_pose_uncalibrated(xa, xb, k, k, 6.0, max_iters=300, seed=3, refine_iters=5, scoring="magsac")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    cam = {"model": "PINHOLE", "params": [800.0, 800.0, G.W_IMG / 2, G.H_IMG / 2]}
    opt = {"max_epipolar_error": 6.0, "max_iterations": 200}
    pose, info = geometry.estimate_relative_pose(xa, xb, cam, cam, opt, seed=3, scoring="magsac")
    thr = 6.0 * 0.5 * (1.0 / 800.0 + 1.0 / 800.0)                  # estimate_relative_pose's calibrated threshold, as it computes it
    R0, t0, _ = geometry.estimate_pose(xa, xb, k, k, thr, max_iters=200, seed=3, scoring="magsac")
    R, t, mask = geometry.refine_pose(R0, t0, xa, xb, k, k, thr)
    assert torch.equal(pose.R, R) and torch.equal(pose.t, t) and torch.equal(info["inliers"], mask)
    assert PR.rotation_error_deg(pose.R.cpu().numpy(), PR.scene_pose(13)[1]) < 0.5
