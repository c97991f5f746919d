"""roma_amd.geometry: RANSAC for fundamental matrices and homographies (csrc/geometry.hip), against the numpy restatement in
tests/geometry_ref.py.  CPU tests pin the restatement and the C-ABI argument checks; GPU tests pin the kernels."""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import geometry_ref as G
from tests.helpers import dev

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_ransac_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    rc = lib.roma_ransac_hypotheses(0, None, None, 1, 100, 10, 3.0, 0, 0, None, 0, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_ransac_hypotheses: null pointer" in lib.roma_last_error()
    rc = lib.roma_ransac_select(1, None, None, 1, 100, 10, 3.0, 3, None, 0, None, None, None)
    assert rc == _lib.ROMA_E_ARG and b"roma_ransac_select: null pointer" in lib.roma_last_error()
    buf = (ctypes.c_double * 16)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.roma_ransac_hypotheses(0, a, a, 1, 6, 10, 3.0, 0, 0, a, 1 << 40, None)            # N = 6 < 7
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 7" in lib.roma_last_error()
    rc = lib.roma_ransac_hypotheses(1, a, a, 1, 3, 10, 3.0, 0, 0, a, 1 << 40, None)            # N = 3 < 4
    assert rc == _lib.ROMA_E_SHAPE and b"need at least 4" in lib.roma_last_error()
    rc = lib.roma_ransac_hypotheses(0, a, a, 0, 100, 10, 3.0, 0, 0, a, 1 << 40, None)          # P = 0
    assert rc == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    rc = lib.roma_ransac_hypotheses(2, a, a, 1, 100, 10, 3.0, 0, 0, a, 1 << 40, None)          # unknown kind
    assert rc == _lib.ROMA_E_ARG and b"kind" in lib.roma_last_error()
    need = lib.roma_ransac_workspace(0, 1, 100, 10, None)
    assert need > 0
    rc = lib.roma_ransac_hypotheses(0, a, a, 1, 100, 10, 3.0, 0, 0, a, need - 1, None)         # workspace too small
    assert rc == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    rc = lib.roma_ransac_select(0, a, a, 1, 100, 10, -1.0, 3, a, need, a, a, None)              # threshold <= 0
    assert rc == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    assert lib.roma_ransac_workspace(5, 1, 100, 10, None) < 0


def test_chunk_plan_of_a_megadepth_batch_fits_in_256_mb():
    """P = 64, N = 10 000, 10 000 F samples: the chunks cover the batch, and the one workspace (sized for the widest chunk, shared
    by all) plus the fp64 copies of the inputs and the outputs stay under 256 MB.  test_megadepth_batch_fits_in_256_mb measures it."""
    from roma_amd import geometry
    P, N, iters = 64, 10000, 10000
    chunks = geometry._chunks(geometry.KIND_F, P, N, iters)
    assert [a for a, _ in chunks] == [0] + [b for _, b in chunks[:-1]] and chunks[-1][1] == P
    ws, _ = geometry.workspace_layout(geometry.KIND_F, max(b - a for a, b in chunks), N, iters)
    assert ws <= geometry._WORKSPACE_LIMIT
    assert ws + 2 * P * N * 2 * 8 + P * 9 * 8 + 2 * P * N < 256e6


def test_find_fundamental_refuses_cpu_tensors():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_fundamental(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.find_homography(x, x)


def _exact_pair(seed, n):
    rng = np.random.default_rng(seed)
    xa, xb, truth, F, ca, cb = G.two_view_scene(seed, N=400, outlier_frac=0.0, sigma=0.0)
    return ca[:n], cb[:n], F


def test_numpy_seven_point_recovers_the_true_f_on_exact_data():
    for seed in range(5):
        xa, xb, F = _exact_pair(seed, 7)
        cA, cB = G.normalisation(xa, np.ones(7, bool)), G.normalisation(xb, np.ones(7, bool))
        TA, TB = G.transform(cA), G.transform(cB)
        xh, xh2 = (xa - cA[:2]) * cA[2], (xb - cB[:2]) * cB[2]
        models, _, _ = G.seven_point(xh, xh2)
        assert 1 <= len(models) <= 3
        Fs = [G.sign_fixed(G.denormalise("fundamental", m, TA, TB)) for m in models]
        errs = [np.abs(f - F).max() for f in Fs]
        best = int(np.argmin(errs))
        assert errs[best] < 1e-9, errs
        hb = np.concatenate([xh2, np.ones((7, 1))], -1)
        ha = np.concatenate([xh, np.ones((7, 1))], -1)
        for m in models:                                  # every root satisfies the 7 epipolar constraints
            assert np.abs(np.einsum("ni,ij,nj->n", hb, m, ha)).max() < 1e-12
            assert abs(np.linalg.det(m)) < 1e-12


def test_numpy_four_point_recovers_h():
    for seed in range(5):
        xa, xb, truth, H = G.planar_scene(seed, N=50, outlier_frac=0.0, sigma=0.0)
        m, _ = G.four_point(xa[:4], xb[:4])
        m = m / m[2, 2]
        assert np.abs(m - H).max() / np.abs(H).max() < 1e-9


def test_numpy_sample_draw_redraws_repeats():
    xa = np.random.default_rng(0).uniform(0, 100, (2, 7, 2))
    idx = G.minimal_samples(xa, xa, "fundamental", 200, 5)
    valid = idx[..., 0] >= 0
    # N = 7: every valid sample is a permutation.  The last index misses all 16 attempts with probability (6/7)^16 = 0.085, the
    # one before with (5/7)^16 = 0.005: about 91 % of the samples are valid (400 here: one standard deviation is 1.4 %)
    assert valid.mean() > 0.85
    assert all(sorted(r) == list(range(7)) for r in idx[valid])
    xa[0, 3] = np.nan                                      # a non-finite match is never drawn
    idx = G.minimal_samples(xa, xa, "homography", 200, 5)
    assert not (idx[0] == 3).any() and (idx[0, :, 0] >= 0).any()


def test_numpy_restatement_meets_the_two_view_criteria():
    xa, xb, truth, F, ca, cb = G.two_view_scene(1)
    M, mask = G.ransac("fundamental", xa, xb, 1.5, 1000, seed=3)
    _check_two_view(M, mask, truth, ca, cb)


def test_numpy_restatement_meets_the_planar_criteria():
    xa, xb, truth, H = G.planar_scene(2)
    M, mask = G.ransac("homography", xa, xb, 3.0, 1000, seed=4)
    _check_planar(M, mask, truth, H)


def _check_two_view(M, mask, truth, ca, cb):
    rec, prec = G.recall_precision(mask, truth)
    assert rec >= 0.98 and prec >= 0.98, (rec, prec)
    d = np.sqrt(G.errors("fundamental", M, ca[truth], cb[truth]))
    assert np.median(d) <= 0.2, np.median(d)
    s = np.linalg.svd(M / np.linalg.norm(M), compute_uv=False)
    assert s[2] / s[0] < 1e-12, s


def _check_planar(M, mask, truth, H):
    rec, prec = G.recall_precision(mask, truth)
    assert rec >= 0.98 and prec >= 0.98, (rec, prec)
    assert G.corner_error(M, H) <= 1.0, G.corner_error(M, H)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 8, 5000])
def test_sample_indices_equal_the_restatement(N):
    from roma_amd import geometry
    rng = np.random.default_rng(N)
    xa, xb = rng.uniform(0, 1000, (3, N, 2)), rng.uniform(0, 1000, (3, N, 2))
    for model in ("fundamental", "homography"):
        for seed in (0, 123456789):
            got = geometry.minimal_samples(dev(xa), dev(xb), model, max_iters=300, seed=seed).cpu().numpy()
            want = G.minimal_samples(xa, xb, model, 300, seed)
            assert np.array_equal(got, want), (model, seed)
    if N == 7:                                             # every valid F sample is a permutation of the 7: redraws were needed
        got = geometry.minimal_samples(dev(xa), dev(xb), "fundamental", max_iters=300, seed=0).cpu().numpy().reshape(-1, 7)
        assert (got[:, 0] >= 0).mean() > 0.85 and all(sorted(r) == list(range(7)) for r in got if r[0] >= 0)


def _normalised(xa, xb, TA, TB):
    ha = np.concatenate([xa, np.ones_like(xa[..., :1])], -1) @ TA.T
    hb = np.concatenate([xb, np.ones_like(xb[..., :1])], -1) @ TB.T
    return ha[..., :2], hb[..., :2]


@pytest.mark.gpu
def test_minimal_models_match_numpy_fp64():
    from roma_amd import geometry
    xa, xb, _, _, _, _ = G.two_view_scene(5, N=600, outlier_frac=0.3)
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "fundamental", 1.5, max_iters=400, seed=7)
    TA, TB = r["T_A"][0].cpu().numpy(), r["T_B"][0].cpu().numpy()
    xh, xh2 = _normalised(xa, xb, TA, TB)
    models, valid, samples = r["models"][0].cpu().numpy(), r["valid"][0].cpu().numpy(), r["samples"][0].cpu().numpy()
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
    rh = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), "homography", 3.0, max_iters=400, seed=8)
    TA, TB = rh["T_A"][0].cpu().numpy(), rh["T_B"][0].cpu().numpy()
    xh, xh2 = _normalised(xa, xb, TA, TB)
    models, valid, samples = rh["models"][0].cpu().numpy(), rh["valid"][0].cpu().numpy(), rh["samples"][0].cpu().numpy()
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
def test_inlier_counts_equal_an_fp64_recount(model, thr):
    from roma_amd import geometry
    if model == "fundamental":
        xa, xb = G.two_view_scene(6, N=3000)[:2]
    else:
        xa, xb = G.planar_scene(6, N=3000)[:2]
    xa[17] = np.nan                                       # a non-finite match: never an inlier
    r = geometry.score_hypotheses(dev(xa[None]), dev(xb[None]), model, thr, max_iters=200, seed=9)
    TA, TB = r["T_A"][0].cpu().numpy(), r["T_B"][0].cpu().numpy()
    models, valid, count = r["models"][0].cpu().numpy(), r["valid"][0].cpu().numpy(), r["count"][0].cpu().numpy()
    assert valid.sum() > 100
    t2 = thr * thr
    for h, s in zip(*np.nonzero(valid)):
        e = G.errors(model, G.denormalise(model, models[h, s], TA, TB), xa, xb)
        lo, hi = (e < t2 * (1 - 1e-3)).sum(), (e < t2 * (1 + 1e-3)).sum()
        assert lo <= count[h, s] <= hi, (h, s, lo, count[h, s], hi)
    assert (count[~valid] == 0).all() and np.isinf(r["cost"][0].cpu().numpy()[~valid]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model,thr,iters", [("fundamental", 1.5, 1000), ("homography", 3.0, 500)])
def test_selection_and_local_optimisation(model, thr, iters):
    """lo_iters = 0 returns the de-normalised lowest-cost slot of score_hypotheses (lowest slot on ties, as np.argmin); lo_iters = 3
    returns a model of strictly lower MSAC cost (fp64 recount): the least-squares refit is kept only when it improves."""
    from roma_amd import geometry
    xa, xb = (G.two_view_scene(13) if model == "fundamental" else G.planar_scene(13))[:2]
    fn = geometry.find_fundamental if model == "fundamental" else geometry.find_homography
    r = geometry.score_hypotheses(dev(xa), dev(xb), model, thr, max_iters=iters, seed=21)
    best = int(np.argmin(r["cost"][0].cpu().numpy().reshape(-1)))
    slot = r["models"][0].cpu().numpy().reshape(-1, 3, 3)[best]
    want = G.finish(model, G.denormalise(model, slot, r["T_A"][0].cpu().numpy(), r["T_B"][0].cpu().numpy()))
    M0, mask0 = fn(dev(xa), dev(xb), threshold=thr, max_iters=iters, seed=21, lo_iters=0)
    M0 = M0.cpu().numpy()
    assert np.abs(M0 - want).max() <= 1e-9 * np.abs(want).max(), (M0, want)
    t2 = thr * thr

    def msac(M):
        e = G.errors(model, M, xa, xb)
        return np.where(e < t2, e, t2).sum()
    M3, _ = fn(dev(xa), dev(xb), threshold=thr, max_iters=iters, seed=21, lo_iters=3)
    assert msac(M3.cpu().numpy()) < msac(M0), (msac(M3.cpu().numpy()), msac(M0))


@pytest.mark.gpu
def test_megadepth_batch_fits_in_256_mb():
    """The issue's memory bound, measured: P = 64 pairs of N = 10 000 matches, 10 000 F samples each, in one call."""
    from roma_amd import geometry
    g = torch.Generator().manual_seed(0)
    xa = (torch.rand(64, 10000, 2, generator=g) * 1000).to(DEV)
    xb = (torch.rand(64, 10000, 2, generator=g) * 1000).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    F, mask = geometry.find_fundamental(xa, xb, max_iters=10000, seed=0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"P = 64, N = 10 000, 10 000 samples: peak {peak / 1e6:.1f} MB above the inputs")
    assert peak < 256e6, peak
    assert F.shape == (64, 3, 3) and mask.shape == (64, 10000) and torch.isfinite(F).all()


@pytest.mark.gpu
def test_two_view_scene():
    from roma_amd import geometry
    xa, xb, truth, F, ca, cb = G.two_view_scene(11)
    M, mask = geometry.find_fundamental(dev(xa).float(), dev(xb).float(), threshold=1.5, seed=1)
    assert M.shape == (3, 3) and M.dtype == torch.float64 and mask.shape == (5000,) and mask.dtype == torch.bool
    _check_two_view(M.cpu().numpy(), mask.cpu().numpy(), truth, ca, cb)


@pytest.mark.gpu
def test_planar_scene():
    from roma_amd import geometry
    xa, xb, truth, H = G.planar_scene(12)
    M, mask = geometry.find_homography(dev(xa), dev(xb), threshold=3.0, seed=2)
    assert M.shape == (3, 3) and M.dtype == torch.float64 and float(M[2, 2]) == 1.0
    _check_planar(M.cpu().numpy(), mask.cpu().numpy(), truth, H)


@pytest.mark.gpu
def test_determinism_and_batch_independence():
    from roma_amd import geometry
    scenes = [G.two_view_scene(20 + i, N=2000) for i in range(8)]
    xa = dev(np.stack([s[0] for s in scenes])).float()
    xb = dev(np.stack([s[1] for s in scenes])).float()
    M1, m1 = geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=3000, seed=5)
    M2, m2 = geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=3000, seed=5)
    assert torch.equal(M1, M2) and torch.equal(m1, m2)
    other = [G.two_view_scene(40 + i, N=2000) for i in range(8)]
    xa2, xb2 = xa.clone(), xb.clone()
    for i in range(8):
        if i != 3:
            xa2[i], xb2[i] = dev(other[i][0]).float(), dev(other[i][1]).float()
    M3, m3 = geometry.find_fundamental(xa2, xb2, threshold=1.5, max_iters=3000, seed=5)
    assert torch.equal(M3[3], M1[3]) and torch.equal(m3[3], m1[3])
    H1, h1 = geometry.find_homography(xa, xb, max_iters=500, seed=6)
    H3, h3 = geometry.find_homography(xa2, xb2, max_iters=500, seed=6)
    assert torch.equal(H3[3], H1[3]) and torch.equal(h3[3], h1[3])


@pytest.mark.gpu
def test_degenerate_input_gives_a_zero_model():
    from roma_amd import geometry
    x = torch.full((500, 2), 123.5, device=DEV)
    for fn in (geometry.find_fundamental, geometry.find_homography):
        M, mask = fn(x, x.clone(), max_iters=200, seed=0)
        assert torch.equal(M, torch.zeros_like(M)) and not bool(mask.any())
    bad = torch.full((500, 2), float("nan"), device=DEV)
    M, mask = geometry.find_fundamental(bad, bad, max_iters=50, seed=0)
    assert torch.equal(M, torch.zeros_like(M)) and not bool(mask.any())


@pytest.mark.gpu
def test_argument_errors():
    from roma_amd import geometry
    x = torch.rand(6, 2, device=DEV)
    with pytest.raises(ValueError):
        geometry.find_fundamental(x, x)
    geometry.find_homography(x, x, max_iters=10, seed=0)
    with pytest.raises(ValueError):
        geometry.find_homography(x[:3], x[:3])
    with pytest.raises(ValueError):
        geometry.find_fundamental(torch.rand(100, 2, device=DEV), torch.rand(99, 2, device=DEV))
    with pytest.raises(ValueError):
        geometry.find_fundamental(torch.rand(100, 3, device=DEV), torch.rand(100, 3, device=DEV))


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    xa, xb = G.two_view_scene(30, N=3000)[:2]
    xa, xb = dev(xa).float(), dev(xb).float()
    eager = geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=2000, seed=11)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=2000, seed=11)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = geometry.find_fundamental(xa, xb, threshold=1.5, max_iters=2000, seed=11)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


@pytest.mark.gpu
def test_integration_with_match_and_sample():
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
    F, mask = geometry.find_fundamental(torch.stack(kA), torch.stack(kB), max_iters=1000, seed=0)
    assert F.shape == (2, 3, 3) and mask.shape == (2, 500)
    assert torch.isfinite(F).all()
