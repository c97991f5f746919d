"""roma_amd.geometry.average_rotations / global_positions / initialize_cameras (csrc/motion_average.hip) against the numpy restatement in
tests/motion_ref.py.

Scenes: tests/multiview_scenes.multiview_scene(V, SEED, N) — sigma = 0.5 px, 10 % outlier observations in views >= 1 — and the complete
pose graph made from its ground truth by motion_ref.pairwise: rodrigues(0.2 deg N(0,1)^3) on every pairwise rotation, rodrigues(0.5 deg
N(0,1)^3) on every translation direction, and for V >= 5 every edge with m % 7 == 3 an outlier (25 deg and 40 deg instead).  Threshold
4 px, 4 rounds, root 0.  SEED = 1: with seed 0 the V = 5 scene keeps 0.3 points too few observations, and with seed 2 its outlier edge is
65 deg off, more than the six L1 rounds of the default take back; both are the restatement's own behaviour.

Measured with the restatement (the CPU tests print the figures again and assert the relations):
  ROT_BOUND_DEG,   2 x the worst error over SCENES: the worst angle between R_v and R_true_v R_true_0^T, 0.317 deg (V = 3), and the worst
  CENTRE_BOUND     centre error after a scale-and-translation alignment relative to the extent of the true centres, 0.0135 (V = 5)
  MOTION_TOL       the restatement with the points summed in ascending, descending and shuffled order and with numpy.linalg.eigh against
                   its own cyclic Jacobi, over SCENES and EDGE_CASES without "cap": R, centres and the solved points differ by at most
                   3.87e-13 (the points at V = 3, where two of the three baselines are short); 10 x that.  Masks, solved flags and
                   status are identical across those runs
  CAP_TOL          the same for the case "cap" alone, N = 16 385 points in 3 views: 2.04e-11 (27 times as many terms in every sum, and
                   eigenvalues of 0.3 and 382); 10 x that
The two eigenvalues are held to a bound that is reasoned, not measured: a backward-stable symmetric eigen-solver of n rows returns
eigenvalues within about n eps |S|, and |S| <= tr S <= 2 sum w <= 2 count (each observation adds w (I - d d^T), of trace 2 w <= 2), so
the bound is 3 V eps 2 count — 4e-12 at V = 3 and 2e-10 at V = 32, of eigenvalues between 1e-3 and 15 (1.7e-10 of 382 at N = 16 385);
the restatement's runs differ by 2.3e-13 on the scenes and 2.5e-11 at N = 16 385."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import bundle_ref as B
from tests import motion_ref as MR
from tests import multiview_scenes as MS
from tests.helpers import kernel_resources

DEV = "cuda:0"
SEED = 1
THR = 4.0
SCENES = [(3, 600), (5, 600), (8, 600), (12, 600), (32, 400)]
BOUND_FACTOR = 2.0
ROT_BOUND_DEG, CENTRE_BOUND = 0.64, 0.027
MOTION_TOL = 3.87e-12
CAP_TOL = 2.04e-10
CHUNK, MAX_PARTIALS = 64, 256                       # points per workgroup and the cap of the partial sums (csrc/motion_average.hip)
RUNS = ((0, "eigh"), (1, "eigh"), (2, "eigh"), (0, "jacobi"))


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def problem(V, N, seed=SEED, outliers=None):
    """the scene, its pose graph, and the arguments of the calls: x, K, pairs, R_rel, t_rel, visible, weights"""
    s = MS.multiview_scene(V, seed, N)
    pairs, R_rel, t_rel, bad = MR.pairwise(s, seed, outliers)
    return _frozen(dict(s, pairs=pairs, R_rel=R_rel, t_rel=t_rel, bad=bad, visible=None, weights=None, root=0))


@functools.lru_cache(maxsize=None)
def variant(name):
    """the edge cases: a problem with something changed"""
    if name == "tiny":
        return problem(3, 2)
    if name == "seam":
        return problem(3, CHUNK + 1)
    if name == "wide":
        return problem(32, CHUNK)
    if name == "cap":
        return problem(3, CHUNK * MAX_PARTIALS + 1)
    if name == "root2":
        return _frozen(dict(problem(5, 600), root=2))
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in problem(6 if name == "components" else 5, 300).items()}
    if name == "components":                          # views 4 and 5 hang together but not on the rest
        keep = np.array([(a < 4) == (b < 4) for a, b in p["pairs"]])
        p.update(pairs=p["pairs"][keep], R_rel=p["R_rel"][keep], t_rel=p["t_rel"][keep], bad=p["bad"][keep])
    elif name == "visible":                           # the unseen pixels hold finite garbage and `visible` says so
        p["visible"] = np.isfinite(p["x"]).all(-1)
        p["x"] = np.where(p["visible"][..., None], p["x"], np.float32(123.0))
    elif name == "nan_rows":                          # an edge without a rotation, one without a translation, points nobody sees
        p["R_rel"][1, 1, 1] = np.nan
        p["t_rel"][5] = np.nan
        p["t_rel"][6] = 0.0
        p["x"][:, 7] = np.nan
        p["x"][1:, 8] = np.nan
    elif name == "duplicate":                         # edge 2 twice, and weights as inlier counts would be
        p["pairs"] = np.concatenate([p["pairs"], p["pairs"][2:3]])
        p["R_rel"] = np.concatenate([p["R_rel"], p["R_rel"][2:3]])
        p["t_rel"] = np.concatenate([p["t_rel"], p["t_rel"][2:3]])
        p["bad"] = np.concatenate([p["bad"], p["bad"][2:3]])
        p["weights"] = np.random.default_rng(5).integers(50, 500, len(p["pairs"])).astype(np.float64)
    elif name == "skew":                              # the same scene seen through cameras with a strong skew: the pixels move with K
        K2 = p["K"].copy()
        K2[:, 0, 1] += 25.0
        h = (p["x"].astype(np.float64) - p["K"][:, None, :2, 2])
        y = h[..., 1] / p["K"][:, None, 1, 1]
        p["x"] = (p["x"].astype(np.float64) + np.stack([25.0 * y, np.zeros_like(y)], -1)).astype(np.float32)
        p["K"] = K2
    else:
        raise KeyError(name)
    return _frozen(p)


EDGE_CASES = ["tiny", "seam", "wide", "cap", "components", "visible", "nan_rows", "duplicate", "skew", "root2"]


def _case(case):
    return variant(case) if isinstance(case, str) else problem(*case)


@functools.lru_cache(maxsize=None)
def restated(case, order=0, solver="eigh"):
    p = _case(case)
    V = len(p["x"])
    rot = MR.average_rotations(p["R_rel"], p["pairs"], V, p["weights"], p["root"])
    pos = MR.global_positions(p["x"], rot["R"], p["K"], p["pairs"], p["t_rel"], p["visible"], THR, 4, p["root"], order, solver)
    return _frozen(dict(pos, R=rot["R"], valid=rot["valid"], residual=rot["residual"], rotation_status=rot["status"], position_status=pos["status"]))


def _errors(r, p):
    return MR.rotation_error_deg(r["R"], p["R"], p["root"]), MR.centre_error(r["centres"], p["R"], p["t"], p["root"])


def _check_scene(r, p, what):
    """the scene criteria: both status words 0, the cameras within the truth-aware bounds, the mask keeps at least 1 - outlier share - 0.05
    of the seen observations and at most 2 % of it is outliers"""
    er, ec = _errors(r, p)
    seen = int(p["seen"].sum())
    share = p["outlier"].sum() / seen
    kept = r["mask"].sum() / seen
    wrong = (r["mask"] & p["outlier"]).sum() / max(int(r["mask"].sum()), 1)
    print(f"{what}: worst rotation error {er:.4f} deg, worst centre error {ec:.5f} of the extent, the mask keeps {kept:.4f} of the seen "
          f"observations (outlier share {share:.4f}), {wrong:.4f} of it outliers; eigenvalues {r['eigenvalues'][0]:.3e}, {r['eigenvalues'][1]:.3e}")
    assert r["rotation_status"] == 0 and r["position_status"] == 0
    assert r["count"] == r["mask"].sum()
    assert kept >= 1.0 - share - 0.05 and wrong <= 0.02, (kept, share, wrong)
    assert er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND, (er, ec)
    return er, ec


def _lambda_bound(r):
    """3 V eps 2 count (the module docstring)"""
    return 3 * len(r["R"]) * np.finfo(np.float64).eps * 2 * max(int(r["count"]), 1)


def _diff(a, b):
    """the largest difference in R, centres and points; the NaN patterns must agree"""
    worst = 0.0
    for k in ("R", "centres", "points"):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        if np.isfinite(a[k]).any():
            worst = max(worst, float(np.nanmax(np.abs(a[k] - b[k]))))
    return worst


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("V,N", SCENES)
def test_numpy_restatement_meets_the_scene_criteria(V, N):
    _check_scene(restated((V, N)), problem(V, N), f"restatement, V={V} N={N}")


def test_truth_aware_bounds_are_twice_the_worst_error_of_the_restatement():
    wr = wc = 0.0
    for case in SCENES:
        er, ec = _errors(restated(case), problem(*case))
        wr, wc = max(wr, er), max(wc, ec)
    print(f"restatement over {len(SCENES)} scenes: worst rotation error {wr:.4f} deg, worst centre error {wc:.5f}")
    assert BOUND_FACTOR * wr <= ROT_BOUND_DEG <= (BOUND_FACTOR + 0.1) * wr and BOUND_FACTOR * wc <= CENTRE_BOUND <= (BOUND_FACTOR + 0.1) * wc, (wr, wc)


def test_parity_tolerance_is_ten_times_the_order_of_the_sums_and_the_eigen_solver():
    """over every case the device is compared on; the masks, the solved flags and the status must not depend on either"""
    worst = lam = cap = 0.0
    for case in SCENES + EDGE_CASES:
        r = [restated(case, o, s) for o, s in RUNS]
        for q in r[1:]:
            assert np.array_equal(q["mask"], r[0]["mask"]) and np.array_equal(q["solved"], r[0]["solved"]) and q["status"] == r[0]["status"], case
            dl = float(np.abs(q["eigenvalues"] - r[0]["eigenvalues"]).max()) if r[0]["status"] == 0 else 0.0
            assert dl <= _lambda_bound(r[0]), (case, dl)
            lam = max(lam, dl)
            if case == "cap":
                cap = max(cap, _diff(q, r[0]))
            else:
                worst = max(worst, _diff(q, r[0]))
        print(f"  {case}: {max(_diff(q, r[0]) for q in r[1:]):.3e}")
    print(f"restatement, three orders of the sums and two eigen-solvers over {len(SCENES) + len(EDGE_CASES)} cases: R, centres, points differ by at most "
          f"{worst:.3e} (tolerance {MOTION_TOL:.2e}), at N = {CHUNK * MAX_PARTIALS + 1} by {cap:.3e} (tolerance {CAP_TOL:.2e}), the eigenvalues by {lam:.3e}")
    assert 0 < 10 * worst <= MOTION_TOL * 1.0001 and MOTION_TOL <= 11 * worst, worst
    assert 0 < 10 * cap <= CAP_TOL * 1.0001 and CAP_TOL <= 11 * cap, cap


def test_an_outlier_edge_in_the_spanning_tree():
    """V = 5, edge 3 = (0, 4) is an outlier and, with equal weights, part of the tree: the L1 rounds take it back out"""
    p = problem(5, 600, SEED, (3,))
    assert p["bad"].sum() == 1 and tuple(p["pairs"][3]) == (0, 4)
    start = MR.average_rotations(p["R_rel"], p["pairs"], 5, iters=0)
    r = restated((5, 600, SEED, (3,)))
    res = np.degrees(r["residual"])
    print(f"the tree alone: {MR.rotation_error_deg(start['R'], p['R']):.2f} deg; after 12 rounds: residual {res[3]:.2f} deg on the outlier edge, "
          f"at most {res[~p['bad']].max():.3f} deg on the others")
    assert MR.rotation_error_deg(start["R"], p["R"]) > 5.0 and np.degrees(start["residual"][3]) < 1e-6
    _check_scene(r, p, "restatement, one outlier edge")
    assert (res[p["bad"]] > 5.0).all() and (res[~p["bad"]] < 2.0).all()
    q = problem(5, 600)
    res = np.degrees(restated((5, 600))["residual"])
    assert (res[q["bad"]] > 5.0).all() and (res[~q["bad"]] < 2.0).all()


def test_restatement_on_the_edge_cases():
    r, p = restated("components"), variant("components")
    assert r["valid"].tolist() == [True] * 4 + [False] * 2 and np.isnan(r["R"][4:]).all() and np.isfinite(r["R"][:4]).all()
    assert r["position_status"] == MR.STATUS_UNPLACED and np.isnan(r["centres"][4:]).all() and not r["mask"][4:].any()
    assert np.isnan(r["residual"][-1]) and np.isfinite(r["residual"][:-1]).all()          # the edge (4, 5) is never reached
    er, ec = MR.rotation_error_deg(r["R"][:4], p["R"][:4]), MR.centre_error(r["centres"][:4], p["R"][:4], p["t"][:4])
    assert er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND, (er, ec)
    plain = restated((5, 300))
    r = restated("visible")
    assert np.array_equal(r["mask"], plain["mask"]) and _diff(r, plain) == 0.0
    r = restated("nan_rows")
    assert np.isnan(r["residual"][1]) and np.isfinite(r["residual"][5]) and np.isnan(r["points"][7:9]).all() and not r["mask"][:, 7:9].any()
    assert r["position_status"] == 0
    for case in ("duplicate", "skew", "root2", "nan_rows"):
        er, ec = _errors(restated(case), variant(case))
        assert er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND, (case, er, ec)
    # too little to work with: one track seen by one view only
    p = problem(3, 2)
    x = p["x"].copy()
    x[1:] = np.nan
    r = MR.global_positions(x, p["R"], p["K"], p["pairs"], p["t_rel"])
    assert r["status"] & MR.STATUS_TOO_FEW and np.isnan(r["centres"]).all() and r["count"] == 0


def test_motion_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    off = (ctypes.c_long * 11)()
    op = ctypes.cast(off, ctypes.c_void_p)
    for V, N, M in ((3, 1, 1), (3, 65, 3), (8, 1 << 14, 28), (32, 64, 496), (32, 1 << 17, 4096)):
        need = lib.roma_positions_workspace(V, N, M, op)
        assert need > 0 and lib.roma_positions_workspace(V, N, M, None) == need
        o = list(off)
        assert o[0] == 0 and all(b > a for a, b in zip(o, o[1:])) and all(v % 256 == 0 for v in o) and o[-1] < need and need % 256 == 0
        Ms, P = 3 * V * (3 * V + 1) // 2 + V, min(-(-N // CHUNK), MAX_PARTIALS)
        assert o[10] - o[9] >= 8 * Ms * P and o[9] - o[8] >= 8 * Ms and o[5] - o[4] >= 24 * N and o[4] - o[3] >= 48 * M
    assert lib.roma_positions_workspace(32, 1 << 17, 496, None) < 32 << 20
    for V, N, M in ((2, 64, 3), (33, 64, 3), (3, 0, 3), (3, (1 << 24) + 1, 3), (3, 64, 0), (3, 64, 4097)):
        assert lib.roma_positions_workspace(V, N, M, None) == _lib.ROMA_E_SHAPE and b"roma_positions_workspace: bad shape" in lib.roma_last_error()

    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 8)

    def rot(R_rel=a, pairs=a, weights=None, V=3, M=3, root=0, sigma=5.0, iters=12, R=a, valid=a, residual=a, status=a):
        return lib.roma_rotation_average(R_rel, pairs, weights, V, M, root, sigma, iters, R, valid, residual, status, None)

    for kw in ("R_rel", "pairs", "R", "valid", "residual", "status"):
        assert rot(**{kw: None}) == _lib.ROMA_E_ARG and b"roma_rotation_average: null pointer" in lib.roma_last_error()
    for V in (1, 33):
        assert rot(V=V) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
    for M in (0, 4097):
        assert rot(M=M) == _lib.ROMA_E_SHAPE and b"bad shape M=" in lib.roma_last_error()
    for root in (-1, 3):
        assert rot(root=root) == _lib.ROMA_E_ARG and b"root=" in lib.roma_last_error()
    for sigma in (0.0, -1.0, float("nan")):
        assert rot(sigma=sigma) == _lib.ROMA_E_ARG and b"sigma_deg" in lib.roma_last_error()
    for iters in (-1, 51):
        assert rot(iters=iters) == _lib.ROMA_E_ARG and b"iters must be in [0, 50]" in lib.roma_last_error()
    for kw in ("R_rel", "R"):
        assert rot(**{kw: odd}) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()

    tab = (ctypes.c_void_p * 32)(*[ctypes.addressof(buf)] * 32)
    obs = ctypes.cast(tab, ctypes.c_void_p)
    need = lib.roma_positions_workspace(3, 64, 3, None)

    def pos(obs=obs, stride=2, K=a, R=a, pairs=a, t_rel=a, V=3, N=64, M=3, root=0, thr=4.0, rounds=4, t=a, points=a, mask=a, count=a, lam=a,
            status=a, ws=a, size=need):
        return lib.roma_global_positions(obs, None, None, stride, K, R, pairs, t_rel, V, N, M, root, thr, rounds, t, a, points, mask, count, lam,
                                         status, ws, size, None)

    for kw in ("obs", "K", "R", "pairs", "t_rel", "t", "points", "mask", "count", "lam", "status", "ws"):
        assert pos(**{kw: None}) == _lib.ROMA_E_ARG and b"roma_global_positions: null pointer" in lib.roma_last_error()
    for V in (1, 2, 33):
        assert pos(V=V) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
    assert pos(N=0) == _lib.ROMA_E_SHAPE and b"bad shape N=0" in lib.roma_last_error()
    assert pos(M=0) == _lib.ROMA_E_SHAPE and b"bad shape M=0" in lib.roma_last_error()
    for stride in (0, 1, 3, -2):
        assert pos(stride=stride) == _lib.ROMA_E_SHAPE and b"point_stride" in lib.roma_last_error()
    for root in (-1, 3):
        assert pos(root=root) == _lib.ROMA_E_ARG and b"root=" in lib.roma_last_error()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert pos(thr=thr) == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    for rounds in (1, 9):
        assert pos(rounds=rounds) == _lib.ROMA_E_ARG and b"rounds must be in [2, 8]" in lib.roma_last_error()
    assert pos(size=need - 1) == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    for kw in ("K", "R", "t_rel", "t", "points", "lam", "ws"):
        assert pos(**{kw: odd}) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()
    assert pos(count=ctypes.c_void_p(ctypes.addressof(buf) + 2)) == _lib.ROMA_E_ALIGN and b"4-byte" in lib.roma_last_error()
    tab[2] = ctypes.addressof(buf) + 4
    assert pos() == _lib.ROMA_E_ALIGN and b"observations of view 2" in lib.roma_last_error()
    tab[2] = None
    assert pos() == _lib.ROMA_E_ARG and b"null pointer (observations of view 2)" in lib.roma_last_error()
    assert lib.roma_abi_version() == 5                                         # additive: the ABI stays


def test_motion_surface_validates_without_a_gpu():
    from roma_amd import geometry
    f64 = torch.float64
    x, K = torch.rand(3, 50, 2) * 500, torch.eye(3, dtype=f64)
    R, pairs = torch.eye(3, dtype=f64).expand(3, 3, 3), torch.tensor([[0, 1], [0, 2], [1, 2]], dtype=torch.int32)
    t_rel = torch.ones(3, 3, dtype=f64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.average_rotations(R, pairs, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.global_positions(x, R, K, pairs, t_rel)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.initialize_cameras(x, K, pairs, R, t_rel)
    for V in (1, 33):                                                          # checked before any tensor is examined
        with pytest.raises(ValueError, match="views"):
            geometry.average_rotations(R, pairs, V)
    for root in (-1, 3):
        with pytest.raises(ValueError, match="root"):
            geometry.average_rotations(R, pairs, 3, root=root)
    with pytest.raises(ValueError, match="iters"):
        geometry.average_rotations(R, pairs, 3, iters=51)
    with pytest.raises(ValueError, match="sigma_deg"):
        geometry.average_rotations(R, pairs, 3, sigma_deg=0.0)
    for thr in (0.0, -1.0):
        with pytest.raises(ValueError, match="threshold"):
            geometry.global_positions(x, R, K, pairs, t_rel, threshold=thr)
    for rounds in (1, 9):
        with pytest.raises(ValueError, match="rounds"):
            geometry.global_positions(x, R, K, pairs, t_rel, rounds=rounds)
    need, off = geometry.positions_workspace_layout(5, 300, 10)
    assert need > off[-1] > 0 and len(off) == 11
    with pytest.raises(ValueError, match="bad shape"):
        geometry.positions_workspace_layout(2, 300, 1)
    assert "RotationAverage(R=(3, 3, 3)" in repr(geometry.RotationAverage(R, None, t_rel[:, 0], None))
    assert "GlobalPositions(t=(3, 3)" in repr(geometry.GlobalPositions(t_rel, None, x, None, None, None, None))
    assert "CameraStart(R=(3, 3, 3)" in repr(geometry.CameraStart(R, None, x, None, None, None, None))


def test_motion_kernels_resource_report():
    """The compiler's resource report of csrc/motion_average.hip (the table of DESIGN.md §3.4): nine kernels, none with scratch, and the
    eigen-solve's matrix and eigenvectors of 94 rows beside its static LDS below 160 KB."""
    kernels = kernel_resources("motion_average.hip")
    names = ("rotation_average", "positions_init", "positions_vote", "positions_accumulate", "positions_reduce", "positions_solve",
             "positions_points", "positions_sign", "positions_final")
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch | occupancy |")
    for n in names:
        (k,) = [v for name, v in kernels.items() if f"{n}_kernel" in name]
        print(f"| `{n}_kernel` | {k['VGPRs']} | {k['TotalSGPRs']} | {k['LDS Size']} | {k['ScratchSize']} | {k['Occupancy']} |")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
    assert len(kernels) == len(names), sorted(kernels)
    (solve,) = [v for name, v in kernels.items() if "positions_solve_kernel" in name]
    (acc,) = [v for name, v in kernels.items() if "positions_accumulate_kernel" in name]
    both = 2 * 94 * 94 * 8
    print(f"eigen-solve: {solve['LDS Size']} bytes of static LDS + {both} of the matrix and its eigenvectors at V = 32")
    assert solve["LDS Size"] + both < 160 * 1000
    assert acc["LDS Size"] + 8 * (96 * 97 // 2 + 32) <= 64 * 1024              # the block's partial matrix beside its static LDS


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV)


def _run(p, raw=False, perm=None, R=None):
    """the two stages on the device -> the restatement's dict; with R the second stage runs under these rotations, not the first stage's"""
    from roma_amd import geometry
    x, vis = p["x"], p["visible"]
    if perm is not None:
        x, vis = x[:, perm], None if vis is None else vis[:, perm]
    pairs, t_rel = _dev(p["pairs"]), _dev(p["t_rel"])
    rot = geometry.average_rotations(_dev(p["R_rel"]), pairs, len(x), weights=_dev(p["weights"]), root=p["root"])
    pos = geometry.global_positions(_dev(x), rot.R if R is None else _dev(R), _dev(p["K"]), pairs, t_rel, visible=_dev(vis), threshold=THR, root=p["root"])
    if raw:
        return rot, pos
    out = {k: getattr(pos, k).cpu().numpy() for k in ("t", "centres", "points", "mask", "eigenvalues")}
    out.update(R=rot.R.cpu().numpy(), valid=rot.valid.cpu().numpy(), residual=np.radians(rot.residual_deg.cpu().numpy()),
               rotation_status=int(rot.status), position_status=int(pos.status), status=int(pos.status), count=int(pos.count))
    return out


def _assert_parity(got, want, what, tol=MOTION_TOL, points=True):
    assert got["rotation_status"] == want["rotation_status"] and got["position_status"] == want["position_status"], (got["position_status"], want["position_status"])
    assert np.array_equal(got["valid"], want["valid"]) and got["count"] == want["count"] and np.array_equal(got["mask"], want["mask"])
    assert np.array_equal(np.isnan(got["residual"]), np.isnan(want["residual"]))
    d = _diff(got, want) if points else _diff(dict(got, points=want["points"]), want)
    dr = float(np.nanmax(np.abs(got["residual"] - want["residual"]))) if np.isfinite(want["residual"]).any() else 0.0
    ok = np.isfinite(want["t"])
    dt = float(np.abs(got["t"][ok] - want["t"][ok]).max()) if ok.any() else 0.0
    dl = float(np.abs(got["eigenvalues"] - want["eigenvalues"]).max()) if np.isfinite(want["eigenvalues"]).all() else 0.0
    print(f"{what}: device against the restatement: R, centres, points differ by at most {d:.2e}, t by {dt:.2e}, the edge residuals by {dr:.2e} rad "
          f"(tolerance {tol:.2e}), the eigenvalues by {dl:.2e} (bound {_lambda_bound(want):.2e}); count {got['count']}")
    assert np.array_equal(np.isnan(got["t"]), np.isnan(want["t"])) and np.array_equal(np.isnan(got["eigenvalues"]), np.isnan(want["eigenvalues"]))
    assert d <= tol and dt <= tol and dr <= tol and dl <= _lambda_bound(want), (d, dt, dr, dl)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCENES + EDGE_CASES, ids=lambda c: c if isinstance(c, str) else f"V{c[0]}-N{c[1]}")
def test_device_equals_the_restatement(case):
    """the scenes, and: two points; one point more than a workgroup's chunk; V = 32 (bit 31 of the view masks, 93 unknowns); the partial
    sums at their cap with one workgroup walking a second chunk; a pose graph in two components; `visible` against NaN pixels; NaN rows;
    a duplicated edge with weights; a strong skew; another root.
    Each entry point is held to its restatement on the SAME input: the second stage runs under the restatement's rotations.  Chained on the
    device's own rotations, which differ from them in the last bit (2e-16), masks, count, status, R, t and centres still agree within the
    tolerance, but a point does not have to: P = I - d d^T carries the rounding of d, one ulp, into the smallest eigenvalue of A_n, which
    is theta^2 / 2 for a track of parallax theta, so its depth moves by eps / theta^2 — 5e-8 for the track of case "cap" that views 0 and
    2 see under 0.03 degrees, in the restatement as on the device."""
    p, want = _case(case), restated(case)
    tol = CAP_TOL if case == "cap" else MOTION_TOL
    got = _run(p, R=want["R"])
    _assert_parity(got, want, str(case), tol)
    got = _run(p)
    _assert_parity(got, want, f"{case}, chained", tol, points=False)
    assert np.array_equal(np.isnan(got["points"]), np.isnan(want["points"]))
    print(f"  chained: the points differ by at most {np.nanmax(np.abs(got['points'] - want['points'])) if np.isfinite(want['points']).any() else 0.0:.2e}")
    if case == "components":
        assert got["position_status"] == 2 and not got["valid"][4:].any() and np.isnan(got["R"][4:]).all() and np.isnan(got["t"][4:]).all()
    elif case == "visible":
        plain = _run(problem(5, 300))
        assert all(np.array_equal(got[k], plain[k], equal_nan=True) for k in ("R", "t", "centres", "points", "mask", "eigenvalues"))
    elif not isinstance(case, str):
        _check_scene(got, p, f"device, {case}")


@pytest.mark.gpu
def test_permuting_the_points_changes_nothing():
    p = problem(5, 600)
    perm = np.random.default_rng(3).permutation(600)
    plain, mixed = _run(p), _run(p, perm=perm)
    assert np.array_equal(mixed["mask"], plain["mask"][:, perm]) and mixed["count"] == plain["count"] and mixed["status"] == plain["status"] == 0
    assert np.array_equal(np.isnan(mixed["points"]), np.isnan(plain["points"][perm]))
    d = max(np.abs(mixed["centres"] - plain["centres"]).max(), np.nanmax(np.abs(mixed["points"] - plain["points"][perm])))
    print(f"points permuted: centres and points differ by at most {d:.2e} (tolerance {MOTION_TOL:.2e})")
    assert np.array_equal(mixed["R"], plain["R"]) and d <= MOTION_TOL


@pytest.mark.gpu
def test_relabelling_the_root_gives_the_same_reconstruction():
    """root = 2 against root = 0 on one scene.  The input has no world frame, so there is no origin to move; the two results live in the
    frames of their roots and — the unit norm of the centres is taken with another camera at the origin — are two estimates, not one:
    after alignment they agree within the truth-aware bounds that each of them meets."""
    p, q = problem(5, 600), variant("root2")
    a, b = _run(p), _run(q)
    turn = np.degrees([np.arccos(np.clip((np.trace((b["R"][v] @ a["R"][2]).T @ a["R"][v]) - 1) / 2, -1, 1)) for v in range(5)]).max()
    Ca, Cb = a["centres"] - a["centres"].mean(0), (b["centres"] @ a["R"][2]) - (b["centres"] @ a["R"][2]).mean(0)   # both in root 0's axes
    s = (Ca * Cb).sum() / (Cb * Cb).sum()
    gap = np.sqrt(((s * Cb - Ca) ** 2).sum(-1)).max() / np.sqrt((Ca * Ca).sum(-1)).max()
    print(f"root 2 against root 0: rotations differ by {turn:.4f} deg, centres by {gap:.5f} of their extent")
    assert np.allclose(b["R"][2], np.eye(3), atol=0) and np.array_equal(b["centres"][2], np.zeros(3))
    assert turn <= ROT_BOUND_DEG and gap <= CENTRE_BOUND and (a["mask"] == b["mask"]).mean() > 0.98


@pytest.mark.gpu
def test_bitwise_reproducible_and_capturable():
    """two eager runs and a replayed graph, process defaults left alone; initialize_cameras is the two calls in order"""
    from roma_amd import geometry
    p = problem(8, 600)
    x, K, pairs, R_rel, t_rel = (_dev(p[k]) for k in ("x", "K", "pairs", "R_rel", "t_rel"))
    call = lambda: geometry.initialize_cameras(x, K, pairs, R_rel, t_rel, threshold=THR)  # noqa: E731
    fields = ("R", "t", "points", "mask", "valid", "rotation_status", "position_status")
    same = lambda a, b: all(torch.equal(getattr(a, f).view(torch.uint8) if getattr(a, f).is_floating_point() else getattr(a, f),  # noqa: E731
                                        getattr(b, f).view(torch.uint8) if getattr(b, f).is_floating_point() else getattr(b, f)) for f in fields)
    first, second = call(), call()
    assert same(first, second) and int(first.position_status) == 0 and int(first.mask.sum()) > 0
    rot, pos = _run(p, raw=True)
    assert torch.equal(rot.R, first.R) and torch.equal(pos.t, first.t) and torch.equal(pos.mask, first.mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert same(out, first)


CHAIN = (5, 300)
CHAIN_ITERS = 10


@functools.lru_cache(maxsize=None)
def chain_restated():
    """initialize -> bundle (8 px, the mask) -> bundle (2 px), once through motion_ref and bundle_ref -> the errors of the three states"""
    p, r = problem(*CHAIN), restated(CHAIN)
    a = B.refine(p["x"], p["K"], r["R"], r["t"], r["points"], 8.0, CHAIN_ITERS, (0,), visible=r["mask"])
    b = B.refine(p["x"], p["K"], a["R"], a["t"], a["X"], 2.0, CHAIN_ITERS, (0,))
    return tuple(_pose_errors(s["R"], s["t"], p) for s in (r, a, b)), b, a["steps"]


def _pose_errors(R, t, p):
    return MR.rotation_error_deg(R, p["R"]), MR.centre_error(-np.einsum("vji,vj->vi", R, t), p["R"], p["t"])


def test_restated_chain_reaches_a_refined_reconstruction():
    (start, mid, end), b, a_steps = chain_restated()
    print(f"restated chain, V={CHAIN[0]} N={CHAIN[1]}: rotation {start[0]:.4f} -> {mid[0]:.4f} -> {end[0]:.4f} deg, centre {start[1]:.5f} -> {mid[1]:.5f} "
          f"-> {end[1]:.5f}; {a_steps} steps at 8 px, {b['steps']} at 2 px, cost {b['cost0']:.1f} -> {b['cost']:.1f}")
    assert a_steps >= 1 and b["cost"] <= b["cost0"] and end[0] < start[0] and end[1] < start[1]


@pytest.mark.gpu
def test_chain_from_pairwise_poses_to_a_refined_reconstruction():
    """README's chain from its new first step: initialize_cameras -> bundle_adjust(8 px, visible=mask) -> bundle_adjust(2 px); the result is
    inside five times the error of the same chain through motion_ref and bundle_ref"""
    from roma_amd import geometry
    p = problem(*CHAIN)
    (_, _, want), _, _ = chain_restated()
    x, K = _dev(p["x"]), _dev(p["K"])
    start = geometry.initialize_cameras(x, K, _dev(p["pairs"]), _dev(p["R_rel"]), _dev(p["t_rel"]), threshold=THR)
    assert int(start.rotation_status) == 0 and int(start.position_status) == 0 and bool(start.valid.all())
    a = geometry.bundle_adjust(x, start.R, start.t, K, start.points, visible=start.mask, threshold=8.0, iters=CHAIN_ITERS)
    b = geometry.bundle_adjust(x, a.R, a.t, K, a.points, threshold=2.0, iters=CHAIN_ITERS)
    e0 = _pose_errors(start.R.cpu().numpy(), start.t.cpu().numpy(), p)
    e2 = _pose_errors(b.R.cpu().numpy(), b.t.cpu().numpy(), p)
    print(f"device chain: rotation {e0[0]:.4f} -> {e2[0]:.4f} deg (restated {want[0]:.4f}), centre {e0[1]:.5f} -> {e2[1]:.5f} (restated {want[1]:.5f}); "
          f"{int(a.steps)} + {int(b.steps)} steps")
    assert int(a.steps) >= 1 and int(a.status) == 0 and int(b.status) == 0
    assert e2[0] <= 5 * want[0] and e2[1] <= 5 * want[1], (e2, want)
