"""roma_amd.geometry.bundle_adjust / reconstruction_error (csrc/bundle.hip) against the numpy restatement in tests/bundle_ref.py, which
solves the FULL damped normal equations (no Schur complement) under the Levenberg-Marquardt schedule of tests/lm_ref.py.

Scenes: tests/multiview_scenes.multiview_scene(V, seed, N) — sigma = 0.5 px, 10 % outlier observations in views >= 1 —, threshold
2 px, views 0 and 1 held unless said otherwise, and the start of bundle_ref.perturbed_start: every free view turned by 0.1 deg about
each axis (0.173 deg in all) and moved by 0.01, every point moved along its ray from view 0 by 0.5 % (normal) of its depth.

Measured with the restatement (the CPU tests print the figures again and assert the relations):
  ROT_BOUND_DEG,   5 x the worst error over (V, N) in {(3, 64), (5, 300)} x seeds 0-2, 10 steps: 0.0451 deg and 0.00796 (from 0.173 deg
  CENTRE_BOUND     and 0.0068-0.016 at the start), rounded up.  Views 0 and 1 are held at the truth, so the errors need no alignment
  BUNDLE_TOL       the restatement with the points summed in ascending, descending and shuffled order, over the parity cases (V = 2 with
                   one view held, V = 3 / N = 64 seeds 0-2, V = 5 / N = 300): R, t, X differ by at most 1.29e-12 (the V = 2 case, whose
                   scale only the damping holds; 7.5e-14 for the others); 10 x that
  INVARIANCE_TOL   the restatement on the world moved by multiview_scenes.WORLD_OFFSET (|offset| = 2.3e4), mapped back: R, t, X differ by
                   at most 2.43e-11 (V = 3 / N = 64, seeds 0-2); 10 x that

Two of the issue's cases are read here as its definition states them: a free view without a usable observation, or with a NaN pose, is
HELD — it comes back bit for bit — while the other views and the points are refined (steps >= 1), exactly as the restatement does."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import bundle_ref as B
from tests import multiview_scenes as MS
from tests.helpers import kernel_resources

DEV = "cuda:0"
THR = 2.0
ROT_BOUND_DEG, CENTRE_BOUND = 0.23, 0.04
BUNDLE_TOL = 1.3e-11
INVARIANCE_TOL = 2.43e-10
CHUNK, MAX_PARTIALS = 64, 256                       # points per workgroup and the cap of the partial sums (csrc/bundle.hip)
SCENES = [(3, 64, 0), (3, 64, 1), (3, 64, 2), (5, 300, 0), (5, 300, 1), (5, 300, 2)]
# (V, N, seed, fixed, iters): what the device is compared with the restatement on
PARITY = [(2, 64, 0, (0,), 6), (3, 64, 0, (0, 1), 10), (3, 64, 1, (0, 1), 10), (3, 64, 2, (0, 1), 10), (5, 300, 0, (0, 1), 6)]
SEAMS = [(3, CHUNK - 1, 1, (0, 1), 6), (3, CHUNK, 1, (0, 1), 6), (3, CHUNK + 1, 1, (0, 1), 6), (3, 3 * CHUNK + 1, 1, (0, 1), 6)]
WIDE = (32, 96, 0, (0, 1), 6)


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def problem(V, N, seed, fixed=(0, 1)):
    """the scene and its perturbed start"""
    s = MS.multiview_scene(V, seed, N)
    R0, t0, X0 = B.perturbed_start(s, seed, fixed)
    return _frozen(dict(s, R0=R0, t0=t0, X0=X0))


@functools.lru_cache(maxsize=None)
def restated(V, N, seed, fixed=(0, 1), iters=10, order=0):
    p = problem(V, N, seed, fixed)
    return _frozen(B.refine(p["x"], p["K"], p["R0"], p["t0"], p["X0"], THR, iters, fixed, order=order))


def _check_scene(r, p, what):
    """the scene criteria: the cost drops, a step is kept, no outlier is weighted, at most 5 % of the clean observations are not, and
    the cameras end within the truth-aware bounds"""
    er, ec = B.worst_errors(r["R"], r["t"], p["R"], p["t"])
    clean = p["seen"] & ~p["outlier"]
    lost = int((clean & ~r["mask"]).sum())
    print(f"{what}: cost {r['cost0']:.1f} -> {r['cost']:.1f} in {r['steps']} steps, worst rotation error {er:.4f} deg, worst centre error "
          f"{ec:.5f}, {lost} of {int(clean.sum())} clean observations outside the threshold, {int((r['mask'] & p['outlier']).sum())} outliers inside")
    assert r["cost"] < r["cost0"] and r["steps"] >= 1
    assert not (r["mask"] & p["outlier"]).any()
    assert lost <= 0.05 * clean.sum()
    assert r["count"] == r["mask"].sum()
    assert er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND, (er, ec)
    return er, ec


def _max_diff(a, b):
    return max(float(np.abs(a[k] - b[k]).max()) for k in ("R", "t", "X"))


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("V,N,seed", SCENES)
def test_numpy_restatement_meets_the_scene_criteria(V, N, seed):
    _check_scene(restated(V, N, seed), problem(V, N, seed), f"restatement, V={V} N={N} seed {seed}")


def test_truth_aware_bounds_are_five_times_the_worst_error_of_the_restatement():
    wr = wc = 0.0
    for V, N, seed in SCENES:
        r, p = restated(V, N, seed), problem(V, N, seed)
        er, ec = B.worst_errors(r["R"], r["t"], p["R"], p["t"])
        wr, wc = max(wr, er), max(wc, ec)
    print(f"restatement over {len(SCENES)} scenes: worst rotation error {wr:.4f} deg, worst centre error {wc:.5f}")
    assert 5 * wr <= ROT_BOUND_DEG <= 6 * wr and 5 * wc <= CENTRE_BOUND <= 6 * wc, (wr, wc)


def test_bundle_tolerance_is_ten_times_the_order_of_the_sums():
    worst = 0.0
    for case in PARITY:
        r = [restated(*case, order=o) for o in (0, 1, 2)]
        assert all(q["steps"] == r[0]["steps"] >= 1 and np.array_equal(q["mask"], r[0]["mask"]) for q in r)
        worst = max([worst] + [_max_diff(q, r[0]) for q in r[1:]])
    print(f"restatement, three orders of the sums over {len(PARITY)} cases: R, t, X differ by at most {worst:.3e}; tolerance {BUNDLE_TOL:.2e}")
    assert 0 < 10 * worst <= BUNDLE_TOL * 1.0001 and BUNDLE_TOL <= 11 * worst, worst


def _offset_start(p):
    return p["R0"], p["t0"] - p["R0"] @ MS.WORLD_OFFSET, p["X0"] + MS.WORLD_OFFSET


def _mapped_back(r):
    return {"R": r["R"], "t": r["t"] + r["R"] @ MS.WORLD_OFFSET, "X": r["X"] - MS.WORLD_OFFSET}


def test_invariance_tolerance_is_ten_times_what_the_world_offset_moves_the_restatement():
    worst = 0.0
    for seed in range(3):
        p, r = problem(3, 64, seed), restated(3, 64, seed)
        o = B.refine(p["x"], p["K"], *_offset_start(p), THR, 10, (0, 1))
        assert o["steps"] == r["steps"] and np.array_equal(o["mask"], r["mask"])
        worst = max(worst, _max_diff(_mapped_back(o), r))
    print(f"restatement, world moved by {np.linalg.norm(MS.WORLD_OFFSET):.3g}: R, t, X differ by at most {worst:.3e}; tolerance {INVARIANCE_TOL:.2e}")
    assert 0 < 10 * worst <= INVARIANCE_TOL * 1.0001 and INVARIANCE_TOL <= 11 * worst, worst


def test_schur_complement_step_equals_the_full_solve():
    """steps 1 to 4 of the kernels in numpy — eliminate each point, solve the reduced camera system, substitute back — against
    lm_ref.cholesky_solve on the full damped equations: V = 3, N = 8, view 0 held, no outliers, every observation weighted (50 px)"""
    s = MS.multiview_scene(3, 0, 8, outlier_frac=0.0)
    R0, t0, X0 = B.perturbed_start(s, 0, (0,))
    dc, dp, fc, fp = B.schur_step(s["x"], s["K"], R0, t0, X0, 50.0, (0,), 1e-3)
    assert dc.shape == (2, 6) and dp.shape == (8, 3)
    ec, ep = np.abs(dc - fc).max() / np.abs(fc).max(), np.abs(dp - fp).max() / np.abs(fp).max()
    print(f"Schur step against the full solve: relative difference {ec:.2e} (cameras), {ep:.2e} (points)")
    assert ec <= 1e-10 and ep <= 1e-10


def test_restatement_returns_the_input_where_nothing_can_be_refined():
    p = problem(3, 64, 0)
    x, K, R0, t0, X0 = p["x"], p["K"], p["R0"], p["t0"], p["X0"]
    r = B.refine(x, K, R0, t0, X0, THR, 0, (0, 1))
    assert r["steps"] == 0 and _same_bits(r, R0, t0, X0) and r["cost"] == r["cost0"]
    best = restated(3, 64, 0, iters=50)
    again = B.refine(x, K, best["R"], best["t"], best["X"], THR, 3, (0, 1))
    print(f"from the end of 50 steps: {again['steps']} more kept, cost {best['cost']:.6f} -> {again['cost']:.6f}")
    assert again["steps"] == 0 and again["cost"] == again["cost0"] and _same_bits(again, best["R"], best["t"], best["X"])
    far = B.perturbed_start(p, 0, scale=5.0)                                   # a start five times worse: a polish does not recover it
    r = B.refine(x, K, *far, THR, 10, (0, 1))
    assert r["cost"] <= r["cost0"]


def _same_bits(r, R0, t0, X0):
    from tests.lm_ref import same_bits
    return same_bits(r["R"], R0) and same_bits(r["t"], t0) and same_bits(r["X"], X0)


def test_bundle_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    off = (ctypes.c_long * 11)()
    op = ctypes.cast(off, ctypes.c_void_p)
    for V, N in ((2, 1), (3, 64), (8, 1 << 14), (32, 96), (32, 1 << 17)):
        need = lib.roma_bundle_workspace(V, N, op)
        assert need > 0 and lib.roma_bundle_workspace(V, N, None) == need
        o = list(off)
        assert o[0] == 0 and all(b > a for a, b in zip(o, o[1:])) and all(v % 256 == 0 for v in o) and o[-1] < need and need % 256 == 0
        n = 6 * V
        M, P = n * (n + 1) // 2 + 2 * n + V, min(-(-N // CHUNK), MAX_PARTIALS)
        assert o[10] - o[9] >= 8 * M * P and o[9] - o[8] >= 8 * M and o[6] - o[5] >= 24 * N           # partials, system, points
    assert lib.roma_bundle_workspace(32, 1 << 17, None) < 64 << 20
    for V, N in ((1, 64), (33, 64), (3, 0), (3, (1 << 24) + 1)):
        assert lib.roma_bundle_workspace(V, N, None) == _lib.ROMA_E_SHAPE and b"roma_bundle_workspace: bad shape" in lib.roma_last_error()

    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    tab = (ctypes.c_void_p * 32)(*[ctypes.addressof(buf)] * 32)
    obs = ctypes.cast(tab, ctypes.c_void_p)
    need = lib.roma_bundle_workspace(3, 64, None)

    def call(obs=obs, vis=None, stride=2, K=a, R_in=a, X_in=a, V=3, N=64, fixed=1, thr=2.0, iters=10, R=a, mask=a, count=a, ws=a, size=need):
        return lib.roma_bundle_adjust(obs, None, vis, stride, K, R_in, a, X_in, V, N, fixed, thr, iters, R, a, a, mask, a, count, a, a, ws, size,
                                      None)

    for kw in ("obs", "K", "R_in", "X_in", "R", "mask", "count", "ws"):
        assert call(**{kw: None}) == _lib.ROMA_E_ARG and b"roma_bundle_adjust: null pointer" in lib.roma_last_error()
    for V in (1, 33):
        assert call(V=V) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
    assert call(N=0) == _lib.ROMA_E_SHAPE and b"bad shape N=0" in lib.roma_last_error()
    for stride in (0, 1, 3, -2):
        assert call(stride=stride) == _lib.ROMA_E_SHAPE and b"point_stride" in lib.roma_last_error()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert call(thr=thr) == _lib.ROMA_E_ARG and b"threshold" in lib.roma_last_error()
    for iters in (-1, 51):
        assert call(iters=iters) == _lib.ROMA_E_ARG and b"iters must be in [0, 50]" in lib.roma_last_error()
    for fixed in (0, 8, 9):                                                    # none held; a view that does not exist
        assert call(fixed=fixed) == _lib.ROMA_E_ARG and b"fixed=" in lib.roma_last_error()
    assert call(fixed=7) == _lib.ROMA_E_ARG and b"holds every view" in lib.roma_last_error()
    assert call(V=32, fixed=0xFFFFFFFF, size=1 << 40) == _lib.ROMA_E_ARG and b"holds every view" in lib.roma_last_error()
    assert call(size=need - 1) == _lib.ROMA_E_ARG and b"workspace" in lib.roma_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 8)
    for kw in ("K", "R_in", "X_in", "R", "ws"):
        assert call(**{kw: odd}) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()
    assert call(count=ctypes.c_void_p(ctypes.addressof(buf) + 2)) == _lib.ROMA_E_ALIGN and b"4-byte" in lib.roma_last_error()
    tab[2] = ctypes.addressof(buf) + 4
    assert call() == _lib.ROMA_E_ALIGN and b"observations of view 2" in lib.roma_last_error()
    tab[2] = None
    assert call() == _lib.ROMA_E_ARG and b"null pointer (observations of view 2)" in lib.roma_last_error()
    assert lib.roma_abi_version() == 5                                         # additive: the ABI stays


def test_bundle_surface_validates_without_a_gpu():
    from roma_amd import geometry
    x, X = torch.rand(3, 50, 2) * 500, torch.rand(50, 3)
    R, t, K = torch.eye(3, dtype=torch.float64).expand(3, 3, 3), torch.zeros(3, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.bundle_adjust(x, R, t, K, X)
    with pytest.raises(ValueError, match="threshold"):                        # checked before any tensor is examined
        geometry.bundle_adjust(x, R, t, K, X, threshold=0.0)
    with pytest.raises(ValueError, match="iters"):
        geometry.bundle_adjust(x, R, t, K, X, iters=51)
    assert geometry._fixed_mask((0, 2), 3) == 5 and geometry._fixed_mask(torch.tensor([False, True, False]), 3) == 2
    assert geometry._fixed_mask(torch.tensor([31]), 32) == 1 << 31
    with pytest.raises(ValueError, match="every view is held"):
        geometry._fixed_mask((0, 1, 2), 3)
    with pytest.raises(ValueError, match="at least one view"):
        geometry._fixed_mask((), 3)
    with pytest.raises(ValueError, match="view indices"):
        geometry._fixed_mask((3,), 3)
    with pytest.raises(ValueError, match="bool tensor"):
        geometry._fixed_mask(torch.tensor([True, False]), 3)
    need, off = geometry.bundle_workspace_layout(5, 300)
    assert need > off[-1] > 0 and len(off) == 11
    with pytest.raises(ValueError, match="bad shape"):
        geometry.bundle_workspace_layout(1, 300)
    assert "BundleResult(R=(3, 3, 3)" in repr(geometry.BundleResult(R, t, X, None, None, None, None, None))
    # reconstruction_error is torch ops only: a reconstruction in another frame and unit has no error
    s = MS.multiview_scene(5, 0, 50)
    Q, sc, tau = B.exp_so3(np.array([0.3, -0.2, 0.4])), 2.5, np.array([1.0, -2.0, 0.5])
    R2 = s["R"] @ Q.T
    e = geometry.reconstruction_error(R2, sc * s["t"] - R2 @ tau, sc * (s["X"] @ Q.T) + tau, s["R"], s["t"], s["X"])
    assert all(float(v) < 1e-9 for v in e)
    e = geometry.reconstruction_error(B.exp_so3(np.radians([0.0, 0.0, 1.0])) @ s["R"], s["t"], s["X"], s["R"], s["t"], s["X"])
    assert 0.2 < float(e[0]) < 1.0


def test_bundle_kernels_resource_report():
    """The compiler's resource report of csrc/bundle.hip (the table of DESIGN.md §3.4): nine kernels, none with scratch, and the
    solver's packed triangle of 192 rows beside its static LDS within the 160 KiB of a compute unit."""
    kernels = kernel_resources("bundle.hip")
    names = ("init", "centre", "evaluate", "decide", "accumulate", "reduce", "solve", "propose", "final")
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch | occupancy |")
    for n in names:
        (k,) = [v for name, v in kernels.items() if f"bundle_{n}_kernel" in name]
        print(f"| `bundle_{n}_kernel` | {k['VGPRs']} | {k['TotalSGPRs']} | {k['LDS Size']} | {k['ScratchSize']} | {k['Occupancy']} |")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
    assert len(kernels) == len(names), sorted(kernels)
    (solve,) = [v for name, v in kernels.items() if "bundle_solve_kernel" in name]
    packed = (6 * 32) * (6 * 32 + 1) // 2 * 8
    print(f"solver: {solve['LDS Size']} bytes of static LDS + {packed} of the packed lower triangle at V = 32")
    assert solve["LDS Size"] + packed <= 160 * 1024


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _np(r):
    out = {k: getattr(r, k).cpu().numpy() for k in ("R", "t", "mask")}
    out["X"] = r.points.cpu().numpy()
    out.update(cost=float(r.cost), cost0=float(r.cost0), steps=int(r.steps), count=int(r.count), status=int(r.status))
    return out


def _run(p, fixed=(0, 1), iters=10, start=None, x=None, visible=None, raw=False):
    from roma_amd import geometry
    R0, t0, X0 = (p["R0"], p["t0"], p["X0"]) if start is None else start
    r = geometry.bundle_adjust(_dev(p["x"] if x is None else x), _dev(R0), _dev(t0), _dev(p["K"]), _dev(X0), threshold=THR, iters=iters,
                               fixed=fixed, visible=None if visible is None else _dev(visible))
    return r if raw else _np(r)


def _assert_parity(got, want, tol=BUNDLE_TOL):
    d = _max_diff(got, want)
    print(f"device against the restatement: R, t, X differ by at most {d:.2e} (tolerance {tol:.2e}); steps {got['steps']}, count {got['count']}, "
          f"cost {got['cost0']:.3f} -> {got['cost']:.3f}")
    assert got["status"] == 0 and got["steps"] == want["steps"] and got["count"] == want["count"] and np.array_equal(got["mask"], want["mask"])
    assert abs(got["cost"] - want["cost"]) <= 1e-9 * want["cost"] and abs(got["cost0"] - want["cost0"]) <= 1e-9 * want["cost0"]
    assert d <= tol, d


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY + SEAMS + [WIDE], ids=lambda c: f"V{c[0]}-N{c[1]}-seed{c[2]}-iters{c[4]}")
def test_device_equals_the_restatement(case):
    """the parity cases; N around one and three workgroups' worth of points; V = 32: bit 31 of the view masks and the largest reduced
    system (186 unknowns)"""
    V, N, seed, fixed, iters = case
    want = restated(*case)
    got = _run(problem(V, N, seed, fixed), fixed, iters)
    _assert_parity(got, want)
    assert want["steps"] >= 1
    if V == 32:
        assert got["mask"][31].sum() >= 10 and not np.array_equal(got["R"][31], problem(V, N, seed, fixed)["R0"][31])


@pytest.mark.gpu
def test_partial_sums_at_their_cap():
    """N = 64 * 256 + 1: the partial count is at its cap and one workgroup walks a second chunk.  The full equations of the restatement
    are out of reach at this size, so the result is held to the scene criteria, to the restatement's cost and mask evaluated at the
    returned state, and to a second run bit for bit."""
    N = CHUNK * MAX_PARTIALS + 1
    p = problem(3, N, 0)
    got = _run(p, iters=6)
    _check_scene(got, p, f"device, N={N}")
    P = B.Problem(p["x"], p["K"], got["R"], got["t"], got["X"], None, (0, 1), THR, 0)
    cost, count, mask, _ = P.evaluate((got["R"], got["t"], got["X"]))
    assert abs(cost - got["cost"]) <= 1e-9 * cost and count == got["count"] and np.array_equal(mask, got["mask"])
    again = _run(p, iters=6)
    assert all(np.array_equal(got[k], again[k]) for k in ("R", "t", "X", "mask")) and got["cost"] == again["cost"]


@pytest.mark.gpu
@pytest.mark.parametrize("V,N,seed", SCENES)
def test_device_meets_the_scene_criteria(V, N, seed):
    p = problem(V, N, seed)
    got = _run(p)
    _check_scene(got, p, f"device, V={V} N={N} seed {seed}")
    far = _run(p, start=B.perturbed_start(p, seed, scale=5.0))                  # whatever the start, the cost never rises
    assert far["cost"] <= far["cost0"]


@pytest.mark.gpu
def test_one_held_view_and_a_bool_tensor_for_fixed():
    p = problem(5, 300, 0, (0,))
    got = _run(p, fixed=torch.tensor([True, False, False, False, False]))
    from roma_amd import geometry
    er, ec, ex = (float(v) for v in geometry.reconstruction_error(_dev(got["R"]), _dev(got["t"]), _dev(got["X"]), _dev(p["R"]), _dev(p["t"]), _dev(p["X"])))
    print(f"one view held: {got['steps']} steps, cost {got['cost0']:.1f} -> {got['cost']:.1f}; after alignment {er:.4f} deg, {ec:.5f}, median point {ex:.5f}")
    assert got["steps"] >= 1 and got["cost"] < got["cost0"] and er <= ROT_BOUND_DEG and ec <= CENTRE_BOUND
    assert np.array_equal(got["R"][0], p["R0"][0]) and np.array_equal(got["t"][0], p["t0"][0])


@pytest.mark.gpu
def test_world_offset_changes_nothing():
    for seed in range(3):
        p = problem(3, 64, seed)
        plain, moved = _run(p), _run(p, start=_offset_start(p))
        assert moved["steps"] == plain["steps"] >= 1 and np.array_equal(moved["mask"], plain["mask"])
        d = _max_diff(_mapped_back(moved), plain)
        print(f"seed {seed}: the world offset moves R, t, X by at most {d:.2e} (tolerance {INVARIANCE_TOL:.2e})")
        assert d <= INVARIANCE_TOL


@pytest.mark.gpu
def test_permuting_the_points_changes_nothing():
    p = problem(5, 300, 0)
    perm = np.random.default_rng(3).permutation(300)
    plain = _run(p, iters=6)
    mixed = _run(p, iters=6, start=(p["R0"], p["t0"], p["X0"][perm]), x=p["x"][:, perm])
    assert mixed["steps"] == plain["steps"] and np.array_equal(mixed["mask"], plain["mask"][:, perm])
    d = max(np.abs(mixed["R"] - plain["R"]).max(), np.abs(mixed["t"] - plain["t"]).max(), np.abs(mixed["X"] - plain["X"][perm]).max())
    print(f"points permuted: R, t, X differ by at most {d:.2e}")
    assert d <= BUNDLE_TOL


@pytest.mark.gpu
def test_bitwise_reproducible_and_capturable():
    """two eager runs and a replayed graph, process defaults left alone"""
    from roma_amd import geometry
    p = problem(5, 300, 0)
    args = (_dev(p["x"]), _dev(p["R0"]), _dev(p["t0"]), _dev(p["K"]), _dev(p["X0"]))
    call = lambda: geometry.bundle_adjust(*args, threshold=THR, iters=6, fixed=(0, 1))  # noqa: E731
    fields = ("R", "t", "points", "mask", "cost", "cost0", "steps", "count", "status")
    same = lambda a, b: all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields)  # noqa: E731
    first, second = call(), call()
    assert same(first, second) and int(first.steps) >= 1
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


@pytest.mark.gpu
def test_what_cannot_be_refined_comes_back_bit_for_bit():
    p = problem(3, 64, 0)
    R0, t0, X0 = p["R0"], p["t0"], p["X0"]
    same = lambda r: _same_bits(r, R0, t0, X0)  # noqa: E731
    start_cost = restated(3, 64, 0)["cost0"]
    r = _run(p, iters=0)                                                        # iters = 0
    assert r["steps"] == 0 and same(r) and r["cost"] == r["cost0"] and abs(r["cost0"] - start_cost) <= 1e-9 * start_cost
    assert np.array_equal(r["mask"], B.refine(p["x"], p["K"], R0, t0, X0, THR, 0, (0, 1))["mask"])
    with pytest.raises(ValueError, match="every view is held"):                # every view fixed
        _run(p, fixed=(0, 1, 2))
    best = restated(3, 64, 0, iters=50)                                        # a start at a minimum: no step lowers the cost
    r = _run(p, iters=3, start=(best["R"], best["t"], best["X"]))
    assert r["steps"] == 0 and r["cost"] == r["cost0"] and _same_bits(r, best["R"], best["t"], best["X"])
    # a free view whose observations are all NaN, and one whose pose is NaN: held, bit for bit; the others are still refined
    q = problem(4, 100, 0)
    x = q["x"].copy()
    x[3] = np.nan
    r, want = _run(q, iters=6, x=x), B.refine(x, q["K"], q["R0"], q["t0"], q["X0"], THR, 6, (0, 1))
    assert np.array_equal(r["R"][3], q["R0"][3]) and np.array_equal(r["t"][3], q["t0"][3]) and not r["mask"][3].any()
    _assert_parity(r, want)
    assert r["steps"] >= 1
    Rn = q["R0"].copy()
    Rn[3, 1, 1] = np.nan
    r, want = _run(q, iters=6, start=(Rn, q["t0"], q["X0"])), B.refine(q["x"], q["K"], Rn, q["t0"], q["X0"], THR, 6, (0, 1))
    assert r["R"][3].tobytes() == Rn[3].tobytes() and np.array_equal(r["t"][3], q["t0"][3]) and not r["mask"][3].any()
    r["R"][3], want["R"][3] = 0.0, 0.0
    _assert_parity(r, want)
    # points with no observation, with one, and one that is NaN itself come back unchanged while the rest moves
    x = q["x"].copy()
    x[:, 0] = np.nan
    x[1:, 1] = np.nan
    Xn = q["X0"].copy()
    Xn[2] = np.nan
    r = _run(q, iters=6, x=x, start=(q["R0"], q["t0"], Xn))
    want = B.refine(x, q["K"], q["R0"], q["t0"], Xn, THR, 6, (0, 1))
    assert np.array_equal(r["X"][:2], q["X0"][:2]) and np.isnan(r["X"][2]).all()
    assert not r["mask"][:, 0].any() and not r["mask"][1:, 1].any() and not r["mask"][:, 2].any()
    assert (r["X"][3:] != q["X0"][3:]).any(1).sum() > 80
    r["X"][2], want["X"][2] = 0.0, 0.0
    _assert_parity(r, want)
    # only the held views are usable: status bit 1, the input
    Rn = q["R0"].copy()
    Rn[2:, 0, 0] = np.inf
    r = _run(q, start=(Rn, q["t0"], q["X0"]))
    assert r["steps"] == 0 and r["status"] == 2 and r["R"].tobytes() == Rn.tobytes() and np.array_equal(r["X"], q["X0"])


@pytest.mark.gpu
def test_chain_from_tracks_to_a_refined_reconstruction():
    """README's example: build_tracks -> triangulate_nview -> bundle_adjust on a synthetic scene, Tracks.x / Tracks.visible and the fp32
    points passed on as they come; after alignment the reconstruction is within the truth-aware bounds"""
    from roma_amd import geometry
    from tests.test_tracks import pure_tracks, scene, scene_inputs
    s, inp = scene(5, 0), scene_inputs(5, 0)
    R0, t0, _ = B.perturbed_start(s, 0, (0, 1))                                 # cameras as estimate_pose / find_absolute_pose leave them
    K = _dev(s["K"])
    tracks = geometry.build_tracks(_dev(inp["matches"]), _dev(inp["certainty"]), _dev(inp["pairs"]), inp["sizes"], cell=4, max_tracks=512)
    tri = geometry.triangulate_nview(tracks.x, _dev(R0), _dev(t0), K, visible=tracks.visible)
    ba = geometry.bundle_adjust(tracks.x, _dev(R0), _dev(t0), K, tri.points, visible=tracks.visible, threshold=THR, iters=10, fixed=(0, 1))
    out = {k: getattr(tracks, k).cpu().numpy() for k in ("x", "visible", "track_of_match")}
    pure = pure_tracks(out, s)
    rows, pts = np.array([r for r, _ in pure]), np.array([j for _, j in pure])
    before = geometry.reconstruction_error(_dev(R0), _dev(t0), tri.points[rows], _dev(s["R"]), _dev(s["t"]), _dev(s["X"][pts]))
    after = geometry.reconstruction_error(ba.R, ba.t, ba.points[rows], _dev(s["R"]), _dev(s["t"]), _dev(s["X"][pts]))
    print(f"chain over {len(pure)} pure tracks: {int(ba.steps)} steps, cost {float(ba.cost0):.1f} -> {float(ba.cost):.1f}; rotation "
          f"{float(before[0]):.4f} -> {float(after[0]):.4f} deg, centre {float(before[1]):.5f} -> {float(after[1]):.5f}, median point "
          f"{float(before[2]):.5f} -> {float(after[2]):.5f}")
    assert int(ba.steps) >= 1 and float(ba.cost) < float(ba.cost0) and int(ba.status) == 0
    assert float(after[0]) <= ROT_BOUND_DEG and float(after[1]) <= CENTRE_BOUND and float(after[2]) < float(before[2])
