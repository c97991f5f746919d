"""roma_amd.geometry.triangulate / depth_from_warp (csrc/triangulate.hip) against the numpy restatement in tests/triangulate_ref.py.
Scenes are G.two_view_scene with the true pose of PR.scene_pose.  CPU tests pin the restatement (the correction lands on the epipolar
constraint, the optimal method never loses to the midpoint, clean matches give the true depths), the C-ABI argument checks and the
kernel's resource report; GPU tests pin the kernel and the wrappers.

Parity tolerance.  Device and restatement run the same algorithm from the same fp32 matches and the same fp64 pair constants; the
device computes per match in fp32 where the reference run of the restatement computes in fp64.  What fp32 costs is measured by running
the restatement itself in float32: per scene and method, the largest deviation of its float32 run from its float64 run over the
compared matches, times 4 for the kernel's other operation order and its fused multiply-adds.  Nothing in it comes from the kernel.
Compared are the matches for which the fp64 run finds both depths positive and a parallax of at least 2 degrees (below that the
depth of a match is ill-conditioned in any precision): at least 75 % of all matches and every inlier, both asserted.  Deviations are
measured as |dX| / |X| for points, |dz| / |z| for depths, |d cos| for cos_parallax and |dr| / max(r, 1 px) for reproj_error — absolute
in pixels for matches that fit, relative for outliers whose midpoint projects thousands of pixels away.  For orientation, on
the CPU: about 6e-5 for points and depths, 1e-4 px for reproj_error, 2e-7 for cos_parallax."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import geometry_ref as G
from tests import pose_ref as PR
from tests import triangulate_ref as T
from tests.helpers import dev, kernel_resources

DEV = "cuda:0"
FIELDS = ("points", "depth_a", "depth_b", "reproj", "cos_parallax")
MIN_PARALLAX_DEG = 2.0
COS_MIN_PARALLAX = math.cos(math.radians(MIN_PARALLAX_DEG))


@functools.lru_cache(maxsize=None)
def scene(seed, N=1000):
    """m (N,4) float32 noisy matches with 40 % outliers, truth (N,) inlier flags, clean (N,4) fp64, K, R, t"""
    xa, xb, truth, _, ca, cb = G.two_view_scene(seed, N=N)
    K, R, t = PR.scene_pose(seed)
    return np.concatenate([xa, xb], -1).astype(np.float32), truth, np.concatenate([ca, cb], -1), K, R, t


@functools.lru_cache(maxsize=None)
def ref(seed, N, method, dtype="float64"):
    m, _, _, K, R, t = scene(seed, N)
    return T.triangulate(m, K, K, R, t, method, dtype=getattr(np, dtype))


def deviations(o, r, sel):
    """the five deviation measures of the module docstring of outputs o against the fp64 run r, largest over the matches sel"""
    nrm = np.linalg.norm(r["points"], axis=-1)
    with np.errstate(all="ignore"):
        d = {"points": np.linalg.norm(o["points"].astype(np.float64) - r["points"], axis=-1) / nrm,
             "depth_a": np.abs(o["depth_a"] - r["depth_a"]) / np.abs(r["depth_a"]),
             "depth_b": np.abs(o["depth_b"] - r["depth_b"]) / np.abs(r["depth_b"]),
             "reproj": np.abs(o["reproj"] - r["reproj"]) / np.maximum(r["reproj"], 1.0),
             "cos_parallax": np.abs(o["cos_parallax"] - r["cos_parallax"])}
    return {k: float(v[sel].max()) for k, v in d.items()}


def compared(r):
    return r["valid"] & (r["cos_parallax"] <= COS_MIN_PARALLAX)


def tolerance(r64, r32, sel):
    return {k: 4.0 * v for k, v in deviations(r32, r64, sel).items()}


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_optimal_lands_on_the_epipolar_constraint_and_never_loses_to_midpoint():
    for seed in range(5):
        m, truth, _, K, R, t = scene(seed, 2000)
        o, mid = ref(seed, 2000, "optimal"), ref(seed, 2000, "midpoint")
        F = T.pair_constants(K, K, R, t)[0]
        c = o["corrected"][truth]
        one = np.ones((len(c), 1))
        res = np.abs(np.einsum("ni,ij,nj->n", np.concatenate([c[:, 2:], one], -1), F, np.concatenate([c[:, :2], one], -1)))
        ro, rm = T.reprojection_sq(o["points"], m, K, K, R, t)[truth], T.reprojection_sq(mid["points"], m, K, K, R, t)[truth]
        print(f"scene {seed}: |x_B'^T F x_A'| <= {res.max():.2e} on the inliers; squared reprojection error optimal - midpoint <= "
              f"{(ro - rm).max():.2e}, means {ro.mean():.4f} / {rm.mean():.4f} px^2")
        assert abs(np.sqrt((F * F).sum()) - 1) < 1e-14 and o["finite"][truth].all() and o["valid"][truth].all()
        assert res.max() < 1e-12
        assert (ro <= rm).all() and ro.mean() < rm.mean()
        # what each method reports as reproj_error is the true reprojection error of the point it returns
        assert np.abs(o["reproj"][truth] ** 2 - ro).max() < 1e-9 and np.abs(mid["reproj"][truth] ** 2 - rm).max() < 1e-9
    m, truth, _, K, R, t = scene(0, 2000)
    ro, rm = T.reprojection_sq(ref(0, 2000, "optimal")["points"], m, K, K, R, t)[truth], \
        T.reprojection_sq(ref(0, 2000, "midpoint")["points"], m, K, K, R, t)[truth]
    assert abs(ro.mean() - 0.2605) < 5e-4 and abs(rm.mean() - 0.2623) < 5e-4


def test_clean_matches_with_the_true_pose_reproduce_the_true_depths():
    for seed in range(5):
        _, truth, clean, K, R, t = scene(seed, 2000)
        mid = T.triangulate(clean[truth], K, K, R, t, "midpoint")
        za = mid["depth_a"]
        assert mid["valid"].all() and za.min() >= 4 - 1e-9 and za.max() <= 12 + 1e-9           # the scene draws depths in [4, 12]
        assert mid["reproj"].max() < 1e-9                                                       # the rays of clean matches meet
        Xb = mid["points"] @ R.T + t
        assert np.abs(Xb[:, 2] - mid["depth_b"]).max() < 1e-12
        o = T.triangulate(clean[truth], K, K, R, t, "optimal")
        assert o["valid"].all() and o["reproj"].max() < 1e-9
        assert np.abs(o["depth_a"] / za - 1).max() < 1e-10 and np.abs(o["depth_b"] / mid["depth_b"] - 1).max() < 1e-10
        assert np.abs(o["points"] - mid["points"]).max() < 1e-9
        # the noisy inliers (sigma = 0.5 px): median relative depth error about 0.0045
        noisy = ref(seed, 2000, "optimal")["depth_a"][truth]
        med = float(np.median(np.abs(noisy / za - 1)))
        print(f"scene {seed}: median relative depth error of the noisy inliers {med:.4f}")
        assert 0.003 < med < 0.006


def test_float32_run_of_the_restatement_and_the_shares_of_compared_matches():
    """What the GPU parity test relies on, checked here without a device: the compared matches are >= 75 % of all and every inlier,
    inlier parallax is >= 3.4 deg, and fp32 costs what the module docstring says."""
    for seed in range(3):
        truth = scene(seed)[1]
        for method in T.METHODS:
            r64, r32 = ref(seed, 1000, method), ref(seed, 1000, method, "float32")
            assert r32["points"].dtype == np.float32 and r32["reproj"].dtype == np.float32
            sel = compared(r64)
            par = np.rad2deg(np.arccos(r64["cos_parallax"][truth])).min()
            dev = deviations(r32, r64, sel)
            print(f"scene {seed} {method}: compared {sel.mean():.3f}, smallest inlier parallax {par:.2f} deg, fp32 - fp64: {dev}")
            assert sel.mean() >= 0.75 and sel[truth].all() and par >= 3.4
            assert max(dev["points"], dev["depth_a"], dev["depth_b"]) < 5e-4 and dev["reproj"] < 1e-3 and dev["cos_parallax"] < 2e-6
            assert not np.isnan(r32["points"]).any() and np.array_equal(r32["finite"], r64["finite"])


def test_triangulate_entry_point_validates_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 32)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    inf = float("inf")

    def call(m=a, Ka=a, R=a, t=a, P=1, N=4, method=0, outs=(a, a, a, a, a, a), max_reproj=inf, max_cos=1.0):
        return lib.roma_triangulate(m, None, Ka, a, R, t, None, P, N, method, max_reproj, max_cos, *outs, None)

    for kw in ({"m": None}, {"Ka": None}, {"R": None}, {"t": None}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"roma_triangulate: null pointer" in lib.roma_last_error()
    assert call(outs=(None,) * 6) == _lib.ROMA_E_ARG and b"every output is null" in lib.roma_last_error()
    for kw in ({"P": 0}, {"P": -1}, {"N": 0}, {"N": -5}, {"P": 65536}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    for method in (2, -1):
        assert call(method=method) == _lib.ROMA_E_ARG and b"unknown method" in lib.roma_last_error()
    assert call(max_reproj=float("nan")) == _lib.ROMA_E_ARG and b"NaN" in lib.roma_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 8)
    assert call(m=odd) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()


def test_new_functions_refuse_cpu_tensors_and_bad_arguments():
    from roma_amd import geometry
    x = torch.rand(100, 2) * 500
    K = torch.eye(3, dtype=torch.float64)
    R, t = torch.eye(3, dtype=torch.float64), torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.triangulate(x, x, R, t, K, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.depth_from_warp(torch.rand(8, 16, 4), torch.rand(8, 16), R, t, K, K, 480, 640)
    for fn in (lambda **kw: geometry.triangulate(x, x, R, t, K, K, **kw),
               lambda **kw: geometry.depth_from_warp(torch.rand(8, 16, 4), torch.rand(8, 16), R, t, K, K, 480, 640, **kw)):
        with pytest.raises(ValueError, match="unknown method 'dlt'"):
            fn(method="dlt")
        with pytest.raises(ValueError, match="min_parallax_deg"):
            fn(min_parallax_deg=-1.0)
        with pytest.raises(ValueError, match="max_reproj_error"):
            fn(max_reproj_error=-2.0)


def test_triangulate_kernel_uses_no_scratch_and_spills_nothing():
    """The compiler's resource report of csrc/triangulate.hip (the recipe of test_pose.py); LDS holds the pair constants only."""
    kernels = kernel_resources("triangulate.hip")
    assert sum("triangulate_kernel" in k for k in kernels) == 2, sorted(kernels)
    for name, k in kernels.items():
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] <= 256, (name, k)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _fields(tri):
    """a Triangulation -> the restatement's dict of numpy arrays"""
    return {"points": tri.points.cpu().numpy(), "depth_a": tri.depth_A.cpu().numpy(), "depth_b": tri.depth_B.cpu().numpy(),
            "reproj": tri.reproj_error.cpu().numpy(), "cos_parallax": tri.cos_parallax.cpu().numpy(), "valid": tri.valid.cpu().numpy()}


def _run(m, K, R, t, **kw):
    from roma_amd import geometry
    m = dev(m)
    return geometry.triangulate(m[..., :2], m[..., 2:], dev(R), dev(t), dev(K), dev(K), **kw)


def _assert_within(o, r, sel, tol, what):
    dev = deviations(o, r, sel)
    print(f"{what}: device - fp64 restatement {dev}; tolerance {tol}")
    for k in FIELDS:
        assert dev[k] <= tol[k], (what, k, dev[k], tol[k])


GUARD = 64


def _raw(m, Ka, Kb, R, t, method=0, want=FIELDS + ("valid",), mask=None, max_reproj=float("inf"), max_cos=1.0):
    """roma_triangulate itself on device tensors, each requested output allocated with a guard band behind its P * N elements
    (asserted untouched); outputs that are not wanted are passed as NULL.  Returns {name: tensor}."""
    P, N = m.shape[0], m.shape[1]
    bufs, ptrs = {}, []
    for name in FIELDS + ("valid",):
        if name not in want:
            ptrs.append(None)
            continue
        k = 3 if name == "points" else 1
        bufs[name] = torch.full((P * N * k + GUARD,), 171 if name == "valid" else -7.5, dtype=torch.uint8 if name == "valid" else torch.float32,
                                device=DEV)
        ptrs.append(bufs[name].data_ptr())
    rc = _lib.load().roma_triangulate(m.data_ptr(), None, Ka.data_ptr(), Kb.data_ptr(), R.data_ptr(), t.data_ptr(),
                                      None if mask is None else mask.data_ptr(), P, N, method, max_reproj, max_cos, *ptrs,
                                      torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "roma_triangulate")
    torch.cuda.synchronize()
    out = {}
    for name, b in bufs.items():
        k = 3 if name == "points" else 1
        assert bool((b[P * N * k:] == (171 if name == "valid" else -7.5)).all()), f"{name}: the guard band was written"
        out[name] = b[:P * N * k].reshape((P, N, 3) if name == "points" else (P, N)).clone()
    return out


@pytest.mark.gpu
def test_triangulate_parity_with_the_restatement():
    excused_total = 0
    for seed in range(3):
        m, truth, _, K, R, t = scene(seed)
        for method in T.METHODS:
            r64, r32 = ref(seed, 1000, method), ref(seed, 1000, method, "float32")
            sel = compared(r64)
            assert sel.mean() >= 0.75 and sel[truth].all()
            tol = tolerance(r64, r32, sel)
            tri = _run(m, K, R, t, method=method, max_reproj_error=2.0, min_parallax_deg=MIN_PARALLAX_DEG)
            assert tri.points.shape == (1000, 3) and tri.points.dtype == torch.float32 and tri.valid.dtype == torch.bool
            assert tri.depth_A.shape == (1000,) and tri.reproj_error.dtype == torch.float32
            o = _fields(tri)
            assert all(np.isfinite(o[k]).all() for k in FIELDS)
            _assert_within(o, r64, sel, tol, f"scene {seed} {method}")
            # valid, with the gates of this call, against the restatement's wherever no gated quantity is within the tolerance of its gate
            want = r64["valid"] & (r64["reproj"] <= 2.0) & (r64["cos_parallax"] <= COS_MIN_PARALLAX)
            nrm = np.linalg.norm(r64["points"], axis=-1)
            near = (np.abs(r64["reproj"] - 2.0) <= tol["reproj"] * np.maximum(r64["reproj"], 1.0)) \
                | (np.abs(r64["cos_parallax"] - COS_MIN_PARALLAX) <= tol["cos_parallax"]) \
                | (np.abs(r64["depth_a"]) <= tol["depth_a"] * nrm) | (np.abs(r64["depth_b"]) <= tol["depth_b"] * nrm)
            differ = o["valid"] != want
            print(f"scene {seed} {method}: valid {int(o['valid'].sum())} / {int(want.sum())}, {int(differ.sum())} differ, {int(near.sum())} "
                  f"within the tolerance of a gate")
            assert near.mean() <= 0.005
            assert not (differ & ~near).any()
            assert o["valid"][truth].mean() > 0.9                          # 2 px keeps the inliers of sigma = 0.5 px
            excused_total += int(near.sum())
    print(f"{excused_total} matches excused in all")


def _three_pairs(N):
    """three scenes with three poses, each seen through intrinsics of its own: (m (3,N,4) float32, Ka, Kb (3,3,3), R (3,3,3), t (3,3))"""
    ms, Kas, Kbs, Rs, ts = [], [], [], [], []
    for i, seed in enumerate((0, 1, 2)):
        m, _, _, K, R, t = scene(seed)
        Ka = np.array([[800.0 + 40 * i, 0.5 * i, 512.0 - 10 * i], [0, 780.0 + 25 * i, 384.0 + 7 * i], [0, 0, 1]])
        Kb = np.array([[760.0 - 30 * i, -0.3 * i, 500.0 + 12 * i], [0, 810.0 - 15 * i, 390.0 - 9 * i], [0, 0, 1]])
        h = np.ones((len(m), 1))
        xa = (np.concatenate([m[:, :2].astype(np.float64), h], -1) @ (Ka @ np.linalg.inv(K)).T)[:, :2]
        xb = (np.concatenate([m[:, 2:].astype(np.float64), h], -1) @ (Kb @ np.linalg.inv(K)).T)[:, :2]
        ms.append(np.concatenate([xa, xb], -1).astype(np.float32)[:N])
        Kas.append(Ka), Kbs.append(Kb), Rs.append(R), ts.append(t * (1.0 + 0.5 * i))
    return np.stack(ms), np.stack(Kas), np.stack(Kbs), np.stack(Rs), np.stack(ts)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_triangulate_shapes_batches_null_outputs_and_guard_bands(N):
    full_m, Ka, Kb, R, t = _three_pairs(1000)
    m = full_m[:, :N]
    dm, dKa, dKb, dR, dt = (dev(v) for v in (m, Ka, Kb, R, t))
    for method in (0, 1):
        every = _raw(dm, dKa, dKb, dR, dt, method, max_reproj=3.0, max_cos=COS_MIN_PARALLAX)
        assert all(torch.isfinite(every[k]).all() for k in FIELDS) and int(every["valid"].max()) <= 1
        if N >= 63:
            assert int(every["valid"].sum()) > 0
        # a pair alone computes bit for bit what it computes inside the batch
        for p in range(3):
            alone = _raw(dm[p:p + 1].clone(), dKa[p:p + 1].clone(), dKb[p:p + 1].clone(), dR[p:p + 1].clone(), dt[p:p + 1].clone(), method,
                         max_reproj=3.0, max_cos=COS_MIN_PARALLAX)
            assert all(torch.equal(alone[k][0], every[k][p]) for k in every), (method, p)
        # each output alone, the other five NULL
        for k in every:
            one = _raw(dm, dKa, dKb, dR, dt, method, want=(k,), max_reproj=3.0, max_cos=COS_MIN_PARALLAX)
            assert list(one) == [k] and torch.equal(one[k], every[k]), (method, k)
        # the first N matches of the N = 1000 call
        if N < 1000:
            big = _raw(dev(full_m), dKa, dKb, dR, dt, method, max_reproj=3.0, max_cos=COS_MIN_PARALLAX)
            assert all(torch.equal(big[k][:, :N], every[k]) for k in every), method
        # and the pairs really differ: against the restatement with each pair's own cameras and pose
        if N == 1000:
            for p in range(3):
                r64 = T.triangulate(m[p], Ka[p], Kb[p], R[p], t[p], T.METHODS[method])
                r32 = T.triangulate(m[p], Ka[p], Kb[p], R[p], t[p], T.METHODS[method], dtype=np.float32)
                sel = compared(r64)
                o = {k: every[k][p].cpu().numpy() for k in FIELDS}
                _assert_within(o, r64, sel, tolerance(r64, r32, sel), f"pair {p} method {method}")


@pytest.mark.gpu
def test_triangulate_defined_behaviour_on_bad_input():
    m, truth, _, K, R, t = scene(1)
    for method in T.METHODS:
        base = _fields(_run(m, K, R, t, method=method))
        bad = m.copy()
        rows = np.array([0, 5, 63, 64, 500, 999])
        bad[rows[0], 0], bad[rows[1], 1], bad[rows[2], 2], bad[rows[3], 3] = np.nan, np.inf, -np.inf, np.nan
        bad[rows[4]], bad[rows[5], 1:3] = np.nan, np.inf
        o = _fields(_run(bad, K, R, t, method=method))
        keep = np.ones(1000, bool)
        keep[rows] = False
        for k in FIELDS + ("valid",):
            assert not o[k][rows].any(), (method, k)                              # exact zeros, valid 0
            assert np.array_equal(o[k][keep], base[k][keep]), (method, k)         # and nobody else notices
        # mask 0 -> valid 0, values as without the mask
        mask = np.arange(1000) % 3 != 0
        o = _fields(_run(m, K, R, t, method=method, mask=dev(mask)))
        assert np.array_equal(o["valid"], base["valid"] & mask) and all(np.array_equal(o[k], base[k]) for k in FIELDS)
        # t = 0: no NaN or inf anywhere and no valid match
        o = _fields(_run(m, K, R, np.zeros(3), method=method))
        assert all(np.isfinite(o[k]).all() for k in FIELDS) and not o["valid"].any()
        # a singular K: the same
        Ks = K.copy()
        Ks[1, 1] = 0.0
        from roma_amd import geometry
        dm = dev(m)
        tri = geometry.triangulate(dm[:, :2], dm[:, 2:], dev(R), dev(t), dev(Ks), dev(K), method=method)
        assert all(not _fields(tri)[k].any() for k in FIELDS + ("valid",))
        # the gates narrow valid monotonically, exactly by the reported quantities, and change nothing else
        last = base["valid"]
        for px in (8.0, 2.0, 0.5, 0.0):
            o = _fields(_run(m, K, R, t, method=method, max_reproj_error=px))
            assert np.array_equal(o["valid"], base["valid"] & (base["reproj"] <= np.float32(px))) and not (o["valid"] & ~last).any()
            assert all(np.array_equal(o[k], base[k]) for k in FIELDS)
            last = o["valid"]
        assert int(last.sum()) < int(base["valid"].sum())
        last = base["valid"]
        for deg in (0.5, 2.0, 5.0, 20.0):
            o = _fields(_run(m, K, R, t, method=method, min_parallax_deg=deg))
            assert np.array_equal(o["valid"], base["valid"] & (base["cos_parallax"] <= np.float32(math.cos(math.radians(deg)))))
            assert not (o["valid"] & ~last).any() and all(np.array_equal(o[k], base[k]) for k in FIELDS)
            last = o["valid"]
        assert int(last.sum()) < int(base["valid"].sum()) and base["valid"][truth].all()


@pytest.mark.gpu
def test_triangulate_accuracy_on_the_device():
    for seed in range(5):
        m, truth, clean, K, R, t = scene(seed, 2000)
        za = T.triangulate(clean[truth], K, K, R, t, "midpoint")["depth_a"]               # the clean truth
        o, mid = _fields(_run(m, K, R, t, method="optimal")), _fields(_run(m, K, R, t, method="midpoint"))
        eo, em = float((o["reproj"][truth].astype(np.float64) ** 2).mean()), float((mid["reproj"][truth].astype(np.float64) ** 2).mean())
        med = float(np.median(np.abs(o["depth_a"][truth] / za - 1)))
        med_ref = float(np.median(np.abs(ref(seed, 2000, "optimal")["depth_a"][truth] / za - 1)))
        print(f"scene {seed}: mean squared reprojection error of the inliers optimal {eo:.4f} / midpoint {em:.4f} px^2; median relative "
              f"depth error {med:.5f} (fp64 restatement {med_ref:.5f})")
        assert o["valid"][truth].all() and mid["valid"][truth].all()
        assert eo < em
        assert med <= 4 * med_ref


# ------------------------------------------------------------------------------------------------------------------ depth_from_warp
H_IMG, W_IMG = G.H_IMG, G.W_IMG


def _normalised_grid(H, W):
    x, y = np.meshgrid(np.linspace(-1 + 1 / W, 1 - 1 / W, W), np.linspace(-1 + 1 / H, 1 - 1 / H, H), indexing="xy")
    return np.stack([x, y], -1)


def _to_px(c):
    return np.stack([W_IMG / 2 * (c[..., 0] + 1), H_IMG / 2 * (c[..., 1] + 1)], -1)


def _to_norm(x):
    return np.stack([2 / W_IMG * x[..., 0] - 1, 2 / H_IMG * x[..., 1] - 1], -1)


def _project(X, K):
    p = X @ K.T
    return p[..., :2] / p[..., 2:]


@functools.lru_cache(maxsize=None)
def synthetic_warp(seed, H=16, W=16):
    """A symmetric warp (H, 2W, 4) float32 of a scene with known depths in [4, 12]: left half [grid_A, x_B of the point at depth
    d_A], right half [x_A of the point at depth d_B in B, grid_B], in normalised coordinates.  Returns warp, d_A, d_B (H,W), K, R, t."""
    rng = np.random.default_rng(1000 + seed)
    K, R, t = PR.scene_pose(seed)
    g = _normalised_grid(H, W)
    u = np.concatenate([_to_px(g), np.ones((H, W, 1))], -1) @ np.linalg.inv(K).T
    dA, dB = rng.uniform(4, 12, (H, W)), rng.uniform(4, 12, (H, W))
    XA = u * dA[..., None]
    XinB = XA @ R.T + t
    XB = u * dB[..., None]                                       # in B's frame
    XinA = (XB - t) @ R
    assert (XinB[..., 2] > 1).all() and (XinA[..., 2] > 1).all()
    left = np.concatenate([g, _to_norm(_project(XinB, K))], -1)
    right = np.concatenate([_to_norm(_project(XinA, K)), g], -1)
    return np.concatenate([left, right], 1).astype(np.float32), dA, dB, K, R, t


def _warp_reference(warp, K, R, t, dtype=np.float64):
    return T.triangulate(warp.reshape(-1, 4), K, K, R, t, "optimal", to_px=T.to_px_of(H_IMG, W_IMG, H_IMG, W_IMG), dtype=dtype)


@pytest.mark.gpu
def test_depth_from_warp_on_a_synthetic_warp():
    from roma_amd import geometry
    from roma_amd.matcher import RegressionMatcher
    H = W = 16
    outs = []
    for seed in (0, 1):
        warp, dA, dB, K, R, t = synthetic_warp(seed)
        r64, r32 = _warp_reference(warp, K, R, t), _warp_reference(warp, K, R, t, np.float32)
        sel = compared(r64)
        assert sel.all()
        tol = tolerance(r64, r32, sel)
        # the fp64 restatement of the fp32 warp is the truth up to the rounding of the warp: 2^-24 * W_IMG / 2 = 3e-5 px against a
        # disparity of f |t| / z >= 60 px
        zA, zB = r64["depth_a"].reshape(H, 2 * W)[:, :W], r64["depth_b"].reshape(H, 2 * W)[:, W:]
        assert np.abs(zA / dA - 1).max() < 1e-5 and np.abs(zB / dB - 1).max() < 1e-5
        cert = torch.ones(H, 2 * W, device=DEV)
        out = geometry.depth_from_warp(dev(warp), cert, dev(R), dev(t), dev(K), dev(K), H_IMG, W_IMG)
        assert out.depth_A.shape == (H, W) and out.depth_B.shape == (H, W) and out.valid_A.shape == (H, W) and out.valid_B.shape == (H, W)
        assert out.points.shape == (H, 2 * W, 3) and out.valid.shape == (H, 2 * W) and out.depth_A.dtype == torch.float32
        assert bool(out.valid.all()) and torch.equal(out.valid[:, :W], out.valid_A) and torch.equal(out.valid[:, W:], out.valid_B)
        eA = float(np.abs(out.depth_A.cpu().numpy() / zA - 1).max())
        eB = float(np.abs(out.depth_B.cpu().numpy() / zB - 1).max())
        eP = float((np.linalg.norm(out.points.cpu().numpy().reshape(-1, 3) - r64["points"], axis=-1) / np.linalg.norm(r64["points"], axis=-1)).max())
        print(f"warp {seed}: depth_A {eA:.2e}, depth_B {eB:.2e}, points {eP:.2e} relative to the fp64 restatement; tolerance {tol}")
        assert eA <= tol["depth_a"] and eB <= tol["depth_b"] and eP <= tol["points"]
        assert float(np.abs(out.depth_A.cpu().numpy() / dA - 1).max()) <= tol["depth_a"] + 1e-5
        assert float(np.abs(out.depth_B.cpu().numpy() / dB - 1).max()) <= tol["depth_b"] + 1e-5
        # triangulate on to_pixel_coordinates of the flattened warp: the same up to the fused s * c + o of the kernel
        kA, kB = RegressionMatcher(None, None).to_pixel_coordinates(dev(warp).reshape(-1, 4), H_IMG, W_IMG, H_IMG, W_IMG)
        tri = geometry.triangulate(kA, kB, dev(R), dev(t), dev(K), dev(K))
        o = _fields(tri)
        flat = {"points": out.points.cpu().numpy().reshape(-1, 3)}
        assert float((np.linalg.norm(flat["points"] - o["points"], axis=-1) / np.linalg.norm(o["points"], axis=-1)).max()) <= tol["points"]
        assert float(np.abs(out.depth_A.cpu().numpy() / o["depth_a"].reshape(H, 2 * W)[:, :W] - 1).max()) <= tol["depth_a"]
        assert float(np.abs(out.depth_B.cpu().numpy() / o["depth_b"].reshape(H, 2 * W)[:, W:] - 1).max()) <= tol["depth_b"]
        # a certainty below the threshold, or a cleared mask, zeroes exactly those pixels
        rng = np.random.default_rng(seed)
        low, off = rng.random((H, 2 * W)) < 0.2, rng.random((H, 2 * W)) < 0.2
        cert2 = torch.where(dev(low), 0.04, 0.06)
        for kw, gone in (({}, low), ({"mask": dev(~off)}, low | off), ({"mask": dev((~off).astype(np.float32))}, low | off)):
            part = geometry.depth_from_warp(dev(warp), cert2, dev(R), dev(t), dev(K), dev(K), H_IMG, W_IMG, H_IMG, W_IMG, **kw)
            gone_d = dev(gone)
            assert torch.equal(part.valid, ~gone_d) and torch.equal(part.points, out.points)
            assert torch.equal(part.depth_A, torch.where(gone_d[:, :W], 0.0, out.depth_A))
            assert torch.equal(part.depth_B, torch.where(gone_d[:, W:], 0.0, out.depth_B))
        none = geometry.depth_from_warp(dev(warp), cert2, dev(R), dev(t), dev(K), dev(K), H_IMG, W_IMG, certainty_thresh=0.5)
        assert not bool(none.valid.any()) and not bool(none.depth_A.any()) and not bool(none.depth_B.any())
        # a warp that is not symmetric: the A half only
        half = geometry.depth_from_warp(dev(warp[:, :W]), cert[:, :W], dev(R), dev(t), dev(K), dev(K), H_IMG, W_IMG, symmetric=False)
        assert half.depth_B is None and half.valid_B is None and torch.equal(half.depth_A, out.depth_A) and half.points.shape == (H, W, 3)
        outs.append((warp, K, R, t, out))
    # the stack of both, each with its own pose
    stack = geometry.depth_from_warp(dev(np.stack([o[0] for o in outs])), torch.ones(2, H, 2 * W, device=DEV), dev(np.stack([o[2] for o in outs])),
                                     dev(np.stack([o[3] for o in outs])), dev(outs[0][1]), dev(outs[0][1]), H_IMG, W_IMG)
    assert stack.depth_A.shape == (2, H, W) and stack.points.shape == (2, H, 2 * W, 3) and stack.valid.shape == (2, H, 2 * W)
    for i, (_, _, _, _, out) in enumerate(outs):
        assert torch.equal(stack.depth_A[i], out.depth_A) and torch.equal(stack.depth_B[i], out.depth_B)
        assert torch.equal(stack.points[i], out.points) and torch.equal(stack.valid_B[i], out.valid_B)


@pytest.mark.gpu
def test_depth_from_warp_on_a_real_match():
    """match -> sample -> estimate_pose -> depth_from_warp at the smallest configuration of the suite (synthetic weights: the pose
    means nothing, the plumbing is what is checked)."""
    from roma_amd import geometry
    from roma_amd.model_zoo import build_roma
    from roma_amd.synthetic import load_synthetic_weights, synthetic_pair
    torch.set_grad_enabled(False)
    model = build_roma((112, 112), upsample_preds=True, amp_dtype=torch.float32)
    load_synthetic_weights(model, seed=0)
    model.upsample_res = (168, 168)
    model = model.to(DEV).eval()
    warp, cert = model.match_tensors(*(v.to(DEV) for v in synthetic_pair(0, (112, 112), (168, 168))))
    warp, cert = warp[0], cert[0]
    assert warp.shape == (168, 336, 4)
    mt, _ = model.sample(warp, cert, num=500, seed=0)
    kA, kB = model.to_pixel_coordinates(mt, 480, 640, 480, 640)
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    R, t, _ = geometry.estimate_pose(kA, kB, K, K, 1.0 / 500, max_iters=500, seed=0)
    fb = model.conf_from_fb_consistency(warp[:, :168, 2:], warp[:, 168:, :2], th=2)
    assert fb.shape == (168, 168) and fb.dtype == torch.float32
    for kw in ({}, {"method": "midpoint", "mask": torch.cat([fb, torch.ones_like(fb)], 1)}):
        out = geometry.depth_from_warp(warp, cert, R, t, K, K, 480, 640, certainty_thresh=-1.0, **kw)
        assert out.depth_A.shape == (168, 168) and out.depth_B.shape == (168, 168) and out.points.shape == (168, 336, 3)
        assert out.valid.shape == (168, 336) and out.valid.dtype == torch.bool
        assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in (out.depth_A, out.depth_B, out.points))
        assert bool((out.depth_A[out.valid_A] > 0).all()) and not bool(out.depth_A[~out.valid_A].any())
    assert int(geometry.depth_from_warp(warp, cert, R, t, K, K, 480, 640, certainty_thresh=-1.0).valid.sum()) > 0


@pytest.mark.gpu
def test_triangulation_graph_capture_replays_the_eager_result():
    from roma_amd import geometry
    m, _, _, K, R, t = scene(2)
    dm, dK, dR, dt = dev(m), dev(K), dev(R), dev(t)
    xa, xb = dm[:, :2].contiguous(), dm[:, 2:].contiguous()
    warp, _, _, Kw, Rw, tw = synthetic_warp(0)
    dw, cert, dKw, dRw, dtw = dev(warp), torch.full((16, 32), 0.5, device=DEV), dev(Kw), dev(Rw), dev(tw)

    def both():
        a = geometry.triangulate(xa, xb, dR, dt, dK, dK, max_reproj_error=2.0, min_parallax_deg=1.0)
        b = geometry.depth_from_warp(dw, cert, dRw, dtw, dKw, dKw, H_IMG, W_IMG)
        return (a.points, a.depth_A, a.depth_B, a.reproj_error, a.cos_parallax, a.valid, b.depth_A, b.valid_A, b.depth_B, b.valid_B, b.points,
                b.valid)

    eager = both()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert int(out[5].sum()) > 500 and bool(out[11].all())
