"""Robust two-view geometry on the device: the estimator that follows match -> sample -> to_pixel_coordinates.

`find_fundamental` replaces cv2.findFundamentalMat (demo/demo_fundamental.py:28-34, estimate_pose_uncalibrated in
romatch/utils/utils.py:54-62) and `find_homography` replaces cv2.findHomography (hpatches_sequences_homog_benchmark.py:72-86).
RANSAC with a fixed number of minimal samples (7-point F, 4-point DLT H, fp64, Hartley-normalised), MSAC scoring in fp32,
lowest cost wins, then least-squares local optimisation (kernels in csrc/geometry.hip).  Every sample is
drawn and scored; there is no early stop.  The draw is a pure function of the seed (tests/geometry_ref.py restates it).
No host synchronisation: a call can be captured in a hipGraph.  Tensors must live on a ROCm device; there is no CPU path.

Every estimator takes scoring="msac" (the default, described above) or scoring="magsac": MAGSAC++ sigma-consensus scoring
(Barath et al., CVPR 2020) and iteratively re-weighted local optimisation.  With "magsac" the threshold is only an UPPER BOUND on the
noise — the residual above which a match is an outlier, still what the returned mask uses — and the score marginalises over the
noise scale below it: use it when the noise level is not known and the threshold has to be generous (several times the noise).
At a threshold already tuned to the noise (about 3 sigma) "msac" is the more accurate one.  DESIGN.md §3.4 has the definition and
the measurements; parity with OpenCV's USAC_MAGSAC is not claimed (its threshold means something else).

`find_essential`, `recover_pose`, `estimate_pose` and `estimate_pose_uncalibrated` are the calibrated counterpart (csrc/essential.hip):
the 5-point solver on K^-1 x, the same scoring and selection, local optimisation on the essential manifold, and the cheirality
vote of cv2.recoverPose — what the reference's pose benchmarks run per pair on the host (romatch/utils/utils.py:12-76).

`refine_pose` polishes a pose by Levenberg-Marquardt on the truncated Sampson cost (csrc/pose_refine.hip), and
`estimate_relative_pose` chains find_essential -> recover_pose -> refine_pose behind the signature of
poselib.estimate_relative_pose, the call of the reference's PoseLib benchmark
(romatch/benchmarks/megadepth_pose_estimation_benchmark_poselib.py:82-95).  `pose_error` is compute_pose_error on the device.

`refine_fundamental` is the same polish for the uncalibrated path (csrc/fundamental_refine.hip): Levenberg-Marquardt on the truncated
Sampson cost in pixels over the rank-2 manifold, what cv2.findFundamentalMat runs after consensus.  `find_fundamental` and
`estimate_pose_uncalibrated` run it on request (refine_iters > 0).

`refine_homography` is that polish for a homography (csrc/homography_refine.hip): Levenberg-Marquardt on the truncated forward
transfer cost in the pixels of image B, what cv2.findHomography(..., cv2.RANSAC) runs on its inliers after consensus — the call of
the reference's HPatches benchmark (hpatches_sequences_homog_benchmark.py:80-86).  `find_homography` runs it on request
(refine_iters > 0), and `homography_corner_error` is that benchmark's metric (lines 92-103) on the device.

`triangulate` turns matches and a relative pose into 3-D points, depths, reprojection errors and a validity flag per match
(csrc/triangulate.hip: fp32 per match from pair constants prepared in fp64; Lindstrom's optimal correction or the midpoint), and
`depth_from_warp` does so for every row of the dense warp of match() in one launch: a depth map per image.

`warp_kpts` and `get_gt_warp` are the reference's ground-truth warp from two depth maps and a relative pose (romatch/utils/utils.py:
326-455; csrc/depth_warp.hip, fp64 per point as there), and `dense_match_metrics` / `geometric_dist` the dense MegaDepth benchmark's
EPE and PCK@1/3/5 of a warp against it (romatch/benchmarks/megadepth_dense_benchmark.py:17-42), fused into one pass.

`find_absolute_pose`, `refine_absolute_pose` and `estimate_absolute_pose` place a further image against 3-D points (csrc/
absolute_pose.hip): P3P RANSAC on 2D-3D matches, x ~ K (R X + t), scored by the reprojection error in pixels, and Levenberg-Marquardt
on the truncated reprojection cost — what a host path calls cv2.solvePnPRansac or poselib.estimate_absolute_pose for.  The points come
from `triangulate` (camera A's frame, in baselines), from `depth_from_warp`, or from a depth map through `lift_keypoints`;
`absolute_pose_error` is the metric (camera centre and rotation).

`triangulate_nview` triangulates tracks seen in V posed views from all of them, leaving out the views that disagree (csrc/
triangulate_nview.hip: fp32 per point, relative to the mean camera centre, from view constants prepared in fp64; a pairwise robust
choice of the views, the point closest to their rays, Levenberg-Marquardt on the pixel error), and `depth_from_warps` runs it on the k
warps of one image against k others, read in place: one depth map of that image from all of them.

`find_similarity` and `refine_similarity` register two point clouds given row by row, Y ~ s R X + t (csrc/similarity.hip): 3-point
RANSAC with Umeyama's closed form (the rotation by Horn's quaternion), scored by the distance in Y's units, and the closed form
iterated on the truncated cost — what brings two reconstructions, each in units of its own baseline, into one frame.
`register_depth_maps` does it for two depth maps of one image; `apply_similarity`, `transform_cameras` and `similarity_error` are the
torch helpers around them.

`build_tracks` joins the sampled matches of M image pairs over V views into multi-view tracks (csrc/tracks.hip): endpoints are
quantised to cells of a few pixels, each cell is represented by its most certain endpoint, the matches are the edges of a lock-free
union-find, and every component with at most one cell per view becomes a row of the `(V,T,2)` observations and `(V,T)` visibility
that `triangulate_nview` takes — the step between `sample_batch` and structure, exact and independent of thread order.

`bundle_adjust` refines the cameras and the points of one reconstruction together (csrc/bundle.hip): Levenberg-Marquardt on the
truncated reprojection cost in fp64, the points eliminated per point and the cameras solved through the reduced (Schur-complement)
system, sums in a fixed order, the decision to keep a step taken on the device — the polish after `build_tracks`, the pose calls and
`triangulate_nview`, which each fit one kind while holding the other.  `reconstruction_error` is its metric: the worst rotation and
centre error and the median point error after a closed-form similarity alignment of the camera centres.

`average_rotations`, `global_positions` and `initialize_cameras` deliver the start that `bundle_adjust` asks for (csrc/
motion_average.hip): the rotations of V views averaged over the pose graph of the pairwise `estimate_pose` results (spanning tree, then
re-weighted least squares on the Lie algebra, L1 first), and under those rotations the camera centres and the points from the tracks —
the linear known-rotation problem, the points eliminated one by one and the centres the smallest eigenvector of the reduced matrix,
re-weighted from a majority vote of the pairwise translation directions.

`fuse_depth_maps` is the dense counterpart (csrc/depth_fuse.hip): the depth maps of V posed views — `depth_from_warps` once per image —
are checked against one another by forward-backward reprojection in fp64, every pixel keeps the views that agree with it and the mean
of their depths, each surface point is owned by the lowest view that sees it, and the owners are compacted in a fixed order into one
cloud of a fixed shape.

`render_points` looks at that cloud again from a camera (csrc/render_points.hip): a z-buffered point splat into the depth maps of V
posed views by a 64-bit integer atomic minimum — the nearest point per pixel, whatever order the points arrive in — and per point the
views that see it and those in which a nearer surface is in the way.
"""
from __future__ import annotations

import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import check
from .ops import _need_gpu, _stream

KIND_F, KIND_H = 0, 1
KIND_E = 2                            # this module's name for the essential estimator; the C ABI has entry points of its own for it
_KIND_AP, _KIND_SIM = 3, 4            # and for absolute pose and 3-D similarity, which have no public name for theirs
_WORKSPACE_LIMIT = 192 << 20          # workspace bytes of one call; larger batches run in chunks of pairs that share it
# One RANSAC estimator: its C entry points, the regions its workspace function lays out, the points of a minimal sample, the slots
# (models) per sample, and `lead`, the C arguments in front of the points (the kind, for F and H, which share their entry points).
# Behind the points come the per-pair constants (K_A, K_B for E, K for absolute pose) and behind `scoring` the scalars of the model
# (with_scale for similarity): those are values of a call, which _ransac and _inspect take as `consts` and `tail`.
_Estimator = collections.namedtuple("_Estimator", "workspace hypotheses select regions smin slots lead")
_ENTRIES = {
    KIND_F: _Estimator("roma_ransac_workspace", "roma_ransac_hypotheses_ex", "roma_ransac_select_ex", 9, 7, 3, (KIND_F,)),
    KIND_H: _Estimator("roma_ransac_workspace", "roma_ransac_hypotheses_ex", "roma_ransac_select_ex", 9, 4, 1, (KIND_H,)),
    KIND_E: _Estimator("roma_essential_workspace", "roma_essential_hypotheses_ex", "roma_essential_select_ex", 10, 5, 10, ()),
    _KIND_AP: _Estimator("roma_absolute_pose_workspace", "roma_absolute_pose_hypotheses", "roma_absolute_pose_select", 12, 3, 4, ()),
    _KIND_SIM: _Estimator("roma_similarity_workspace", "roma_similarity_hypotheses", "roma_similarity_select", 12, 3, 1, ()),
}


def _kind(model):
    if model in ("fundamental", "F", KIND_F):
        return KIND_F
    if model in ("homography", "H", KIND_H):
        return KIND_H
    if model in ("essential", "E", KIND_E):
        return KIND_E
    raise ValueError(f"unknown model {model!r}: 'fundamental', 'homography' or 'essential'")


def _prepare(a, b, wa, wb, smin, form, what, rows, differ=None, gpu_first=False):
    """The two point sets of a call, a (N,wa) or (P,N,wa) and b (N,wb) or (P,N,wb), fp32/fp64 device tensors -> contiguous (P,N,wa),
    (P,N,wb) fp64, single-pair flag.  form / differ: the messages for a wrong shape (formatted with the two shapes), what / rows: the
    nouns of the dtype and the count message; gpu_first: whether the device is checked before the shapes or after the counts."""
    if gpu_first:
        _need_gpu(a, b)
    if differ and a.shape != b.shape:
        raise ValueError(differ.format(tuple(a.shape), tuple(b.shape)))
    if a.dim() not in (2, 3) or a.shape[-1] != wa or b.shape != a.shape[:-1] + (wb,):
        raise ValueError(form.format(tuple(a.shape), tuple(b.shape)))
    for t in (a, b):
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what} must be float32 or float64, got {t.dtype}")
    single = a.dim() == 2
    P, N = (1, a.shape[0]) if single else (a.shape[0], a.shape[1])
    if N < smin:
        raise ValueError(f"{N} {rows}, the minimal sample needs {smin}")
    if P < 1:
        raise ValueError("empty batch")
    if not gpu_first:
        _need_gpu(a, b)
    return a.reshape(P, N, wa).to(torch.float64).contiguous(), b.reshape(P, N, wb).to(torch.float64).contiguous(), single


def _points(x_A, x_B, kind):
    """(N,2) or (P,N,2) fp32/fp64 device tensors -> contiguous (P,N,2) fp64, single-pair flag."""
    return _prepare(x_A, x_B, 2, 2, _ENTRIES[kind].smin, "expected (N,2) or (P,N,2) pixel coordinates, got {0}", "pixel coordinates",
                    "matches", differ="x_A {0} and x_B {1} differ in shape", gpu_first=True)


def _mask(mask, P, N, points=None):
    """The optional mask of a call, bool / uint8 -> contiguous (P,N) uint8, or None.  points: the caller's x_A, (N,2) or (P,N,2), whose
    (N,) or (P,N) the mask must have; None where the caller has checked the shape itself."""
    if mask is None:
        return None
    _need_gpu(mask)
    if points is not None and mask.shape != ((N,) if points.dim() == 2 else (P, N)):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the points {tuple(points.shape)}")
    return mask.reshape(P, N).to(torch.uint8).contiguous()


def _seed(seed):
    # like RegressionMatcher.sample: torch's CPU generator, no device sync
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if seed is None else int(seed) & 0xFFFFFFFF


def _scoring(scoring):
    """"msac" / "magsac" -> the C ABI's code; checked before anything looks at a tensor"""
    if scoring == "msac":
        return _lib.SCORE_MSAC
    if scoring == "magsac":
        return _lib.SCORE_MAGSAC
    raise ValueError(f"unknown scoring {scoring!r}: 'msac' or 'magsac'")


def _args(threshold, max_iters, lo_iters):
    if not threshold > 0:
        raise ValueError(f"threshold must be positive, got {threshold}")
    if int(max_iters) < 1:
        raise ValueError(f"max_iters must be positive, got {max_iters}")
    if int(lo_iters) < 0:
        raise ValueError(f"lo_iters must be >= 0, got {lo_iters}")


def _workspace_layout(entry, regions, *shape):
    """(total bytes, [region offsets]) from the library's `entry`(*shape, offsets); raises ValueError on a shape it refuses"""
    off = (ctypes.c_long * regions)()
    total = getattr(_lib.load(), entry)(*shape, ctypes.cast(off, ctypes.c_void_p))
    if total < 0:
        check(int(total), entry)
    return int(total), list(off)


def workspace_layout(kind, P, N, iters):
    """(total bytes, [region offsets]) of the workspace (include/roma_hip.h: the 9 regions of roma_ransac_workspace, the 10 of
    roma_essential_workspace for KIND_E)."""
    est = _ENTRIES[kind]
    return _workspace_layout(est.workspace, est.regions, *est.lead, P, N, iters)


def _chunks(kind, P, N, iters):
    """Pair ranges [a, b) of one call: as few as keep a chunk's workspace within _WORKSPACE_LIMIT, of balanced size."""
    per_pair, _ = workspace_layout(kind, 1, N, iters)
    most = max(1, _WORKSPACE_LIMIT // per_pair)
    n = -(-P // most)
    step = -(-P // n)
    return [(p0, min(P, p0 + step)) for p0 in range(0, P, step)]


def _ap_chunks(P, N, iters):
    """_chunks for absolute pose, under the name it had when each estimator had a chunker of its own"""
    return _chunks(_KIND_AP, P, N, iters)


def _sim_chunks(P, N, iters):
    """_chunks for similarity, likewise"""
    return _chunks(_KIND_SIM, P, N, iters)


def _intrinsics(K, P, device, name):
    """(3,3) (shared by the batch) or (P,3,3), tensor or numpy -> contiguous (P,3,3) fp64 on the device."""
    if not torch.is_tensor(K):
        K = torch.as_tensor(K, dtype=torch.float64).to(device)
    _need_gpu(K)
    if K.shape not in ((3, 3), (P, 3, 3)):
        raise ValueError(f"{name}: expected (3,3) or ({P},3,3) intrinsics, got {tuple(K.shape)}")
    return K.to(torch.float64).expand(P, 3, 3).contiguous()


def _inverse_intrinsics(K):
    """K^-1 of upper-triangular K (..., 3, 3) with last row 0 0 1, in closed form as the kernels do (no host synchronisation; inf / NaN
    for a singular K)."""
    fx, s, cx, fy, cy = K[..., 0, 0], K[..., 0, 1], K[..., 0, 2], K[..., 1, 1], K[..., 1, 2]
    T = torch.zeros_like(K)
    T[..., 0, 0] = 1.0 / fx
    T[..., 0, 1] = -s / (fx * fy)
    T[..., 0, 2] = (s * cy - cx * fy) / (fx * fy)
    T[..., 1, 1] = 1.0 / fy
    T[..., 1, 2] = -cy / fy
    T[..., 2, 2] = 1.0
    return T


def _front(kind, a, b, consts, tail, threshold, iters, score):
    """the C arguments that an estimator's hypotheses and select entries share, up to and including the scalars behind `scoring`"""
    return (*_ENTRIES[kind].lead, a.data_ptr(), b.data_ptr(), *(c.data_ptr() for c in consts), a.shape[0], a.shape[1], iters,
            float(threshold), score, *tail)


def _hypotheses(kind, a, b, consts, tail, threshold, iters, score, seed, p0, ws):
    entry = _ENTRIES[kind].hypotheses
    check(getattr(_lib.load(), entry)(*_front(kind, a, b, consts, tail, threshold, iters, score), seed, p0, ws.data_ptr(), ws.numel(),
                                      _stream()), entry)


def _ransac(kind, a, b, consts, tail, threshold, iters, score, seed, lo_iters, outs):
    """The RANSAC of every estimator, on prepared inputs: a, b the (P,N,.) fp64 points, consts the per-pair constant tensors (P,...),
    tail the scalars behind `scoring`, outs the (P,...) tensors the select entry fills, in its order."""
    select, P, N = _ENTRIES[kind].select, a.shape[0], a.shape[1]
    lib = _lib.load()
    chunks = _chunks(kind, P, N, iters)
    # one workspace, sized for the widest chunk, serves every chunk in stream order (a narrower chunk's layout is no larger)
    total, _ = workspace_layout(kind, max(p1 - p0 for p0, p1 in chunks), N, iters)
    ws = torch.empty((total,), dtype=torch.uint8, device=a.device)
    for p0, p1 in chunks:
        ca, cb, cc = a[p0:p1], b[p0:p1], [c[p0:p1] for c in consts]
        _hypotheses(kind, ca, cb, cc, tail, threshold, iters, score, seed, p0, ws)
        check(getattr(lib, select)(*_front(kind, ca, cb, cc, tail, threshold, iters, score), int(lo_iters), ws.data_ptr(), total,
                                   *(o[p0:p1].data_ptr() for o in outs), _stream()), select)


def _estimate(x_A, x_B, kind, threshold, max_iters, seed, lo_iters, K_A=None, K_B=None, scoring="msac"):
    score = _scoring(scoring)
    _args(threshold, max_iters, lo_iters)
    xa, xb, single = _points(x_A, x_B, kind)
    P, N = xa.shape[0], xa.shape[1]
    K = (_intrinsics(K_A, P, xa.device, "K_A"), _intrinsics(K_B, P, xa.device, "K_B")) if kind == KIND_E else ()
    model = torch.empty((P, 3, 3), dtype=torch.float64, device=xa.device)
    mask = torch.empty((P, N), dtype=torch.uint8, device=xa.device)
    _ransac(kind, xa, xb, K, (), threshold, int(max_iters), score, _seed(seed), lo_iters, (model, mask))
    mask = mask.bool()
    return (model[0], mask[0]) if single else (model, mask)


def _refine_iters(refine_iters):
    try:
        n = int(refine_iters)
    except (TypeError, ValueError):                     # e.g. a scoring name passed by position: scoring is keyword-only
        raise TypeError(f"refine_iters must be an integer, got {refine_iters!r}") from None
    if n < 0:
        raise ValueError(f"refine_iters must be >= 0, got {refine_iters}")
    return n


def find_fundamental(x_A, x_B, threshold=3.0, max_iters=10000, seed=None, lo_iters=3, refine_iters=0, *, scoring="msac"):
    """Fundamental matrix F (x_B^T F x_A = 0) of pixel correspondences x_A <-> x_B, (N,2) or (P,N,2), fp32/fp64 on the device.
    Returns (F fp64 (3,3) or (P,3,3), unit Frobenius norm, largest-magnitude entry positive; inlier mask bool (N,) or (P,N)):
    Sampson error below threshold (pixels).  All zeros and an empty mask when no sample gives a model.
    refine_iters > 0 polishes the RANSAC model by refine_fundamental on all matches at the same threshold (at most that many
    Levenberg-Marquardt steps) and returns the refined model's mask; 0, the default, returns the RANSAC model as it is.
    scoring: "msac" or "magsac" (module docstring); the refinement keeps its truncated Sampson cost either way."""
    _scoring(scoring)
    refine_iters = _refine_iters(refine_iters)
    F, mask = _estimate(x_A, x_B, KIND_F, threshold, max_iters, seed, lo_iters, scoring=scoring)
    if refine_iters == 0:
        return F, mask
    return refine_fundamental(F, x_A, x_B, threshold, refine_iters)


def find_homography(x_A, x_B, threshold=3.0, max_iters=2000, seed=None, lo_iters=3, refine_iters=0, *, scoring="msac"):
    """Homography H (x_B ~ H x_A) of pixel correspondences, shapes as find_fundamental.  Returns (H fp64 with H[2,2] = 1 — unit
    Frobenius norm if |H[2,2]| < 1e-12 |H| —, inlier mask: forward transfer error below threshold).  refine_iters > 0 polishes the
    RANSAC model by refine_homography on all matches at the same threshold (at most that many Levenberg-Marquardt steps) and returns
    the refined model's mask; 0, the default, returns the RANSAC model as it is.  scoring: "msac" or "magsac"; the refinement keeps
    its truncated transfer cost either way."""
    _scoring(scoring)
    refine_iters = _refine_iters(refine_iters)
    H, mask = _estimate(x_A, x_B, KIND_H, threshold, max_iters, seed, lo_iters, scoring=scoring)
    if refine_iters == 0:
        return H, mask
    return refine_homography(H, x_A, x_B, threshold, refine_iters)


def find_essential(x_A, x_B, K_A, K_B, threshold, max_iters=2000, seed=None, lo_iters=3, *, scoring="msac"):
    """Essential matrix E (x_hat_B^T E x_hat_A = 0, x_hat = K^-1 x) of PIXEL correspondences x_A <-> x_B, (N,2) or (P,N,2), fp32/fp64 on
    the device; K_A, K_B: (3,3) (shared by the batch) or (P,3,3) intrinsics, tensors or numpy, upper triangular with last row 0 0 1.
    threshold is in calibrated units (the reference's norm_thresh, e.g. 0.5 px / focal length): inlier when the Sampson error of the
    calibrated points is below it.  Returns (E fp64 (3,3) or (P,3,3) with singular values (1, 1, 0) / sqrt 2 and its largest-magnitude
    entry positive; inlier mask bool).  All zeros and an empty mask when no sample gives a model, e.g. for a singular K.
    max_iters = 2000 samples of 5 points, up to 10 models each, every one scored: there is no confidence exit, so the number of
    samples is the whole budget.  At 30 % inliers (1 - 0.3^5)^2000 = 0.8 % of the calls draw no clean sample, at 40 % 1e-9; raise
    max_iters for harder pairs.  scoring: "msac" or "magsac" (module docstring)."""
    return _estimate(x_A, x_B, KIND_E, threshold, max_iters, seed, lo_iters, K_A, K_B, scoring=scoring)


def recover_pose(E, x_A, x_B, K_A, K_B, mask=None):
    """Relative pose (R, t) of camera B with respect to A (X_B = R X_A + t, |t| = 1) from an essential matrix — of find_essential, or
    K_B^T F K_A of find_fundamental — by the cheirality vote of cv2.recoverPose: of the four decompositions the one under which most
    matches of `mask` (bool / uint8, default all) have positive depth in both cameras.  E (3,3) or (P,3,3); points and intrinsics as
    find_essential.  Returns (R fp64 (3,3) / (P,3,3), t fp64 (3,) / (P,3), the mask narrowed to the matches that passed — what the
    reference's estimate_pose returns).  A zero E gives R = I, t = 0 and an empty mask."""
    _need_gpu(E)
    xa, xb, single = _points(x_A, x_B, KIND_E)
    P, N = xa.shape[0], xa.shape[1]
    if E.shape != ((3, 3) if single else (P, 3, 3)):
        raise ValueError(f"E {tuple(E.shape)} does not match the points {tuple(x_A.shape)}")
    Ka, Kb = _intrinsics(K_A, P, xa.device, "K_A"), _intrinsics(K_B, P, xa.device, "K_B")
    e = E.reshape(P, 3, 3).to(torch.float64).contiguous()
    m = _mask(mask, P, N, x_A)
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=xa.device)
    t = torch.empty((P, 3), dtype=torch.float64, device=xa.device)
    count = torch.empty((P,), dtype=torch.int32, device=xa.device)
    out = torch.empty((P, N), dtype=torch.uint8, device=xa.device)
    check(_lib.load().roma_recover_pose(xa.data_ptr(), xb.data_ptr(), Ka.data_ptr(), Kb.data_ptr(), e.data_ptr(),
                                        None if m is None else m.data_ptr(), P, N, R.data_ptr(), t.data_ptr(), count.data_ptr(),
                                        out.data_ptr(), _stream()), "roma_recover_pose")
    out = out.bool()
    return (R[0], t[0], out[0]) if single else (R, t, out)


def estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, *, max_iters=2000, seed=None, scoring="msac"):
    """Drop-in for estimate_pose of the reference (romatch/utils/utils.py:31-52) on the device: find_essential, then recover_pose on
    its inliers.  None for fewer than 5 matches, else (R, t, mask) — batched tensors for (P,N,2) input.  `conf` is accepted for the
    signature and unused: every one of the max_iters samples is drawn and scored, there is no early stop.  scoring as find_essential."""
    _scoring(scoring)
    if kpts0.shape[-2] < 5:
        return None
    E, mask = find_essential(kpts0, kpts1, K0, K1, norm_thresh, max_iters=max_iters, seed=seed, scoring=scoring)
    return recover_pose(E, kpts0, kpts1, K0, K1, mask)


def estimate_pose_uncalibrated(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, *, max_iters=10000, seed=None, refine_iters=0,
                               scoring="msac"):
    """Drop-in for estimate_pose_uncalibrated of the reference (utils.py:54-76): find_fundamental with norm_thresh in PIXELS, E =
    K1^T F K0, recover_pose on the inliers of F.  None for fewer than 5 matches (find_fundamental itself needs 7).  `conf` unused.
    refine_iters > 0: the pose comes from the F that refine_fundamental polished (see find_fundamental) and from its inliers.
    scoring as find_fundamental (the reference calls cv2.findFundamentalMat with USAC_ACCURATE here)."""
    _scoring(scoring)
    refine_iters = _refine_iters(refine_iters)
    if kpts0.shape[-2] < 5:
        return None
    F, mask = find_fundamental(kpts0, kpts1, threshold=norm_thresh, max_iters=max_iters, seed=seed, refine_iters=refine_iters,
                               scoring=scoring)
    P = 1 if F.dim() == 2 else F.shape[0]
    Ka, Kb = _intrinsics(K0, P, F.device, "K0"), _intrinsics(K1, P, F.device, "K1")
    if F.dim() == 2:
        Ka, Kb = Ka[0], Kb[0]
    return recover_pose(Kb.transpose(-1, -2) @ F @ Ka, kpts0, kpts1, Ka, Kb, mask)


def _refine_args(threshold, iters):
    if not float(threshold) > 0:
        raise ValueError(f"threshold must be positive, got {threshold}")
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")


def _refined(res, info, single, return_info):
    """What a refine_* call returns from its batched outputs: res = (the model(s), mask), of the one pair where the call was for one, and
    on request the dict info = (cost, count, steps)"""
    if single:
        res = tuple([v[0] for v in res])
    if not return_info:
        return res
    cost, count, steps = info
    return res + ({"cost": cost[0], "count": count[0], "steps": steps[0]} if single else {"cost": cost, "count": count, "steps": steps},)


def _run_refine(entry, inputs, P, N, scalars, *shapes):
    """A refine_* entry point on prepared (P,...) tensors: entry(inputs (None: a null pointer)..., P, N, scalars..., outputs..., stream).
    Allocates the outputs every one of them has — an fp64 model tensor (P, *shape) per shape, the (P,N) mask, cost, count, steps — and
    returns (models..., mask bool), (cost, count, steps)."""
    dev = inputs[0].device
    models = [torch.empty((P,) + shape, dtype=torch.float64, device=dev) for shape in shapes]
    out = torch.empty((P, N), dtype=torch.uint8, device=dev)
    info = (torch.empty((P,), dtype=torch.float64, device=dev), torch.empty((P,), dtype=torch.int32, device=dev),
            torch.empty((P,), dtype=torch.int32, device=dev))
    check(getattr(_lib.load(), entry)(*(None if v is None else v.data_ptr() for v in inputs), P, N, *scalars,
                                      *(o.data_ptr() for o in (*models, out, *info)), _stream()), entry)
    return (*models, out.bool()), info


def _refine(R, t, x_A, x_B, K_A, K_B, threshold, iters, mask):
    """refine_pose on batched outputs: (R (P,3,3), t (P,3), mask (P,N) bool), (cost (P,) fp64, count (P,) int32, steps (P,) int32), single"""
    _need_gpu(R, t)
    _refine_args(threshold, iters)
    xa, xb, single = _points(x_A, x_B, KIND_E)
    P, N = xa.shape[0], xa.shape[1]
    if R.shape != ((3, 3) if single else (P, 3, 3)) or t.shape != ((3,) if single else (P, 3)):
        raise ValueError(f"R {tuple(R.shape)}, t {tuple(t.shape)} do not match the points {tuple(x_A.shape)}")
    Ka, Kb = _intrinsics(K_A, P, xa.device, "K_A"), _intrinsics(K_B, P, xa.device, "K_B")
    r0 = R.reshape(P, 3, 3).to(torch.float64).contiguous()
    t0 = t.reshape(P, 3).to(torch.float64).contiguous()
    m = _mask(mask, P, N, x_A)
    return _run_refine("roma_refine_pose", (xa, xb, Ka, Kb, r0, t0, m), P, N, (float(threshold), int(iters)), (3, 3), (3,)) + (single,)


def refine_pose(R, t, x_A, x_B, K_A, K_B, threshold, iters=15, mask=None, return_info=False):
    """Non-linear refinement of a relative pose (R, t) — of recover_pose / estimate_pose — on the matches it was estimated from:
    Levenberg-Marquardt, at most `iters` steps, on the sum over the matches of min(r^2, threshold^2), r the Sampson residual of the
    calibrated points under E = [t]x R (threshold in calibrated units, as find_essential).  Matches beyond the threshold carry no
    weight (the truncated loss, the MSAC score of the estimator), and `mask` (bool / uint8) optionally names the only matches that
    may carry any.  R (3,3) or (P,3,3), t (3,) or (P,3); points and intrinsics as recover_pose.  Returns (R orthonormal fp64, t unit
    fp64, mask bool: r^2 < threshold^2 under the returned pose); with return_info also a dict of device tensors: cost (fp64, the
    truncated cost of the returned pose), count (int32, its inliers), steps (int32, the steps kept).  A step is kept only if it
    lowers the cost, so the returned pose never has a higher cost than the given one; a pair that cannot be refined (fewer than 5
    weighted matches, a singular normal matrix, a pose that is not finite) gets its pose back unchanged."""
    return _refined(*_refine(R, t, x_A, x_B, K_A, K_B, threshold, iters, mask), return_info)


def _refine_model(M, x_A, x_B, kind, least, entry, threshold, iters, mask, return_info):
    """what refine_fundamental and refine_homography run alike: the checks, the outputs and the call of the C entry point `entry`"""
    name = "F" if kind == KIND_F else "H"
    _need_gpu(M)
    _refine_args(threshold, iters)
    xa, xb, single = _points(x_A, x_B, kind)
    P, N = xa.shape[0], xa.shape[1]
    if N < least:
        raise ValueError(f"{N} matches, the refinement needs {least}")
    if M.shape != ((3, 3) if single else (P, 3, 3)):
        raise ValueError(f"{name} {tuple(M.shape)} does not match the points {tuple(x_A.shape)}")
    m0 = M.reshape(P, 3, 3).to(torch.float64).contiguous()
    m = _mask(mask, P, N, x_A)
    return _refined(*_run_refine(entry, (xa, xb, m0, m), P, N, (float(threshold), int(iters)), (3, 3)), single, return_info)


def refine_fundamental(F, x_A, x_B, threshold=3.0, iters=15, mask=None, return_info=False):
    """Non-linear refinement of a fundamental matrix F — of find_fundamental — on the matches it was estimated from: Levenberg-
    Marquardt, at most `iters` steps, on the sum over the matches of min(r^2, threshold^2), r the Sampson residual in pixels (what
    find_fundamental scores with), over the rank-2 matrices (F^ = U diag(1, s, 0) V^T in normalised coordinates).  Matches beyond the
    threshold carry no weight, and `mask` (bool / uint8) optionally names the only matches that may carry any.  F (3,3) or (P,3,3);
    points as find_fundamental.  Returns (F fp64, mask bool: r^2 < threshold^2 under the returned model); with return_info also a
    dict of device tensors: cost (fp64, the truncated cost of the returned model), count (int32, its inliers), steps (int32, the
    steps kept).  A pair comes back either as a rank-2 model of unit Frobenius norm, largest-magnitude entry positive, of strictly
    lower cost than the given F, or — no step lowered the cost, fewer than 8 weighted matches, a singular normal matrix, an F that is
    not finite or has rank below 2 — as the given F bit for bit, with steps = 0."""
    return _refine_model(F, x_A, x_B, KIND_F, 8, "roma_refine_fundamental", threshold, iters, mask, return_info)


def refine_homography(H, x_A, x_B, threshold=3.0, iters=15, mask=None, return_info=False):
    """Non-linear refinement of a homography H — of find_homography — on the matches it was estimated from: Levenberg-Marquardt, at
    most `iters` steps, on the sum over the matches of min(e, threshold^2), e the squared forward transfer error in the pixels of
    image B (what find_homography scores with), over 8 entries of the Hartley-normalised H with its largest entry held.  Matches
    beyond the threshold carry no weight, and `mask` (bool / uint8) optionally names the only matches that may carry any.  H (3,3)
    or (P,3,3); points as find_homography.  Returns (H fp64, mask bool: e < threshold^2 under the returned model); with return_info
    also a dict of device tensors: cost (fp64, the truncated cost of the returned model), count (int32, its inliers), steps (int32,
    the steps kept).  A pair comes back either as a model with H[2,2] = 1 (find_homography's convention) of strictly lower cost than
    the given H, or — no step lowered the cost, fewer than 4 weighted matches, a singular normal matrix, an H that is not finite or
    is all zero — as the given H bit for bit, with steps = 0."""
    return _refine_model(H, x_A, x_B, KIND_H, 4, "roma_refine_homography", threshold, iters, mask, return_info)


def homography_corner_error(H, H_gt, w, h, scale=1.0):
    """The metric of the reference's HPatches benchmark (hpatches_sequences_homog_benchmark.py:92-103) in torch on the device,
    batched: the mean distance in pixels between the corners (0,0), (0,h-1), (w-1,0), (w-1,h-1) of image A warped by H and by H_gt,
    divided by `scale` (the benchmark passes min(w2, h2) / 480).  H, H_gt (...,3,3), H_gt a tensor or numpy; fp64.  An all-zero H —
    find_homography's "no model" — gives inf."""
    _need_gpu(H)
    H = H.to(torch.float64)
    H_gt = torch.as_tensor(H_gt).to(device=H.device, dtype=torch.float64)
    c = torch.tensor([[0, 0, 1], [0, h - 1, 1], [w - 1, 0, 1], [w - 1, h - 1, 1]], dtype=torch.float64).to(H.device)
    a, b = c @ H.transpose(-1, -2), c @ H_gt.transpose(-1, -2)
    d = torch.linalg.norm(a[..., :2] / a[..., 2:] - b[..., :2] / b[..., 2:], dim=-1).mean(-1) / scale
    return torch.where(torch.isnan(d) & ~H.any(-1).any(-1), torch.full_like(d, float("inf")), d)


class RelativePose:
    """What estimate_relative_pose returns in place of poselib.CameraPose: R (3,3) / (P,3,3), t (3,) / (P,3) (unit), Rt = [R | t]
    (3,4) / (P,3,4), fp64 device tensors."""
    __slots__ = ("R", "t")

    def __init__(self, R, t):
        self.R, self.t = R, t

    @property
    def Rt(self):
        return torch.cat([self.R, self.t.unsqueeze(-1)], -1)

    def __repr__(self):
        return f"RelativePose(R={tuple(self.R.shape)}, t={tuple(self.t.shape)}, device={self.R.device})"


_RANSAC_OPT = {"max_epipolar_error": 1.0, "max_iterations": 2000, "min_inliers": 5, "refine_iterations": 15, "max_reproj_error": None}


def _focal(camera, name):
    if not isinstance(camera, dict) or camera.get("model") != "PINHOLE":
        model = camera.get("model") if isinstance(camera, dict) else type(camera).__name__
        raise ValueError(f"{name}: camera model {model!r} is not supported, only 'PINHOLE' with params = [fx, fy, cx, cy]")
    params = [float(v) for v in camera["params"]]
    if len(params) != 4:
        raise ValueError(f"{name}: a PINHOLE camera has 4 params [fx, fy, cx, cy], got {len(params)}")
    fx, fy, cx, cy = params
    return 0.5 * (fx + fy), [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]


def estimate_relative_pose(kpts0, kpts1, camera0, camera1, ransac_opt=None, *, seed=None, scoring="msac"):
    """Drop-in for poselib.estimate_relative_pose as the reference's PoseLib benchmark calls it, on the device: find_essential ->
    recover_pose -> refine_pose (RANSAC, cheirality, then Levenberg-Marquardt on the truncated Sampson cost of all matches).
    kpts0, kpts1: (N,2) or (P,N,2) pixel coordinates on the device; camera0, camera1: dicts with model 'PINHOLE' and params
    [fx, fy, cx, cy] (one camera per image for the whole batch).  ransac_opt keys:
      max_epipolar_error  pixels, default 1.0.  OUR DEFINITION of the calibrated threshold: max_epipolar_error * (1/f0 + 1/f1) / 2
                          with f = (fx + fy) / 2 of each camera
      max_iterations      default 2000 samples, not PoseLib's 10 000: there is no early exit here, every sample is drawn and
                          scored, so this is the whole budget and not a cap (see find_essential for what 2000 buys)
      min_inliers         default 5: a pair whose RANSAC pose has fewer inliers that pass cheirality keeps that pose unrefined
      refine_iterations   default 15 Levenberg-Marquardt steps
      max_reproj_error    accepted (the reference passes it) and unused: it belongs to PoseLib's absolute-pose estimators
    Any other key, or another camera model, raises ValueError.  Returns (pose, info): pose.R, pose.t, pose.Rt; info = {inliers: bool
    mask of the returned pose, num_inliers: int32, model_score: fp64 truncated cost, refinements: int32 steps kept — device tensors,
    nothing is copied to the host —, iterations: max_iterations}.  scoring: of find_essential; refine_pose keeps its truncated cost."""
    _scoring(scoring)
    opt = dict(_RANSAC_OPT)
    for k, v in (ransac_opt or {}).items():
        if k not in opt:
            raise ValueError(f"ransac_opt: unknown key {k!r}; known: {sorted(opt)}")
        opt[k] = v
    f0, K0 = _focal(camera0, "camera0")
    f1, K1 = _focal(camera1, "camera1")
    if not float(opt["max_epipolar_error"]) > 0:
        raise ValueError(f"ransac_opt: max_epipolar_error must be positive, got {opt['max_epipolar_error']}")
    if int(opt["max_iterations"]) < 1 or int(opt["min_inliers"]) < 0 or int(opt["refine_iterations"]) < 0:
        raise ValueError(f"ransac_opt: bad counts {opt}")
    _need_gpu(kpts0, kpts1)
    thr = float(opt["max_epipolar_error"]) * 0.5 * (1.0 / f0 + 1.0 / f1)
    K0 = torch.tensor(K0, dtype=torch.float64).to(kpts0.device)
    K1 = torch.tensor(K1, dtype=torch.float64).to(kpts0.device)
    E, emask = find_essential(kpts0, kpts1, K0, K1, thr, max_iters=int(opt["max_iterations"]), seed=seed, scoring=scoring)
    R0, t0, mask0 = recover_pose(E, kpts0, kpts1, K0, K1, emask)
    R, t, mask, refined = refine_pose(R0, t0, kpts0, kpts1, K0, K1, thr, int(opt["refine_iterations"]), return_info=True)
    cost, count, steps = refined["cost"], refined["count"], refined["steps"]
    keep = mask0.sum(-1) >= int(opt["min_inliers"])                  # on the device: no host synchronisation
    R = torch.where(keep[..., None, None], R, R0)
    t = torch.where(keep[..., None], t, t0)
    steps = torch.where(keep, steps, torch.zeros_like(steps))
    info = {"inliers": mask, "num_inliers": count, "model_score": cost, "iterations": int(opt["max_iterations"]), "refinements": steps}
    return RelativePose(R, t), info


def pose_error(R, t, T_gt):
    """compute_pose_error of the reference (romatch/utils/utils.py:116-134) in torch on the device, batched, so that a benchmark loop
    needs no copy to the host before its AUC: R (...,3,3), t (...,3) against T_gt (...,3,4) or (...,4,4) = [R_gt | t_gt] (tensor or
    numpy).  Returns (e_t, e_R) in degrees: the angle between the translation directions folded by the sign ambiguity of E,
    min(e, 180 - e), and the geodesic angle of R^T R_gt."""
    _need_gpu(R, t)
    T_gt = torch.as_tensor(T_gt).to(device=R.device, dtype=R.dtype)
    R_gt, t_gt = T_gt[..., :3, :3], T_gt[..., :3, 3]
    n = torch.linalg.norm(t, dim=-1) * torch.linalg.norm(t_gt, dim=-1)
    e_t = torch.rad2deg(torch.acos(torch.clamp((t * t_gt).sum(-1) / n, -1.0, 1.0)))
    e_t = torch.minimum(e_t, 180.0 - e_t)
    cos = ((R * R_gt).sum((-1, -2)) - 1.0) / 2.0                    # trace(R^T R_gt) = sum of the elementwise product
    e_R = torch.rad2deg(torch.acos(torch.clamp(cos, -1.0, 1.0)).abs())
    return e_t, e_R


def _view(ws, off, i, dtype, shape):
    n = 1
    for s in shape:
        n *= s
    item = torch.empty((), dtype=dtype).element_size()
    return ws[off[i]:off[i] + n * item].view(dtype).reshape(shape)


def _inspect(name, kind, a, b, consts, tail, threshold, max_iters, score, seed):
    """What the inspectors share: one hypotheses call on the whole batch, which `name` refuses beyond _WORKSPACE_LIMIT.  consts() gives
    the per-pair constant tensors once the batch is accepted; the other arguments as _ransac's.  Returns the views every estimator
    has — samples (P,iters,smin), valid, cost, count (P,iters,slots) —, view(region, dtype, shape behind P) for the estimator's own,
    and the constants."""
    est, P, N, iters = _ENTRIES[kind], a.shape[0], a.shape[1], int(max_iters)
    total, off = workspace_layout(kind, P, N, iters)
    if total > _WORKSPACE_LIMIT:
        raise ValueError(f"{name}: {P} pairs need a {total >> 20} MiB workspace, over the {_WORKSPACE_LIMIT >> 20} MiB "
                         "limit; call it on fewer pairs")
    ws = torch.empty((total,), dtype=torch.uint8, device=a.device)
    consts = consts()
    _hypotheses(kind, a, b, consts, tail, threshold, iters, score, _seed(seed), 0, ws)

    def view(region, dtype, shape):
        return _view(ws, off, region, dtype, (P,) + tuple(shape))

    slots = (iters, est.slots)
    return {"samples": view(2, torch.int32, (iters, est.smin)).clone(), "valid": view(4, torch.int32, slots) != 0,
            "cost": view(7, torch.float64, slots).clone(), "count": view(8, torch.int32, slots).clone()}, view, consts


def minimal_samples(x_A, x_B, model="fundamental", max_iters=10000, seed=0, K_A=None, K_B=None):
    """The indices each minimal sample draws: (P, max_iters, s) int32, s = 7 (F) / 4 (H) / 5 (E), a row of -1 for an invalid sample.
    An inspection helper like score_hypotheses, with its batch limit.  model = "essential" takes the intrinsics (default: identity)."""
    if _kind(model) == KIND_E and K_A is None and K_B is None:
        K_A = K_B = torch.eye(3, dtype=torch.float64, device=x_A.device)
    return score_hypotheses(x_A, x_B, model, 3.0, max_iters, seed, K_A, K_B)["samples"]


def score_hypotheses(x_A, x_B, model="fundamental", threshold=3.0, max_iters=10000, seed=0, K_A=None, K_B=None, *, scoring="msac"):
    """Every hypothesis of one call, before selection (batched (P,...) shapes even for a single pair):
    samples (P,iters,s) int32; models (P,iters,R,3,3) fp64 in normalised coordinates (unit Frobenius norm), R = 3 root slots
    for F, 1 for H; valid (P,iters,R) bool; count (P,iters,R) int32 inliers; cost (P,iters,R) fp64 cost of the chosen `scoring`, MSAC
    by default (+inf if invalid);
    T_A, T_B (P,3,3) fp64 normalising transforms (x_hat = T x).  A model in pixels is T_B^T F^ T_A or T_B^-1 H^ T_A.
    Pair p draws what it draws in find_fundamental / find_homography with the same seed.  An inspection helper: it keeps the
    whole batch's workspace and returns every slot, so it refuses a batch whose workspace exceeds the chunk limit of the
    estimators (192 MiB: about 35 pairs at N = 10 000 and 10 000 F samples) — call it on fewer pairs.
    model = "essential" needs K_A, K_B (as find_essential; threshold in calibrated units): R = 10 slots ordered by the solver's
    hidden variable, models in calibrated coordinates, T_A = K_A^-1, T_B = K_B^-1."""
    kind, score = _kind(model), _scoring(scoring)
    _args(threshold, max_iters, 0)
    xa, xb, _ = _points(x_A, x_B, kind)
    P = xa.shape[0]

    def intrinsics():
        if kind != KIND_E:
            return ()
        if K_A is None or K_B is None:
            raise ValueError("score_hypotheses: model 'essential' needs K_A and K_B")
        return _intrinsics(K_A, P, xa.device, "K_A"), _intrinsics(K_B, P, xa.device, "K_B")

    c, view, K = _inspect("score_hypotheses", kind, xa, xb, intrinsics, (), threshold, max_iters, score, seed)
    if kind == KIND_E:
        T = _inverse_intrinsics(torch.stack(K, 1))
    else:
        norm = view(0, torch.float64, (2, 4))
        T = torch.zeros((P, 2, 3, 3), dtype=torch.float64, device=xa.device)
        T[:, :, 0, 0] = norm[:, :, 2]
        T[:, :, 1, 1] = norm[:, :, 2]
        T[:, :, 0, 2] = -norm[:, :, 2] * norm[:, :, 0]
        T[:, :, 1, 2] = -norm[:, :, 2] * norm[:, :, 1]
        T[:, :, 2, 2] = 1.0
    return {"samples": c["samples"], "models": view(3, torch.float64, c["valid"].shape[1:] + (3, 3)).clone(), "valid": c["valid"],
            "cost": c["cost"], "count": c["count"], "T_A": T[:, 0].clone(), "T_B": T[:, 1].clone()}


# ------------------------------------------------------------------------------------------------------------ triangulation
_METHODS = {"optimal": 0, "midpoint": 1}


class Triangulation:
    """What triangulate returns: points (..., N, 3) in camera A's frame, depth_A, depth_B (the z in each camera), reproj_error
    (pixels), cos_parallax — fp32 —, valid (bool); all (..., N) device tensors."""
    __slots__ = ("points", "depth_A", "depth_B", "reproj_error", "cos_parallax", "valid")

    def __init__(self, points, depth_A, depth_B, reproj_error, cos_parallax, valid):
        self.points, self.depth_A, self.depth_B = points, depth_A, depth_B
        self.reproj_error, self.cos_parallax, self.valid = reproj_error, cos_parallax, valid

    def __repr__(self):
        return f"Triangulation(points={tuple(self.points.shape)}, device={self.points.device})"


class WarpDepth:
    """What depth_from_warp returns: depth_A (..., H, W) with valid_A, depth_B (..., H, W) with valid_B (None for a warp that is not
    symmetric) — fp32, 0 where not valid —, points (..., H, W or 2W, 3) in camera A's frame and valid (..., H, W or 2W) of every row."""
    __slots__ = ("depth_A", "valid_A", "depth_B", "valid_B", "points", "valid")

    def __init__(self, depth_A, valid_A, depth_B, valid_B, points, valid):
        self.depth_A, self.valid_A, self.depth_B, self.valid_B, self.points, self.valid = depth_A, valid_A, depth_B, valid_B, points, valid

    def __repr__(self):
        return f"WarpDepth(depth_A={tuple(self.depth_A.shape)}, points={tuple(self.points.shape)}, device={self.points.device})"


def _gates(method, max_reproj_error, min_parallax_deg):
    """-> (method code, max_reproj in pixels, max_cos_parallax), checked before anything looks at a tensor"""
    if method not in _METHODS:
        raise ValueError(f"unknown method {method!r}: 'optimal' or 'midpoint'")
    max_reproj = float("inf") if max_reproj_error is None else float(max_reproj_error)
    if not max_reproj >= 0:
        raise ValueError(f"max_reproj_error must be >= 0 pixels or None, got {max_reproj_error}")
    deg = float(min_parallax_deg)
    if not 0.0 <= deg <= 180.0:
        raise ValueError(f"min_parallax_deg must be in [0, 180], got {min_parallax_deg}")
    return _METHODS[method], max_reproj, (1.0 if deg == 0.0 else math.cos(math.radians(deg)))


def _pose(R, t, P, single, device):
    """(3,3) / (3,) or (P,3,3) / (P,3), tensor or numpy -> contiguous (P,3,3), (P,3) fp64 on the device"""
    if not torch.is_tensor(R):
        R = torch.as_tensor(R, dtype=torch.float64).to(device)
    if not torch.is_tensor(t):
        t = torch.as_tensor(t, dtype=torch.float64).to(device)
    _need_gpu(R, t)
    if (R.shape != (3, 3) or t.shape != (3,)) and (single or R.shape != (P, 3, 3) or t.shape != (P, 3)):
        raise ValueError(f"R {tuple(R.shape)}, t {tuple(t.shape)}: expected (3,3) and (3,)" + ("" if single else f", or ({P},3,3) and ({P},3)"))
    return R.to(torch.float64).expand(P, 3, 3).contiguous(), t.to(torch.float64).expand(P, 3).contiguous()


def _triangulate(m, to_px, R, t, K_A, K_B, single, code, max_reproj, max_cos, mask, want_all=True):
    """m: (P,N,4) device tensor of any float dtype -> the six outputs of roma_triangulate, batched"""
    P, N = m.shape[0], m.shape[1]
    if P < 1 or N < 1:
        raise ValueError(f"no matches: {P} pairs of {N}")
    m = m.to(torch.float32).contiguous()
    Ka, Kb = _intrinsics(K_A, P, m.device, "K_A"), _intrinsics(K_B, P, m.device, "K_B")
    Rp, tp = _pose(R, t, P, single, m.device)
    mk = _mask(mask, P, N)                                    # triangulate has checked its shape; depth_from_warp built it
    f32 = dict(dtype=torch.float32, device=m.device)
    points = torch.empty((P, N, 3), **f32)
    depth_a, depth_b = torch.empty((P, N), **f32), torch.empty((P, N), **f32)
    reproj, cosp = (torch.empty((P, N), **f32), torch.empty((P, N), **f32)) if want_all else (None, None)
    valid = torch.empty((P, N), dtype=torch.uint8, device=m.device)
    px = None if to_px is None else (ctypes.c_float * 8)(*to_px)
    check(_lib.load().roma_triangulate(m.data_ptr(), None if px is None else ctypes.cast(px, ctypes.c_void_p), Ka.data_ptr(), Kb.data_ptr(),
                                       Rp.data_ptr(), tp.data_ptr(), None if mk is None else mk.data_ptr(), P, N, code, max_reproj, max_cos,
                                       points.data_ptr(), depth_a.data_ptr(), depth_b.data_ptr(), None if reproj is None else reproj.data_ptr(),
                                       None if cosp is None else cosp.data_ptr(), valid.data_ptr(), _stream()), "roma_triangulate")
    return points, depth_a, depth_b, reproj, cosp, valid.bool()


def triangulate(x_A, x_B, R, t, K_A, K_B, *, method="optimal", max_reproj_error=None, min_parallax_deg=0.0, mask=None):
    """3-D points of pixel correspondences x_A <-> x_B under a known relative pose — of recover_pose / estimate_pose / refine_pose —
    in their convention x_B ~ K_B (R X_A + t) (csrc/triangulate.hip).  Points are in camera A's frame and in units of |t|: with the
    unit t of recover_pose, depths come out in baselines.
    x_A, x_B: (N,2) with R (3,3), t (3,), or (P,N,2) with (P,3,3), (P,3) or one shared pose; any float dtype on the device (the kernel
    computes in fp32 from pair constants prepared in fp64).  K_A, K_B: (3,3) shared or (P,3,3), as find_essential.
    method "optimal": Lindstrom's closed-form correction moves the match by the smallest pixel distance onto the epipolar line pair,
    the corrected rays meet in the point, reproj_error = that distance, sqrt(|d_A|^2 + |d_B|^2).  "midpoint": the middle of the two
    rays' closest points, reproj_error the root of the sum over both images of its squared reprojection distance; cheaper, never
    more accurate.  cos_parallax is the cosine of the angle between the two rays.
    valid: the match is finite, `mask` (bool / uint8, optional) is set, the solution is finite, both depths are positive,
    reproj_error <= max_reproj_error (pixels; None = no gate) and the parallax is at least min_parallax_deg.  Matches that are not
    finite, or have no finite solution (parallel rays, t = 0, a singular K), get zeros in every field; the others their values,
    valid or not.  Returns a Triangulation: points (N,3) / (P,N,3), depth_A, depth_B, reproj_error, cos_parallax fp32, valid bool.
    No host synchronisation: the call can be captured in a hipGraph."""
    code, max_reproj, max_cos = _gates(method, max_reproj_error, min_parallax_deg)
    _need_gpu(x_A, x_B)
    if x_A.shape != x_B.shape or x_A.dim() not in (2, 3) or x_A.shape[-1] != 2:
        raise ValueError(f"expected two (N,2) or (P,N,2) tensors of pixel coordinates, got {tuple(x_A.shape)} and {tuple(x_B.shape)}")
    if not (x_A.is_floating_point() and x_B.is_floating_point()):
        raise ValueError(f"pixel coordinates must be floating point, got {x_A.dtype} and {x_B.dtype}")
    single = x_A.dim() == 2
    P, N = (1, x_A.shape[0]) if single else (x_A.shape[0], x_A.shape[1])
    if mask is not None and mask.shape != ((N,) if single else (P, N)):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the points {tuple(x_A.shape)}")
    m = torch.cat((x_A.reshape(P, N, 2).float(), x_B.reshape(P, N, 2).float()), -1)
    out = _triangulate(m, None, R, t, K_A, K_B, single, code, max_reproj, max_cos, mask)
    return Triangulation(*((o[0] for o in out) if single else out))


def depth_from_warp(warp, certainty, R, t, K_A, K_B, H_A, W_A, H_B=None, W_B=None, *, certainty_thresh=0.05, method="optimal",
                    max_reproj_error=None, min_parallax_deg=0.0, mask=None, symmetric=True):
    """Dense depth maps of both images from the warp of match() and a relative pose (of estimate_pose on its sampled matches, say).
    warp: (H, 2W, 4) symmetric — the left half rows are [grid_A, predicted x_B], the right half [predicted x_A, grid_B] — or
    (P, H, 2W, 4) of match_tensors, in normalised coordinates; every row is an (x_A, x_B) match, and the whole array goes through
    triangulate's kernel in one launch, which maps it to pixels as to_pixel_coordinates(warp, H_A, W_A, H_B, W_B) does (H_B, W_B
    default to H_A, W_A).  K_A, K_B are the intrinsics at those image sizes; R, t, method, max_reproj_error, min_parallax_deg as
    triangulate.  A row counts only where certainty (H, 2W) > certainty_thresh and `mask` (same shape, optional — e.g. of
    RegressionMatcher.conf_from_fb_consistency) is set.  symmetric=False: the warp of a matcher that is not symmetric, (H, W, 4), every
    row [grid_A, predicted x_B]; it gives the A half only (the shape cannot tell the two apart, and looking at the grid would
    synchronise with the host).
    Returns a WarpDepth: depth_A (H,W) = z in camera A of the left half with valid_A, depth_B (H,W) = z in camera B of the right
    half with valid_B, 0 where not valid; points (H, 2W, 3) in A's frame and valid (H, 2W) of every row; a leading P if given."""
    code, max_reproj, max_cos = _gates(method, max_reproj_error, min_parallax_deg)
    _need_gpu(warp, certainty, mask)
    if warp.dim() not in (3, 4) or warp.shape[-1] != 4 or not warp.is_floating_point():
        raise ValueError(f"expected a floating-point warp (H, W2, 4) or (P, H, W2, 4), got {tuple(warp.shape)} {warp.dtype}")
    single = warp.dim() == 3
    P, H, W2 = (1,) + tuple(warp.shape[:2]) if single else tuple(warp.shape[:3])
    for name, v in (("certainty", certainty), ("mask", mask)):
        if v is not None and v.shape != warp.shape[:-1]:
            raise ValueError(f"{name} {tuple(v.shape)} does not match the warp {tuple(warp.shape)}")
    H_B, W_B = H_A if H_B is None else H_B, W_A if W_B is None else W_B
    to_px = (W_A / 2, W_A / 2, H_A / 2, H_A / 2, W_B / 2, W_B / 2, H_B / 2, H_B / 2)
    keep = certainty > certainty_thresh
    if mask is not None:
        keep = keep & (mask != 0)
    points, da, db, _, _, valid = _triangulate(warp.reshape(P, H * W2, 4), to_px, R, t, K_A, K_B, single, code, max_reproj, max_cos,
                                               keep.reshape(P, H * W2), want_all=False)
    points, valid = points.reshape(P, H, W2, 3), valid.reshape(P, H, W2)
    da, db = torch.where(valid, da.reshape(P, H, W2), 0.0), torch.where(valid, db.reshape(P, H, W2), 0.0)
    if symmetric and W2 % 2:
        raise ValueError(f"a symmetric warp has an even width, got {W2}; pass symmetric=False for an (H, W, 4) warp")
    W = W2 // 2 if symmetric else W2
    res = (da[..., :W], valid[..., :W], db[..., W:] if symmetric else None, valid[..., W:] if symmetric else None, points, valid)
    return WarpDepth(*((None if o is None else o[0]) for o in res) if single else res)


# ------------------------------------------------------------------------------------------------------ N-view triangulation
_MAX_VIEWS = 32


class MultiViewTriangulation:
    """What triangulate_nview returns, (N,) device tensors: points (N,3) fp32 in the world frame, depth (the z in view ref_view),
    reproj_error (pixels, the root of the MEAN over the used views of the squared error), cos_parallax — fp32 —, views (int32 holding
    the bit pattern of the views used: view v took part where (views >> v) & 1), num_views (uint8, their number), valid (bool)."""
    __slots__ = ("points", "depth", "reproj_error", "cos_parallax", "views", "num_views", "valid")

    def __init__(self, points, depth, reproj_error, cos_parallax, views, num_views, valid):
        self.points, self.depth, self.reproj_error, self.cos_parallax = points, depth, reproj_error, cos_parallax
        self.views, self.num_views, self.valid = views, num_views, valid

    def __repr__(self):
        return f"MultiViewTriangulation(points={tuple(self.points.shape)}, device={self.points.device})"


class MultiViewDepth:
    """What depth_from_warps returns: depth_A (H,W) fp32, 0 where not valid, valid_A (H,W) bool, num_views (H,W) uint8 (image A
    counts), reproj_error (H,W) fp32 and points (H,W,3) fp32 in camera A's frame."""
    __slots__ = ("depth_A", "valid_A", "num_views", "reproj_error", "points")

    def __init__(self, depth_A, valid_A, num_views, reproj_error, points):
        self.depth_A, self.valid_A, self.num_views, self.reproj_error, self.points = depth_A, valid_A, num_views, reproj_error, points

    def __repr__(self):
        return f"MultiViewDepth(depth_A={tuple(self.depth_A.shape)}, device={self.depth_A.device})"


def _nview_gates(max_view_error, iters, min_views, max_reproj_error, min_parallax_deg, ref_view):
    """-> (max_view_error or inf, iters, min_views, max_reproj, max_cos_parallax, ref_view), checked before anything looks at a tensor"""
    view_error = float("inf") if max_view_error is None else float(max_view_error)
    if not view_error > 0:
        raise ValueError(f"max_view_error must be positive pixels or None, got {max_view_error}")
    if not 0 <= int(iters) <= 10:
        raise ValueError(f"iters must be in [0, 10], got {iters}")
    if not 2 <= int(min_views) <= _MAX_VIEWS:
        raise ValueError(f"min_views must be at least 2 and at most the number of views, got {min_views}")
    if int(ref_view) < 0:
        raise ValueError(f"ref_view must be a view index, got {ref_view}")
    _, max_reproj, max_cos = _gates("midpoint", max_reproj_error, min_parallax_deg)
    return view_error, int(iters), int(min_views), max_reproj, max_cos, int(ref_view)


def _popcount(views):
    """the number of set bits of an int32 bit pattern, uint8"""
    x = views.to(torch.int64) & 0xFFFFFFFF
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return (((x * 0x01010101) >> 24) & 0xFF).to(torch.uint8)


def _triangulate_nview(obs, to_px, vis, vis_stride, K, R, t, rows, row_len, row_stride, point_stride, gates, device, keep):
    """roma_triangulate_nview on V observation pointers and optional visibility pointers (sequences of ints, or None); `keep` holds the tensors
    behind them.  -> points (N,3), depth, reproj, cos_parallax fp32, views int32, valid bool, N = rows * row_len"""
    V = len(obs)
    view_error, iters, min_views, max_reproj, max_cos, ref_view = gates
    if not 2 <= V <= _MAX_VIEWS:
        raise ValueError(f"{V} views: 2 to {_MAX_VIEWS} are supported")
    if min_views > V or ref_view >= V:
        raise ValueError(f"min_views {min_views} and ref_view {ref_view} do not fit {V} views")
    N = rows * row_len
    f32 = dict(dtype=torch.float32, device=device)
    points, depth, reproj, cosp = torch.empty((N, 3), **f32), torch.empty((N,), **f32), torch.empty((N,), **f32), torch.empty((N,), **f32)
    views = torch.empty((N,), dtype=torch.int32, device=device)
    valid = torch.empty((N,), dtype=torch.uint8, device=device)
    obs_tab = (ctypes.c_void_p * V)(*obs)
    px_tab = None if to_px is None else (ctypes.c_float * (4 * V))(*[float(s) for row in to_px for s in row])
    vis_tab = None if vis is None else (ctypes.c_void_p * V)(*vis)
    check(_lib.load().roma_triangulate_nview(ctypes.cast(obs_tab, ctypes.c_void_p), None if px_tab is None else ctypes.cast(px_tab, ctypes.c_void_p),
                                             None if vis_tab is None else ctypes.cast(vis_tab, ctypes.c_void_p), int(vis_stride),
                                             K.data_ptr(), R.data_ptr(), t.data_ptr(), V, rows, row_len, int(row_stride), int(point_stride),
                                             view_error, iters, min_views, ref_view, max_reproj, max_cos, points.data_ptr(), depth.data_ptr(),
                                             reproj.data_ptr(), cosp.data_ptr(), views.data_ptr(), valid.data_ptr(), _stream()),
          "roma_triangulate_nview")
    del keep                                                  # alive until the launch is queued; the stream orders the rest
    return points, depth, reproj, cosp, views, valid.bool()


def _poses(R, t, V, device):
    """(V,3,3), (V,3), tensors or numpy -> contiguous fp64 on the device"""
    if not torch.is_tensor(R):
        R = torch.as_tensor(R, dtype=torch.float64).to(device)
    if not torch.is_tensor(t):
        t = torch.as_tensor(t, dtype=torch.float64).to(device)
    _need_gpu(R, t)
    if R.shape != (V, 3, 3) or t.shape != (V, 3):
        raise ValueError(f"R {tuple(R.shape)}, t {tuple(t.shape)}: expected ({V},3,3) and ({V},3)")
    return R.to(torch.float64).contiguous(), t.to(torch.float64).contiguous()


def _threshold_px(threshold):
    thr = float(threshold)
    if not 0.0 < thr < 1e18:
        raise ValueError(f"threshold must be positive pixels, got {threshold}")
    return thr


def _observations(x, visible, min_views):
    """x (V,N,2), any float dtype, and visible (V,N) or None, as triangulate_nview, bundle_adjust and global_positions take them ->
    (xs fp32 contiguous, vis uint8 contiguous or None, V, N, the ctypes table of the V observation pointers, that of the V visibility
    pointers or None); the tables point into xs and vis, which the caller keeps alive until the launch is queued"""
    if x.dim() != 3 or x.shape[-1] != 2 or not x.is_floating_point():
        raise ValueError(f"expected floating-point observations (V,N,2), got {tuple(x.shape)} {x.dtype}")
    V, N = x.shape[0], x.shape[1]
    if not min_views <= V <= _MAX_VIEWS:
        raise ValueError(f"{V} views: {min_views} to {_MAX_VIEWS} are supported")
    if N < 1:
        raise ValueError("no points")
    if visible is not None and visible.shape != (V, N):
        raise ValueError(f"visible {tuple(visible.shape)} does not match the observations {tuple(x.shape)}")
    xs = x.to(torch.float32).contiguous()
    vis = None if visible is None else visible.to(torch.uint8).contiguous()
    obs_tab = (ctypes.c_void_p * V)(*[xs.data_ptr() + 8 * N * v for v in range(V)])
    vis_tab = None if vis is None else (ctypes.c_void_p * V)(*[vis.data_ptr() + N * v for v in range(V)])
    return xs, vis, V, N, obs_tab, vis_tab


def triangulate_nview(x, R, t, K, *, visible=None, max_view_error=None, iters=3, min_views=2, max_reproj_error=None, min_parallax_deg=0.0,
                      ref_view=0):
    """3-D points of tracks seen in V posed views (2 <= V <= 32), each triangulated from all the views that see it, with the views that
    disagree left out (csrc/triangulate_nview.hip) — what follows find_absolute_pose once a third camera is placed.  Convention of
    find_absolute_pose: x_v ~ K_v (R_v X + t_v); the points come out in the frame the poses are expressed in (camera A's, when view 0
    is the identity and the others come from estimate_pose / find_absolute_pose against triangulate's cloud).  One reconstruction per
    call: the views are the batch.
    x: (V,N,2) pixels, any float dtype on the device, NaN (or anything not finite) where a view does not see a point; visible: (V,N)
    bool / uint8, optional, the same as NaN where 0.  R (V,3,3), t (V,3); K (3,3) shared or (V,3,3).  A view with a singular K or a
    pose that is not finite sees nothing.
    max_view_error None: every observing view is used.  A number of pixels (robust mode): every pair of observing views proposes the
    midpoint of its two rays, a view agrees with positive depth and an error within max_view_error, the proposal whose own two views
    agree and whose truncated squared error over all views is lowest wins (the first pair on a tie), and the views that agree with it
    are used.  Then the point closest to the rays of the used views, polished by `iters` (0 to 10) Levenberg-Marquardt steps on the
    squared pixel error; a step is kept only if the error drops.
    Returns a MultiViewTriangulation: points (N,3), depth (z in view ref_view), reproj_error (root of the MEAN squared pixel error
    over the used views — triangulate reports the root of the SUM over its two), cos_parallax (the smallest cosine between the rays of
    two used views at the point: the largest triangulation angle) fp32; views int32, bit v set where view v was used, (views >> v) & 1;
    num_views uint8; valid bool: at least min_views views used, finite, in front of every used view, reproj_error <=
    max_reproj_error (None = no gate), parallax >= min_parallax_deg.  A point with fewer than two usable views or no finite solution
    gets zeros in every field; the others their values, valid or not.  The kernel computes in fp32 relative to the mean of the camera
    centres (prepared in fp64), so the result does not depend on where the world's origin is.  No host synchronisation: the call can
    be captured in a hipGraph."""
    gates = _nview_gates(max_view_error, iters, min_views, max_reproj_error, min_parallax_deg, ref_view)
    _need_gpu(x, visible)
    xs, vis, V, N, obs_tab, vis_tab = _observations(x, visible, 2)
    Rp, tp = _poses(R, t, V, x.device)
    Kp = _intrinsics(K, V, x.device, "K")
    points, depth, reproj, cosp, views, valid = _triangulate_nview(obs_tab, None, vis_tab, N, Kp, Rp, tp, 1, N, 0, 2, gates, x.device, (xs, vis))
    return MultiViewTriangulation(points, depth, reproj, cosp, views, _popcount(views), valid)


def depth_from_warps(warps, certainties, R, t, K_A, K, H_A, W_A, sizes=None, *, certainty_thresh=0.05, masks=None, symmetric=True,
                     max_view_error=None, iters=3, min_views=2, max_reproj_error=None, min_parallax_deg=0.0):
    """ONE depth map of image A from its k warps against k other images B_1 .. B_k (k <= 31) and their poses: every pixel of A is a
    track seen by A at its grid position and by each B_v at the warp's prediction, triangulated by triangulate_nview's kernel in one
    launch — views that disagree can be left out (max_view_error), and short baselines are backed by long ones.
    warps: a list or tuple of k warps of match(A, B_v), (H,2W,4) each — the left half rows are [grid_A, predicted x_Bv] —, or (H,W,4)
    each with symmetric=False, in normalised coordinates; or one (k,H,2W,4) tensor.  They are read in place: fp32 warps of one
    common layout whose last dimension is dense (stride 1), with even row and point strides and an 8-byte aligned address — what
    match() returns, a slice of match_tensors or of a stack of them; anything else is refused (make it .float().contiguous()).
    certainties: the k certainty maps, (H,2W) (or (H,W)) each, or one (k,...) tensor; masks: optional, the same shapes.  View v sees
    a pixel where certainty_v > certainty_thresh and mask_v is set.
    View 0 is A itself, observed at its grid (columns 0:2 of the first warp), always visible, with the identity pose and K_A at H_A x
    W_A.  Views 1 .. k are the B_v with R[v-1], t[v-1] such that x_Bv ~ K[v-1] (R[v-1] X_A + t[v-1]); R (k,3,3), t (k,3), K (3,3)
    shared or (k,3,3); sizes: k pairs (H_Bv, W_Bv), default (H_A, W_A) for all.
    THE k POSES MUST SHARE ONE SCALE.  k results of estimate_pose do not: each has a unit baseline of its own.  Take estimate_pose for
    B_1, triangulate its matches, and place B_2, ... against that cloud with find_absolute_pose: those poses do.
    max_view_error, iters, min_views (A counts), max_reproj_error, min_parallax_deg as triangulate_nview.
    Returns a MultiViewDepth: depth_A (H,W) = z in camera A, 0 where not valid, valid_A, num_views, reproj_error and points (H,W,3)
    in A's frame.  The B-side depth maps are not computed.  No host synchronisation."""
    gates = _nview_gates(max_view_error, iters, min_views, max_reproj_error, min_parallax_deg, 0)
    thresh = float(certainty_thresh)

    def listed(v, name):
        if torch.is_tensor(v):
            _need_gpu(v)
            return [v[i] for i in range(v.shape[0])]
        if not isinstance(v, (list, tuple)) or len(v) < 1:
            raise ValueError(f"{name}: expected a list or tuple of tensors, or one stacked tensor")
        _need_gpu(*v)
        return list(v)

    ws, cs = listed(warps, "warps"), listed(certainties, "certainties")
    ms = None if masks is None else listed(masks, "masks")
    k = len(ws)
    if not 1 <= k <= _MAX_VIEWS - 1:
        raise ValueError(f"{k} warps: 1 to {_MAX_VIEWS - 1} are supported")
    if len(cs) != k or (ms is not None and len(ms) != k):
        raise ValueError(f"{k} warps need {k} certainties (and masks), got {len(cs)}" + ("" if ms is None else f" and {len(ms)}"))
    w0 = ws[0]
    if w0.dim() != 3 or w0.shape[-1] != 4:
        raise ValueError(f"expected warps (H, W2, 4), got {tuple(w0.shape)}")
    H, W2 = w0.shape[0], w0.shape[1]
    if symmetric and W2 % 2:
        raise ValueError(f"a symmetric warp has an even width, got {W2}; pass symmetric=False for (H, W, 4) warps")
    W = W2 // 2 if symmetric else W2
    for i, w in enumerate(ws):
        if w.shape != w0.shape or w.dtype != torch.float32 or w.device != w0.device:
            raise ValueError(f"warp {i}: expected float32 {tuple(w0.shape)} on {w0.device}, got {w.dtype} {tuple(w.shape)} on {w.device}")
        if w.stride() != w0.stride() or w.stride(2) != 1 or w.stride(0) % 2 or w.stride(1) % 2 or w.stride(0) < 0 or w.stride(1) < 2 \
                or w.data_ptr() % 8:
            raise ValueError(f"warp {i}: strides {w.stride()} at address % 8 = {w.data_ptr() % 8} cannot be read in place (one common layout, "
                             "last dimension dense, even strides, 8-byte aligned); pass .contiguous() warps")
    for name, vs in (("certainty", cs), ("mask", ms)):
        for i, v in enumerate(vs or ()):
            if v.shape != (H, W2):
                raise ValueError(f"{name} {i} {tuple(v.shape)} does not match the warps {tuple(w0.shape)}")
    sizes = [(H_A, W_A)] * k if sizes is None else [tuple(s) for s in sizes]
    if len(sizes) != k:
        raise ValueError(f"sizes: expected {k} pairs (H_B, W_B), got {len(sizes)}")
    dev = w0.device
    Rk, tk = _poses(R, t, k, dev)
    Rp = torch.cat([torch.eye(3, dtype=torch.float64, device=dev)[None], Rk])
    tp = torch.cat([torch.zeros((1, 3), dtype=torch.float64, device=dev), tk])
    Kp = torch.cat([_intrinsics(K_A, 1, dev, "K_A"), _intrinsics(K, k, dev, "K")])
    keep = []
    for i in range(k):
        v = cs[i][:, :W] > thresh
        if ms is not None:
            v = v & (ms[i][:, :W] != 0)
        keep.append(v.to(torch.uint8).contiguous())
    obs = [w0.data_ptr()] + [w.data_ptr() + 8 for w in ws]
    vis = [None] + [v.data_ptr() for v in keep]
    to_px = [(W_A / 2, W_A / 2, H_A / 2, H_A / 2)] + [(wb / 2, wb / 2, hb / 2, hb / 2) for hb, wb in sizes]
    points, depth, reproj, _, views, valid = _triangulate_nview(obs, to_px, vis, W, Kp, Rp, tp, H, W, w0.stride(0), w0.stride(1), gates, dev,
                                                                (ws, keep))
    valid = valid.reshape(H, W)
    return MultiViewDepth(torch.where(valid, depth.reshape(H, W), 0.0), valid, _popcount(views).reshape(H, W), reproj.reshape(H, W),
                          points.reshape(H, W, 3))


# ------------------------------------------------------------------------------------- tracks from pairwise matches
_TRACKS_WORKSPACE_LIMIT = 2 << 30


class Tracks:
    """What build_tracks returns, device tensors: x (V,T,2) fp32 pixels, NaN where a view does not see a track; visible (V,T) bool;
    views (T) int32, bit v set where view v sees the track, (views >> v) & 1; num_views (T) uint8; track_of_match (M,k) int32, the row
    of the track a match belongs to or -1; counts (4) int32: qualifying components before truncation to T rows, conflicting
    components, components below min_views, and a status word that is 0.  Rows from min(counts[0], T) on are empty."""
    __slots__ = ("x", "visible", "views", "num_views", "track_of_match", "counts")

    def __init__(self, x, visible, views, num_views, track_of_match, counts):
        self.x, self.visible, self.views, self.num_views = x, visible, views, num_views
        self.track_of_match, self.counts = track_of_match, counts

    def __repr__(self):
        return f"Tracks(x={tuple(self.x.shape)}, track_of_match={tuple(self.track_of_match.shape)}, device={self.x.device})"


def build_tracks(matches, certainty, pairs, sizes, *, cell=4, certainty_thresh=0.0, mask=None, min_views=2, max_tracks):
    """Multi-view tracks from the pairwise matches of M image pairs over V views (2 <= V <= 32), on the device (csrc/tracks.hip) — the
    step between sample_batch and triangulate_nview.  A dense matcher has no repeatable keypoints, so every view is cut into cells of
    `cell` pixels (1 to 64): a cell that receives a match endpoint is a node, represented by its endpoint of the highest certainty (the
    first on a tie); a match is an edge between its two nodes; a connected component with at most one node per view and at least
    min_views views is a track.  A component with two nodes in one view is conflicting and gives none.
    matches: (M,k,4) normalised [xA, yA, xB, yB] as sample_batch returns them; certainty: (M,k); pairs: (M,2) integer tensor on the
    device, the views (a_m, b_m) of pair m; sizes: V pairs (H_v, W_v) of Python ints; mask: optional (M,k) bool / uint8, for instance
    the inlier masks of find_fundamental.  A match takes part when both endpoints lie inside their images, its certainty is finite
    and > certainty_thresh (>= 0), its mask is set, and its two views are different views in [0, V).
    Tracks are numbered by their lowest cell (view 0 first, row by row); max_tracks = T fixes the shape, rows beyond it are dropped
    and counts[0] still has the full number.  Returns a Tracks; x and visible go to triangulate_nview(tracks.x, R, t, K,
    visible=tracks.visible) as they are.  The result is a pure function of the inputs (integer atomics that commute, no float
    atomics); tests/tracks_ref.py restates it exactly.  No host synchronisation: the call can be captured in a hipGraph."""
    try:
        sizes = [(int(h), int(w)) for h, w in sizes]
    except (TypeError, ValueError):
        raise ValueError("sizes: expected V pairs (H_v, W_v) of ints") from None
    V = len(sizes)
    if not 2 <= V <= _MAX_VIEWS:
        raise ValueError(f"{V} views: 2 to {_MAX_VIEWS} are supported")
    if any(not (1 <= h <= 65536 and 1 <= w <= 65536) for h, w in sizes):
        raise ValueError(f"sizes: every (H_v, W_v) must be in [1, 65536], got {sizes}")
    cell, min_views, T, thresh = int(cell), int(min_views), int(max_tracks), float(certainty_thresh)
    if not 1 <= cell <= 64:
        raise ValueError(f"cell must be in [1, 64] pixels, got {cell}")
    if not 2 <= min_views <= V:
        raise ValueError(f"min_views must be in [2, V={V}], got {min_views}")
    if not (1 <= T and V * T < 1 << 30):
        raise ValueError(f"max_tracks must be at least 1 with V * max_tracks < 2^30, got {T}")
    if not 0.0 <= thresh < math.inf:
        raise ValueError(f"certainty_thresh must be finite and not negative, got {certainty_thresh}")
    lib = _lib.load()
    size_tab = (ctypes.c_int * (2 * V))(*[s for hw in sizes for s in hw])
    size_ptr = ctypes.cast(size_tab, ctypes.c_void_p)
    ws_bytes = lib.roma_tracks_workspace(V, size_ptr, cell, None)
    check(min(ws_bytes, 0), "roma_tracks_workspace")
    if ws_bytes > _TRACKS_WORKSPACE_LIMIT:
        raise ValueError(f"build_tracks: a workspace of {ws_bytes} bytes is above the limit of {_TRACKS_WORKSPACE_LIMIT}; use a larger cell "
                         f"than {cell}")
    if matches.dim() != 3 or matches.shape[-1] != 4 or not matches.is_floating_point():
        raise ValueError(f"expected floating-point matches (M,k,4), got {tuple(matches.shape)} {matches.dtype}")
    M, k = matches.shape[0], matches.shape[1]
    if M < 1 or k < 1 or M * k >= 1 << 31:
        raise ValueError(f"matches {tuple(matches.shape)}: M * k must be in [1, 2^31)")
    if certainty.shape != (M, k) or not certainty.is_floating_point():
        raise ValueError(f"certainty {tuple(certainty.shape)} {certainty.dtype} does not match the matches {tuple(matches.shape)}")
    if pairs.shape != (M, 2) or pairs.is_floating_point() or pairs.dtype == torch.bool:
        raise ValueError(f"pairs: expected an integer tensor ({M},2), got {tuple(pairs.shape)} {pairs.dtype}")
    if mask is not None and mask.shape != (M, k):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the matches {tuple(matches.shape)}")
    _need_gpu(matches, certainty, pairs, mask)
    dev = matches.device
    m = matches.to(torch.float32).contiguous()
    c = certainty.to(torch.float32).contiguous()
    pr = pairs.to(torch.int32).contiguous()
    mk = None if mask is None else mask.to(torch.uint8).contiguous()
    x = torch.empty((V, T, 2), dtype=torch.float32, device=dev)
    visible = torch.empty((V, T), dtype=torch.bool, device=dev)
    views = torch.empty((T,), dtype=torch.int32, device=dev)
    num_views = torch.empty((T,), dtype=torch.uint8, device=dev)
    track_of_match = torch.empty((M, k), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    check(lib.roma_build_tracks(m.data_ptr(), c.data_ptr(), None if mk is None else mk.data_ptr(), pr.data_ptr(), size_ptr, M, k, V, cell,
                                thresh, min_views, T, x.data_ptr(), visible.data_ptr(), views.data_ptr(), num_views.data_ptr(),
                                track_of_match.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
          "roma_build_tracks")
    return Tracks(x, visible, views, num_views, track_of_match, counts)


# ------------------------------------------------------------------------------------- ground-truth warp from depth, dense metrics
_DEPTH_MODES = {"bilinear": 0, "nearest": 1, "combined": 2}
_METRICS_PIXELS_PER_PARTIAL, _METRICS_PARTIAL_BYTES = 1024, 40


def dense_metrics_workspace(P, H, W):
    """Bytes of workspace roma_dense_match_metrics needs for P warps of H x W (include/roma_hip.h): one 40-byte partial per 1024
    pixels of a pair."""
    return P * (-(-(H * W) // _METRICS_PIXELS_PER_PARTIAL)) * _METRICS_PARTIAL_BYTES


class DenseMatchMetrics:
    """What dense_match_metrics returns, all device tensors.  Per pair (P,): epe_sum fp64 = the sum of the end-point error in pixels
    over the pixels with a ground truth, n_valid, n_pck_1, n_pck_3, n_pck_5 int64 = their number and how many lie within 1, 3, 5 px.
    Pooled over the batch (0-d fp64): epe, pck_1, pck_3, pck_5 = the sum of sums over the sum of counts (NaN when no pixel has a
    ground truth), computed when read.  counts (P,4) int64 holds the four n_ columns.  With return_maps: gd (P,H,W) fp64 of every
    pixel and prob (P,H,W) fp32, 1 where the ground truth is valid; else None."""
    __slots__ = ("epe_sum", "counts", "gd", "prob")

    def __init__(self, epe_sum, counts, gd, prob):
        self.epe_sum, self.counts, self.gd, self.prob = epe_sum, counts, gd, prob

    n_valid, n_pck_1, n_pck_3, n_pck_5 = (property(lambda self, k=k: self.counts[:, k]) for k in range(4))

    def _pooled(self, k):
        total = self.counts.sum(0).to(torch.float64)
        return total[k] / total[0]

    epe = property(lambda self: self.epe_sum.sum() / self.counts[:, 0].sum().to(torch.float64))
    pck_1, pck_3, pck_5 = (property(lambda self, k=k: self._pooled(k)) for k in (1, 2, 3))

    def __repr__(self):
        return f"DenseMatchMetrics(pairs={self.epe_sum.shape[0]}, device={self.epe_sum.device})"


def _depth_mode(mode, threshold):
    """-> (mode code, threshold), checked before anything looks at a tensor"""
    if mode not in _DEPTH_MODES:
        raise ValueError(f"unknown depth_interpolation_mode {mode!r}: 'bilinear', 'nearest' or 'combined'")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("relative_depth_error_threshold must not be NaN")
    return _DEPTH_MODES[mode], threshold


def _depth_pair(depth_A, depth_B, T, K_A, K_B):
    """-> contiguous depth_A (P,Ha,Wa), depth_B (P,Hb,Wb) fp32, T (P,3,4), K_A, K_B (P,3,3) fp64"""
    _need_gpu(depth_A, depth_B, T, K_A, K_B)
    if depth_A.dim() != 3 or depth_B.dim() != 3 or depth_A.shape[0] != depth_B.shape[0]:
        raise ValueError(f"expected depth maps (P,H_A,W_A) and (P,H_B,W_B), got {tuple(depth_A.shape)} and {tuple(depth_B.shape)}")
    P = depth_A.shape[0]
    if T.shape not in ((P, 3, 4), (P, 4, 4)):
        raise ValueError(f"expected a pose ({P},3,4) or ({P},4,4), got {tuple(T.shape)}")
    for name, K in (("K_A", K_A), ("K_B", K_B)):
        if K.shape != (P, 3, 3):
            raise ValueError(f"{name}: expected ({P},3,3) intrinsics, got {tuple(K.shape)}")
    return (depth_A.to(torch.float32).contiguous(), depth_B.to(torch.float32).contiguous(), T[:, :3, :4].to(torch.float64).contiguous(),
            K_A.to(torch.float64).contiguous(), K_B.to(torch.float64).contiguous())


def warp_kpts(kpts0, depth0, depth1, T_0to1, K0, K1, smooth_mask=False, return_relative_depth_error=False,
              depth_interpolation_mode="bilinear", relative_depth_error_threshold=0.05):
    """warp_kpts of the reference (romatch/utils/utils.py:358-455) on the device (csrc/depth_warp.hip): key-points of image 0 are
    lifted by depth0, moved by T_0to1 and projected into image 1; a point is valid where depth0 has a depth, the projection lies
    strictly inside image 1 and the depth of depth1 there agrees with the computed one to relative_depth_error_threshold.
    kpts0: (P,N,2) normalised to [-1,1], or the first two columns of a (P,N,4) warp (read in place); depth0 (P,H0,W0), depth1
    (P,H1,W1); T_0to1 (P,3,4) or (P,4,4); K0, K1 (P,3,3).  Key-points and depths are used as fp32 — what the reference's callers hold
    before their .double() — and everything per point is fp64 as there.  depth_interpolation_mode: "bilinear", "nearest", or
    "combined" (the nearest result where the bilinear one is not valid; the reference's own branch asks grid_sample for
    'nearest-exact', which torch refuses, so "nearest" is what it uses here).
    Returns (valid bool (P,N), x2 fp64 (P,N,2) normalised in image 1), or (relative depth error fp64 (P,N), x2) with
    return_relative_depth_error.  smooth_mask is not implemented.  No host synchronisation.
    Which key-points are read in place: fp32 ones that are contiguous, or whose strides are exactly (4 N, 4, 1) at an 8-byte aligned
    address (the [..., :2] view of a contiguous (P,N,4) warp).  Anything else — fp64 or fp16 key-points, other strides, and views whose
    size-1 dimensions carry a foreign stride — is first copied to contiguous fp32; the result is the same."""
    if smooth_mask is not False:
        raise NotImplementedError("warp_kpts: smooth_mask is not implemented on the device")
    code, threshold = _depth_mode(depth_interpolation_mode, relative_depth_error_threshold)
    _need_gpu(kpts0)
    if kpts0.dim() != 3 or kpts0.shape[-1] != 2 or not kpts0.is_floating_point():
        raise ValueError(f"expected floating-point key-points (P,N,2), got {tuple(kpts0.shape)} {kpts0.dtype}")
    da, db, T, Ka, Kb = _depth_pair(depth0, depth1, T_0to1, K0, K1)
    P, N = kpts0.shape[:2]
    if P != da.shape[0] or N < 1:
        raise ValueError(f"key-points {tuple(kpts0.shape)} do not match {da.shape[0]} depth maps")
    x = kpts0.to(torch.float32)
    stride = 4 if x.stride() == (4 * N, 4, 1) and x.data_ptr() % 8 == 0 else 2
    if stride == 2:
        x = x.contiguous()
    x2 = torch.empty((P, N, 2), dtype=torch.float64, device=x.device)
    valid = None if return_relative_depth_error else torch.empty((P, N), dtype=torch.uint8, device=x.device)
    rel = torch.empty((P, N), dtype=torch.float64, device=x.device) if return_relative_depth_error else None
    check(_lib.load().roma_warp_kpts(x.data_ptr(), stride, da.data_ptr(), db.data_ptr(), T.data_ptr(), Ka.data_ptr(), Kb.data_ptr(), P, N,
                                     da.shape[1], da.shape[2], db.shape[1], db.shape[2], code, threshold, x2.data_ptr(),
                                     None if valid is None else valid.data_ptr(), None if rel is None else rel.data_ptr(), _stream()),
          "roma_warp_kpts")
    return (rel if return_relative_depth_error else valid.bool()), x2


def gt_warp_grid(B, H, W, device):
    """The key-points get_gt_warp warps: the pixel centres of an H x W image, (B, H*W, 2) fp32 [x, y] — torch.linspace(-1 + 1/n,
    1 - 1/n, n) in fp32 on the device per axis, as the reference builds them."""
    gx = torch.linspace(-1 + 1 / W, 1 - 1 / W, W, device=device)
    gy = torch.linspace(-1 + 1 / H, 1 - 1 / H, H, device=device)
    return torch.stack((gx[None, :].expand(H, W), gy[:, None].expand(H, W)), dim=-1).reshape(1, H * W, 2).expand(B, H * W, 2).contiguous()


def get_gt_warp(depth1, depth2, T_1to2, K1, K2, depth_interpolation_mode="bilinear", relative_depth_error_threshold=0.05, H=None,
                W=None):
    """get_gt_warp of the reference (utils.py:326-355): warp_kpts on the pixel centres of an H x W grid (default: the size of depth1).
    Returns (x2 (B,H,W,2) fp64 normalised in image 2, prob (B,H,W) fp32: 1 where the warp is valid)."""
    _depth_mode(depth_interpolation_mode, relative_depth_error_threshold)
    _need_gpu(depth1)
    if depth1.dim() != 3:
        raise ValueError(f"expected a depth map (B,H,W), got {tuple(depth1.shape)}")
    B = depth1.shape[0]
    if H is None:
        H, W = depth1.shape[1:]
    mask, x2 = warp_kpts(gt_warp_grid(B, H, W, depth1.device), depth1, depth2, T_1to2, K1, K2,
                         depth_interpolation_mode=depth_interpolation_mode, relative_depth_error_threshold=relative_depth_error_threshold)
    return x2.reshape(B, H, W, 2), mask.float().reshape(B, H, W)


def dense_match_metrics(warp, depth_A, depth_B, T_AtoB, K_A, K_B, *, depth_interpolation_mode="bilinear",
                        relative_depth_error_threshold=0.05, return_maps=False):
    """End-point error and PCK@1/3/5 px of a dense warp against the ground truth of two depth maps and a pose, in one pass
    (csrc/depth_warp.hip): geometric_dist of the reference's MegadepthDenseBenchmark fused — the warp_kpts chain on columns 0-1 of every
    pixel, the distance in pixels (of the warp's own H x W) between that and columns 2-3, and per-pair sums.
    warp: (P,H,W,4) fp32 [x_A, y_A, predicted x_B, y_B] normalised; the left half warp[:, :, :W] of a symmetric (P,H,2W,4) result of
    match() is read in place.  depth_A, depth_B, T_AtoB, K_A, K_B and the two options as warp_kpts.
    Which warps are read in place: fp32 ones whose strides are exactly (H pitch, pitch, 4, 1) with pitch a multiple of 4 and >= 4 W, at
    a 16-byte aligned address — a contiguous warp, or the left half above.  Anything else (another dtype, other strides, a size-1
    dimension with a foreign stride) is first copied to contiguous fp32; the result is the same.
    Returns a DenseMatchMetrics; return_maps adds the per-pixel distance and validity.  No host synchronisation, no atomics: the
    result is bitwise reproducible and a pair's sums do not depend on the rest of the batch."""
    code, threshold = _depth_mode(depth_interpolation_mode, relative_depth_error_threshold)
    _need_gpu(warp)
    if warp.dim() != 4 or warp.shape[-1] != 4 or not warp.is_floating_point():
        raise ValueError(f"expected a floating-point warp (P,H,W,4), got {tuple(warp.shape)} {warp.dtype}")
    da, db, T, Ka, Kb = _depth_pair(depth_A, depth_B, T_AtoB, K_A, K_B)
    P, H, W = warp.shape[:3]
    if P != da.shape[0] or H < 1 or W < 1:
        raise ValueError(f"warp {tuple(warp.shape)} does not match {da.shape[0]} depth maps")
    w = warp.to(torch.float32)
    pitch = w.stride(1)
    if w.stride() != (H * pitch, pitch, 4, 1) or pitch < 4 * W or pitch % 4 or w.data_ptr() % 16:
        w = w.contiguous()
        pitch = 4 * W
    dev = w.device
    nbytes = dense_metrics_workspace(P, H, W)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    epe_sum = torch.empty(P, dtype=torch.float64, device=dev)
    counts = torch.empty((P, 4), dtype=torch.int64, device=dev)
    gd = torch.empty((P, H, W), dtype=torch.float64, device=dev) if return_maps else None
    valid = torch.empty((P, H, W), dtype=torch.uint8, device=dev) if return_maps else None
    check(_lib.load().roma_dense_match_metrics(w.data_ptr(), pitch, da.data_ptr(), db.data_ptr(), T.data_ptr(), Ka.data_ptr(), Kb.data_ptr(),
                                               P, H, W, da.shape[1], da.shape[2], db.shape[1], db.shape[2], code, threshold, ws.data_ptr(),
                                               nbytes, epe_sum.data_ptr(), counts.data_ptr(), None if gd is None else gd.data_ptr(),
                                               None if valid is None else valid.data_ptr(), _stream()), "roma_dense_match_metrics")
    return DenseMatchMetrics(epe_sum, counts, gd, None if valid is None else valid.float())


def geometric_dist(depth1, depth2, T_1to2, K1, K2, dense_matches):
    """MegadepthDenseBenchmark.geometric_dist of the reference (megadepth_dense_benchmark.py:17-42), its five-tuple: (gd[prob == 1]
    fp64, pck_1, pck_3, pck_5 fp32 scalars, prob (B,H,W) fp32).  Selecting gd[prob == 1] synchronises with the host, as it does in
    the reference; dense_match_metrics is the call without that."""
    m = dense_match_metrics(dense_matches, depth1, depth2, T_1to2, K1, K2, return_maps=True)
    n = m.n_valid.sum().to(torch.float32)
    return (m.gd[m.prob == 1], m.n_pck_1.sum().to(torch.float32) / n, m.n_pck_3.sum().to(torch.float32) / n,
            m.n_pck_5.sum().to(torch.float32) / n, m.prob)


# ------------------------------------------------------------------------------------------------------------ absolute pose
CameraPose = RelativePose                 # what estimate_absolute_pose returns: the same R / t / Rt holder, t in world units
_AP_RANSAC_OPT = {"max_reproj_error": 12.0, "max_iterations": 1000, "min_inliers": 3, "refine_iterations": 15}


def _points3d(X, x):
    """X (N,3) or (P,N,3), x (N,2) or (P,N,2), fp32/fp64 device tensors -> contiguous (P,N,3), (P,N,2) fp64, single-pair flag"""
    return _prepare(X, x, 3, 2, _ENTRIES[_KIND_AP].smin,
                    "expected world points (N,3) or (P,N,3) and pixels (N,2) or (P,N,2), got {0} and {1}", "points", "matches")


def absolute_pose_workspace_layout(P, N, iters):
    """(total bytes, [region offsets]) of the workspace of roma_absolute_pose_hypotheses (include/roma_hip.h: 12 regions)"""
    return workspace_layout(_KIND_AP, P, N, iters)


def find_absolute_pose(X, x, K, threshold=2.0, max_iters=1000, seed=None, lo_iters=3, refine_iters=0, *, scoring="msac"):
    """Camera pose (R, t) with x ~ K (R X + t) from 2D-3D matches, on the device (csrc/absolute_pose.hip): what places a further image
    against the points of `triangulate`, of `depth_from_warp` or of `lift_keypoints` — the call a host path makes to
    cv2.solvePnPRansac.  X: world points (N,3) or (P,N,3) in any frame, x: their pixels (N,2) or (P,N,2) in the image being placed,
    fp32/fp64; K: (3,3) shared or (P,3,3), tensor or numpy, upper triangular with last row 0 0 1.  RANSAC with max_iters P3P samples
    per pair, all drawn and scored (up to 4 poses each, fp64), the squared reprojection error in pixels scored in fp32 on world points
    normalised per pair, lowest cost wins, then lo_iters rounds of a damped Gauss-Newton step on the inliers.  A match is an inlier
    when its reprojection error is below threshold (pixels) and it lies in front of the camera.  Rows with a NaN / inf in X or x are
    never sampled and never inliers (triangulate's invalid rows can be passed as NaN).  Returns (R fp64 (3,3) or (P,3,3) orthonormal
    with det +1, t fp64 (3,) or (P,3) in world units, mask bool); R and t all zero and an empty mask when no sample gives a model.
    refine_iters > 0 polishes the RANSAC pose by refine_absolute_pose on all matches at the same threshold and returns the refined
    pose's mask; 0, the default, returns the RANSAC pose as it is.  scoring: "msac" or "magsac" (module docstring).
    At 30 % inliers (1 - 0.3^3)^1000 = 1e-12 of the calls draw no clean sample.  No host synchronisation."""
    score = _scoring(scoring)
    refine_iters = _refine_iters(refine_iters)
    _args(threshold, max_iters, lo_iters)
    Xw, xp, single = _points3d(X, x)
    P, N = Xw.shape[0], Xw.shape[1]
    Kp = _intrinsics(K, P, Xw.device, "K")
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=Xw.device)
    t = torch.empty((P, 3), dtype=torch.float64, device=Xw.device)
    mask = torch.empty((P, N), dtype=torch.uint8, device=Xw.device)
    _ransac(_KIND_AP, Xw, xp, (Kp,), (), threshold, int(max_iters), score, _seed(seed), lo_iters, (R, t, mask))
    if refine_iters > 0:
        (R, t, mask), _ = _refine_absolute(R, t, Xw, xp, Kp, threshold, refine_iters, None)
    else:
        mask = mask.bool()
    return (R[0], t[0], mask[0]) if single else (R, t, mask)


def _refine_absolute(R, t, Xw, xp, Kp, threshold, iters, m):
    """roma_refine_absolute_pose on prepared (P,...) tensors -> (R, t, mask bool), (cost, count, steps)"""
    return _run_refine("roma_refine_absolute_pose", (Xw, xp, Kp, R, t, m), Xw.shape[0], Xw.shape[1], (float(threshold), int(iters)),
                       (3, 3), (3,))


def refine_absolute_pose(R, t, X, x, K, threshold=2.0, iters=15, mask=None, return_info=False):
    """Non-linear refinement of an absolute pose (R, t) — of find_absolute_pose — on the 2D-3D matches it was estimated from:
    Levenberg-Marquardt, at most `iters` steps over 3 rotation and 3 translation parameters, on the sum over the matches of
    min(e, threshold^2), e the squared reprojection error in pixels (what find_absolute_pose scores with).  Matches beyond the
    threshold, behind the camera or not finite carry no weight, and `mask` (bool / uint8) optionally names the only matches that may
    carry any.  R (3,3) or (P,3,3), t (3,) or (P,3); X, x, K as find_absolute_pose (at least 4 matches).  Returns (R orthonormal fp64,
    t fp64, mask bool: e < threshold^2 and in front under the returned pose); with return_info also a dict of device tensors: cost
    (fp64, the truncated cost of the returned pose), count (int32, its inliers), steps (int32, the steps kept).  A step is kept only
    if it lowers the cost; a pair that cannot be refined (fewer than 4 weighted matches, a singular normal matrix, a pose that is not
    finite, no step that lowers the cost) gets its pose back bit for bit, with steps = 0."""
    _need_gpu(R, t)
    _refine_args(threshold, iters)
    Xw, xp, single = _points3d(X, x)
    P, N = Xw.shape[0], Xw.shape[1]
    if N < 4:
        raise ValueError(f"{N} matches, the refinement needs 4")
    if R.shape != ((3, 3) if single else (P, 3, 3)) or t.shape != ((3,) if single else (P, 3)):
        raise ValueError(f"R {tuple(R.shape)}, t {tuple(t.shape)} do not match the points {tuple(X.shape)}")
    Kp = _intrinsics(K, P, Xw.device, "K")
    r0 = R.reshape(P, 3, 3).to(torch.float64).contiguous()
    t0 = t.reshape(P, 3).to(torch.float64).contiguous()
    m = _mask(mask, P, N, x)
    res, info = _refine_absolute(r0, t0, Xw, xp, Kp, threshold, iters, m)
    return _refined(res, info, single, return_info)


def estimate_absolute_pose(points2D, points3D, camera, ransac_opt=None, *, seed=None, scoring="msac"):
    """Drop-in for poselib.estimate_absolute_pose on the device: find_absolute_pose -> refine_absolute_pose.  points2D (N,2) or
    (P,N,2) pixels, points3D (N,3) or (P,N,3) on the device; camera: a dict with model 'PINHOLE' and params [fx, fy, cx, cy] (one
    camera for the whole batch).  ransac_opt keys:
      max_reproj_error    pixels, default 12.0 (PoseLib's default)
      max_iterations      default 1000 samples; there is no early exit, every sample is drawn and scored, so this is the whole budget
      min_inliers         default 3: a pair whose RANSAC pose has fewer inliers keeps that pose unrefined
      refine_iterations   default 15 Levenberg-Marquardt steps
    Any other key, or another camera model, raises ValueError, and so do fewer than 3 matches (as estimate_relative_pose below its
    minimal sample).  Returns (pose, info): pose.R, pose.t,
    pose.Rt (CameraPose; x ~ K (R X + t)); info = {inliers: bool mask of the returned pose, num_inliers: int32, model_score: fp64
    truncated cost, refinements: int32 steps kept — device tensors, nothing is copied to the host —, iterations: max_iterations}."""
    _scoring(scoring)
    opt = dict(_AP_RANSAC_OPT)
    for k, v in (ransac_opt or {}).items():
        if k not in opt:
            raise ValueError(f"ransac_opt: unknown key {k!r}; known: {sorted(opt)}")
        opt[k] = v
    _, K = _focal(camera, "camera")
    if not float(opt["max_reproj_error"]) > 0:
        raise ValueError(f"ransac_opt: max_reproj_error must be positive, got {opt['max_reproj_error']}")
    if int(opt["max_iterations"]) < 1 or int(opt["min_inliers"]) < 0 or int(opt["refine_iterations"]) < 0:
        raise ValueError(f"ransac_opt: bad counts {opt}")
    thr = float(opt["max_reproj_error"])
    _points3d(points3D, points2D)                                    # shapes, counts and the device, before anything is allocated
    K = torch.tensor(K, dtype=torch.float64).to(points2D.device)
    R0, t0, mask0 = find_absolute_pose(points3D, points2D, K, thr, int(opt["max_iterations"]), seed, scoring=scoring)
    if points2D.shape[-2] < 4:                                       # the refinement needs 4 matches
        count = mask0.sum(-1).to(torch.int32)
        info = {"inliers": mask0, "num_inliers": count, "model_score": torch.full_like(count, float("nan"), dtype=torch.float64),
                "iterations": int(opt["max_iterations"]), "refinements": torch.zeros_like(count)}
        return CameraPose(R0, t0), info
    R, t, mask, refined = refine_absolute_pose(R0, t0, points3D, points2D, K, thr, int(opt["refine_iterations"]), return_info=True)
    cost, count, steps = refined["cost"], refined["count"], refined["steps"]
    keep = mask0.sum(-1) >= int(opt["min_inliers"])                  # on the device: no host synchronisation
    R = torch.where(keep[..., None, None], R, R0)
    t = torch.where(keep[..., None], t, t0)
    steps = torch.where(keep, steps, torch.zeros_like(steps))
    info = {"inliers": mask, "num_inliers": count, "model_score": cost, "iterations": int(opt["max_iterations"]), "refinements": steps}
    return CameraPose(R, t), info


def absolute_pose_error(R, t, T_gt):
    """Error of an absolute pose against T_gt (...,3,4) or (...,4,4) = [R_gt | t_gt] (tensor or numpy), in torch on the device, batched:
    (e_c, e_R) = the distance between the camera centres -R^T t in world units, and the geodesic angle of R^T R_gt in degrees."""
    _need_gpu(R, t)
    T_gt = torch.as_tensor(T_gt).to(device=R.device, dtype=R.dtype)
    R_gt, t_gt = T_gt[..., :3, :3], T_gt[..., :3, 3]
    centre = -(R.transpose(-1, -2) @ t.unsqueeze(-1)).squeeze(-1)
    centre_gt = -(R_gt.transpose(-1, -2) @ t_gt.unsqueeze(-1)).squeeze(-1)
    e_c = torch.linalg.norm(centre - centre_gt, dim=-1)
    cos = ((R * R_gt).sum((-1, -2)) - 1.0) / 2.0
    return e_c, torch.rad2deg(torch.acos(torch.clamp(cos, -1.0, 1.0)).abs())


def lift_keypoints(kpts, depth, K):
    """World points of pixel key-points from a depth map, in that camera's frame: X = depth(kpt) K^-1 (u, v, 1).  kpts (N,2) or (P,N,2)
    pixels (the centre of the top-left pixel is (0.5, 0.5), as to_pixel_coordinates), depth (H,W) or (P,H,W), K as find_absolute_pose.
    The depth is sampled nearest-neighbour.  Returns (...,N,3) fp64; a row is NaN where the depth is <= 0 or not finite or the
    key-point lies outside the map — rows the absolute-pose estimators skip by construction.  torch ops only; not a hot path."""
    _need_gpu(kpts, depth)
    if kpts.dim() not in (2, 3) or kpts.shape[-1] != 2 or depth.dim() != kpts.dim() or (kpts.dim() == 3 and depth.shape[0] != kpts.shape[0]):
        raise ValueError(f"expected key-points (N,2) with depth (H,W), or (P,N,2) with (P,H,W), got {tuple(kpts.shape)} and {tuple(depth.shape)}")
    single = kpts.dim() == 2
    kp = kpts.reshape((1,) + tuple(kpts.shape[-2:]) if single else kpts.shape).to(torch.float64)
    dm = depth.reshape((1,) + tuple(depth.shape[-2:]) if single else depth.shape).to(torch.float64)
    P, N, (H, W) = kp.shape[0], kp.shape[1], dm.shape[-2:]
    Ki = _inverse_intrinsics(_intrinsics(K, P, kp.device, "K"))
    col, row = torch.floor(kp[..., 0]), torch.floor(kp[..., 1])
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    idx = (row.clamp(0, H - 1) * W + col.clamp(0, W - 1)).to(torch.int64)
    d = torch.gather(dm.reshape(P, H * W), 1, torch.where(inside, idx, torch.zeros_like(idx)))
    ok = inside & torch.isfinite(d) & (d > 0)
    rays = torch.cat([kp, torch.ones_like(kp[..., :1])], -1) @ Ki.transpose(-1, -2)
    X = torch.where(ok[..., None], rays * d[..., None], torch.full_like(rays, float("nan")))
    return X[0] if single else X


def absolute_pose_hypotheses(X, x, K, threshold=2.0, max_iters=1000, seed=0, *, scoring="msac"):
    """Every hypothesis of one find_absolute_pose call, before selection (batched (P,...) shapes even for a single pair): samples
    (P,iters,3) int32 (a row of -1 for an invalid sample); R (P,iters,4,3,3), t (P,iters,4,3) fp64 in the WORLD frame (slots in the
    solver's order, zero where not valid); valid (P,iters,4) bool; cost (P,iters,4) fp64 of the chosen scoring (+inf if invalid);
    count (P,iters,4) int32 inliers; centroid (P,3), scale (P,) of the normalisation.  Pair p draws what it draws in
    find_absolute_pose with the same seed.  An inspection helper with score_hypotheses' batch limit."""
    score = _scoring(scoring)
    _args(threshold, max_iters, 0)
    Xw, xp, _ = _points3d(X, x)
    Kp = _intrinsics(K, Xw.shape[0], Xw.device, "K")
    h, view, _ = _inspect("absolute_pose_hypotheses", _KIND_AP, Xw, xp, lambda: (Kp,), (), threshold, max_iters, score, seed)
    norm, valid = view(0, torch.float64, (8,)), h["valid"]
    c, s = norm[:, :3].clone(), norm[:, 3].clone()
    R = view(3, torch.float64, valid.shape[1:] + (3, 3)).clone()
    tn = view(9, torch.float64, valid.shape[1:] + (3,))
    t = tn / s[:, None, None, None] - (R @ c[:, None, None, :, None]).squeeze(-1)
    return {"samples": h["samples"], "R": R, "t": torch.where(valid[..., None], t, torch.zeros_like(t)), "valid": valid,
            "cost": h["cost"], "count": h["count"], "centroid": c, "scale": s}


# ------------------------------------------------------------------------------------------------------ similarity registration
def _clouds(X, Y):
    """X, Y (N,3) or (P,N,3) fp32/fp64 device tensors of one shape -> contiguous (P,N,3) fp64 each, single-pair flag"""
    return _prepare(X, Y, 3, 3, _ENTRIES[_KIND_SIM].smin, "expected two clouds (N,3) or (P,N,3) of one shape, got {0} and {1}", "points",
                    "correspondences")


def similarity_workspace_layout(P, N, iters):
    """(total bytes, [region offsets]) of the workspace of roma_similarity_hypotheses (include/roma_hip.h: 12 regions)"""
    return workspace_layout(_KIND_SIM, P, N, iters)


def _refine_sim(s, R, t, Xw, Yw, threshold, iters, with_scale, m):
    """roma_refine_similarity on prepared (P,...) tensors -> (s, R, t, mask bool), (cost, count, steps)"""
    return _run_refine("roma_refine_similarity", (Xw, Yw, s, R, t, m), Xw.shape[0], Xw.shape[1],
                       (float(threshold), int(iters), int(bool(with_scale))), (), (3, 3), (3,))


def find_similarity(X, Y, threshold, max_iters=1000, seed=None, lo_iters=3, refine_iters=0, *, with_scale=True, scoring="msac"):
    """Similarity (s, R, t) with Y ~ s R X + t from putative 3D-3D correspondences with outliers, on the device (csrc/similarity.hip):
    what puts two reconstructions — each known only up to the scale of its own baseline — into one frame, or a reconstruction onto a
    ground-truth cloud.  X, Y: (N,3) or (P,N,3), fp32/fp64, row i of X corresponds to row i of Y.  RANSAC with max_iters samples of 3
    rows per pair, all drawn and scored (Umeyama's closed form in fp64, the rotation by Horn's quaternion), the squared distance scored
    in fp32 on clouds normalised per pair (so neither a far origin nor the ratio of the scales reaches fp32), lowest cost wins, then
    lo_iters rounds of the closed form on the inliers.  threshold is a DISTANCE IN THE UNITS OF Y: row i is an inlier when
    |Y_i - (s R X_i + t)| < threshold.  The noise of triangulated points grows with their depth (about quadratically, for a fixed
    pixel noise), so for clouds from `triangulate` / `depth_from_warp` choose it for the far points you want kept, or gate the clouds by
    parallax first.  with_scale=False estimates the rigid model (s = 1).  Rows with a NaN / inf in X or Y are never sampled and never
    inliers (triangulate's invalid rows can be passed as NaN).  Returns (s fp64 () or (P,), R fp64 (3,3) or (P,3,3) orthonormal with
    det +1, t fp64 (3,) or (P,3), mask bool); s, R and t all zero and an empty mask when no sample gives a model (collinear clouds,
    fewer than 3 usable rows).  refine_iters > 0 polishes the RANSAC model by refine_similarity on all rows at the same threshold and
    returns the refined model's mask.  scoring: "msac" or "magsac" (module docstring).  No host synchronisation."""
    score = _scoring(scoring)
    refine_iters = _refine_iters(refine_iters)
    _args(threshold, max_iters, lo_iters)
    Xw, Yw, single = _clouds(X, Y)
    P, N = Xw.shape[0], Xw.shape[1]
    dev = Xw.device
    s = torch.empty((P,), dtype=torch.float64, device=dev)
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((P, N), dtype=torch.uint8, device=dev)
    valid = torch.empty((P,), dtype=torch.int32, device=dev)
    _ransac(_KIND_SIM, Xw, Yw, (), (int(bool(with_scale)),), threshold, int(max_iters), score, _seed(seed), lo_iters,
            (s, R, t, mask, valid))
    if refine_iters > 0:
        (s, R, t, mask), _ = _refine_sim(s, R, t, Xw, Yw, threshold, refine_iters, with_scale, None)
    else:
        mask = mask.bool()
    return (s[0], R[0], t[0], mask[0]) if single else (s, R, t, mask)


def refine_similarity(s, R, t, X, Y, threshold, iters=15, mask=None, return_info=False, *, with_scale=True):
    """Refinement of a similarity (s, R, t) — of find_similarity — on the correspondences it was estimated from: at most `iters` rounds
    of the closed-form weighted least-squares fit (Umeyama) on the rows within the threshold of the current model, on the sum over the
    rows of min(e, threshold^2), e the squared distance |Y - (s R X + t)|^2 in Y units, in fp64.  Rows beyond the threshold or not
    finite carry no weight, and `mask` (bool / uint8) optionally names the only rows that may carry any.  s () or (P,), R (3,3) or
    (P,3,3), t (3,) or (P,3); X, Y as find_similarity.  Returns (s, R orthonormal, t, all fp64, mask bool: e < threshold^2 under the
    returned model); with return_info also a dict of device tensors: cost (fp64, the truncated cost of the returned model), count (int32,
    its inliers), steps (int32, the rounds kept).  A round is kept only if it lowers the cost, and the first that does not ends the
    loop; a pair that cannot be refined (fewer than 3 weighted rows, rows that do not fix the rotation, a model that is not finite, no
    round that lowers the cost) gets its model back bit for bit, with steps = 0.  with_scale=False keeps s = 1 in every round."""
    _need_gpu(s, R, t)
    _refine_args(threshold, iters)
    Xw, Yw, single = _clouds(X, Y)
    P, N = Xw.shape[0], Xw.shape[1]
    if s.shape != (() if single else (P,)) or R.shape != ((3, 3) if single else (P, 3, 3)) or t.shape != ((3,) if single else (P, 3)):
        raise ValueError(f"s {tuple(s.shape)}, R {tuple(R.shape)}, t {tuple(t.shape)} do not match the points {tuple(X.shape)}")
    s0 = s.reshape(P).to(torch.float64).contiguous()
    r0 = R.reshape(P, 3, 3).to(torch.float64).contiguous()
    t0 = t.reshape(P, 3).to(torch.float64).contiguous()
    m = _mask(mask, P, N, X)
    res, info = _refine_sim(s0, r0, t0, Xw, Yw, threshold, iters, with_scale, m)
    return _refined(res, info, single, return_info)


def similarity_hypotheses(X, Y, threshold, max_iters=1000, seed=0, *, with_scale=True, scoring="msac"):
    """Every hypothesis of one find_similarity call, before selection (batched (P,...) shapes even for a single pair): samples
    (P,iters,3) int32 (a row of -1 for an invalid sample); s (P,iters), R (P,iters,3,3), t (P,iters,3) fp64 in the CALLER'S units (zero
    where not valid); valid (P,iters) bool; cost (P,iters) fp64 of the chosen scoring in squared NORMALISED Y units, i.e. times
    scale_Y^2 (+inf if invalid); count (P,iters) int32 inliers; centroid_X, centroid_Y (P,3), scale_X, scale_Y (P,) of the
    normalisation.  Pair p draws what it draws in find_similarity with the same seed.  An inspection helper with score_hypotheses' batch
    limit."""
    score = _scoring(scoring)
    _args(threshold, max_iters, 0)
    Xw, Yw, _ = _clouds(X, Y)
    h, view, _ = _inspect("similarity_hypotheses", _KIND_SIM, Xw, Yw, lambda: (), (int(bool(with_scale)),), threshold, max_iters, score, seed)
    norm, iters = view(0, torch.float64, (8,)), int(max_iters)
    cX, sX, cY, sY = norm[:, :3].clone(), norm[:, 3].clone(), norm[:, 4:7].clone(), norm[:, 7].clone()
    R = view(3, torch.float64, (iters, 3, 3)).clone()
    ts = view(9, torch.float64, (iters, 4))
    valid = h["valid"][..., 0]                                       # one slot per sample: no slot axis in what is returned
    s = ts[..., 3] * (sX / sY)[:, None]
    t = ts[..., :3] / sY[:, None, None] + cY[:, None, :] - s[..., None] * (R @ cX[:, None, :, None]).squeeze(-1)
    return {
        "samples": h["samples"],
        "s": torch.where(valid, s, torch.zeros_like(s)),
        "R": R,
        "t": torch.where(valid[..., None], t, torch.zeros_like(t)),
        "valid": valid,
        "cost": h["cost"][..., 0],
        "count": h["count"][..., 0],
        "centroid_X": cX, "scale_X": sX, "centroid_Y": cY, "scale_Y": sY,
    }


def apply_similarity(X, s, R, t):
    """s R X + t for points X (...,N,3) and a similarity s (...), R (...,3,3), t (...,3) of find_similarity: torch ops only, CPU or
    device tensors."""
    s, R, t = (torch.as_tensor(v, dtype=X.dtype, device=X.device) for v in (s, R, t))
    return s[..., None, None] * (X @ R.transpose(-1, -2)) + t[..., None, :]


def transform_cameras(R_cam, t_cam, s, R, t):
    """Cameras x ~ K (R_cam X + t_cam) of the source frame, expressed in the destination frame Y = s R X + t of a similarity (of
    find_similarity): R' = R_cam R^T, t' = s t_cam - R' t, so that K (R' Y + t') ~ K (R_cam X + t_cam) — the same pixels.  R_cam
    (...,3,3), t_cam (...,3); s (), R (3,3), t (3,) or batched alike.  torch ops only, CPU or device tensors."""
    s, R, t = (torch.as_tensor(v, dtype=R_cam.dtype, device=R_cam.device) for v in (s, R, t))
    Rn = R_cam @ R.transpose(-1, -2)
    return Rn, s[..., None] * t_cam - (Rn @ t[..., None]).squeeze(-1)


def similarity_error(s, R, t, s_gt, R_gt, t_gt, at):
    """Error of a similarity against (s_gt, R_gt, t_gt): (the geodesic angle of R^T R_gt in degrees, |log(s / s_gt)|, the distance
    between the two images of the points `at` (...,N,3) divided by s_gt — in the units of the source cloud), batched, torch ops only,
    CPU or device tensors."""
    s_gt, R_gt, t_gt = (torch.as_tensor(v, dtype=R.dtype, device=R.device) for v in (s_gt, R_gt, t_gt))
    cos = ((R * R_gt).sum((-1, -2)) - 1.0) / 2.0
    e_R = torch.rad2deg(torch.acos(torch.clamp(cos, -1.0, 1.0)).abs())
    e_s = torch.log(s / s_gt).abs()
    d = torch.linalg.norm(apply_similarity(at, s, R, t) - apply_similarity(at, s_gt, R_gt, t_gt), dim=-1) / s_gt[..., None]
    return e_R, e_s, d


def register_depth_maps(depth_src, depth_dst, K, threshold, **kw):
    """Similarity between two depth maps (H,W) of the SAME image, each in its own unit — e.g. of depth_from_warp against two partners:
    the pixel grid (centres at +0.5, as lift_keypoints) is lifted with each map, X = depth_src K^-1 (u, v, 1) and Y likewise, cells where
    either depth is <= 0 or not finite become NaN rows, and find_similarity(X, Y, threshold, **kw) registers them.  Returns (s, R, t,
    mask (H,W)); s is the ratio of the units (R ~ I, t ~ 0 for maps of one image) — what gives the poses passed to depth_from_warps
    their shared scale.  threshold in the units of depth_dst."""
    _need_gpu(depth_src, depth_dst)
    if depth_src.dim() != 2 or depth_src.shape != depth_dst.shape:
        raise ValueError(f"expected two depth maps (H,W) of one shape, got {tuple(depth_src.shape)} and {tuple(depth_dst.shape)}")
    H, W = depth_src.shape
    dev = depth_src.device
    Ki = _inverse_intrinsics(_intrinsics(K, 1, dev, "K"))[0]
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev) + 0.5, torch.arange(W, dtype=torch.float64, device=dev) + 0.5,
                          indexing="ij")
    rays = (torch.stack([u, v, torch.ones_like(u)], -1) @ Ki.transpose(-1, -2)).reshape(H * W, 3)
    ds, dd = depth_src.reshape(-1).to(torch.float64), depth_dst.reshape(-1).to(torch.float64)
    ok = torch.isfinite(ds) & torch.isfinite(dd) & (ds > 0) & (dd > 0)
    nan = torch.full_like(rays, float("nan"))
    X = torch.where(ok[:, None], rays * ds[:, None], nan)
    Y = torch.where(ok[:, None], rays * dd[:, None], nan)
    s, R, t, mask = find_similarity(X, Y, threshold, **kw)
    return s, R, t, mask.reshape(H, W)


# ------------------------------------------------------------------------------------------------------------ bundle adjustment
_BUNDLE_REGIONS = 11


class BundleResult:
    """What bundle_adjust returns, device tensors: R (V,3,3), t (V,3), points (N,3) fp64; mask (V,N) bool, the observations inside the
    threshold (with positive depth) under the returned state; cost and cost0, fp64 scalars, the truncated cost of the result and of the
    input (cost <= cost0); steps int32, the Levenberg-Marquardt steps kept (0: R, t, points are the input bit for bit); count int32,
    the number of set mask entries; status int32 (include/roma_hip.h: 0, or why the input came back)."""
    __slots__ = ("R", "t", "points", "mask", "cost", "cost0", "steps", "count", "status")

    def __init__(self, R, t, points, mask, cost, cost0, steps, count, status=None):
        self.R, self.t, self.points, self.mask, self.cost, self.cost0 = R, t, points, mask, cost, cost0
        self.steps, self.count, self.status = steps, count, status

    def __repr__(self):
        return f"BundleResult(R={tuple(self.R.shape)}, points={tuple(self.points.shape)}, device={self.R.device})"


def bundle_workspace_layout(V, N):
    """-> (bytes, offsets of the 11 regions) of roma_bundle_workspace; raises ValueError on a bad shape"""
    return _workspace_layout("roma_bundle_workspace", _BUNDLE_REGIONS, int(V), int(N))


def _fixed_mask(fixed, V):
    """a sequence of view indices or a (V,) bool tensor -> the 32-bit pattern of the held views"""
    if torch.is_tensor(fixed) and fixed.dtype == torch.bool:
        if fixed.shape != (V,):
            raise ValueError(f"fixed: expected a ({V},) bool tensor, got {tuple(fixed.shape)}")
        idx = [v for v, f in enumerate(fixed.tolist()) if f]
    else:
        idx = [int(v) for v in (fixed.tolist() if torch.is_tensor(fixed) else fixed)]
    if any(not 0 <= v < V for v in idx):
        raise ValueError(f"fixed: view indices must be in [0, {V}), got {idx}")
    if not idx:
        raise ValueError("fixed: at least one view must be held (the gauge)")
    if len(set(idx)) == V:
        raise ValueError("fixed: every view is held, nothing to refine")
    bits = 0
    for v in idx:
        bits |= 1 << v
    return bits


def bundle_adjust(x, R, t, K, X, *, visible=None, threshold=2.0, iters=10, fixed=(0,), return_info=False):
    """Cameras and points of one reconstruction refined TOGETHER (csrc/bundle.hip): Levenberg-Marquardt on the truncated reprojection
    cost sum min(e, threshold^2) over the observations, the cameras solved through the Schur complement of the points — the step after
    build_tracks -> estimate_pose / find_absolute_pose -> triangulate_nview, which each fit one kind while holding the other.
    Convention of triangulate_nview: x_v ~ K_v (R_v X + t_v), 2 <= V <= 32 views, one reconstruction per call.
    x: (V,N,2) pixels, any float dtype on the device, NaN where a view does not see a point, and visible (V,N) bool / uint8, optional —
    `Tracks.x` and `Tracks.visible` of build_tracks as they come; R (V,3,3), t (V,3); K (3,3) shared or (V,3,3); X: (N,3) points, fp32
    (`MultiViewTriangulation.points`) or fp64.  threshold in pixels; iters 0 to 50; fixed: the views that are held, a sequence of
    indices or a (V,) bool tensor (a tensor on the device is read back: keep it on the host under graph capture).
    This is a POLISH, as the other refine_* functions are: an observation more than `threshold` pixels off under the start counts as
    an outlier, so the start has to reproject within a few pixels — a camera left with too few inliers does not move, and when no step
    lowers the cost the input comes back bit for bit with steps = 0.  The gauge: with ONE fixed view the scale of the reconstruction is
    left to the damping (it stays near the input's), TWO fixed views determine it.
    A free view without an inlier and a point with fewer than two are held for that step; views and points held throughout come back
    bit for bit.  Returns a BundleResult (R, t, points fp64, mask, cost, cost0, steps, count); with return_info=True also a dict with the
    status word.  fp64 relative to the mean camera centre: the result does not depend on where the world's origin is.  Sums are taken
    in a fixed order (no floating-point atomics): bitwise reproducible.  The decision to keep a step is taken on the device: no host
    synchronisation, the call can be captured in a hipGraph."""
    thr, iters = _threshold_px(threshold), int(iters)
    if not 0 <= iters <= 50:
        raise ValueError(f"iters must be in [0, 50], got {iters}")
    _need_gpu(x, visible, X)
    xs, vis, V, N, obs_tab, vis_tab = _observations(x, visible, 2)
    if X.shape != (N, 3) or not X.is_floating_point():
        raise ValueError(f"points {tuple(X.shape)} {X.dtype}: expected floating-point ({N},3)")
    bits = _fixed_mask(fixed, V)
    dev = x.device
    Rp, tp = _poses(R, t, V, dev)
    Kp = _intrinsics(K, V, dev, "K")
    Xp = X.to(torch.float64).contiguous()
    need, _ = bundle_workspace_layout(V, N)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    Ro, to, Xo, cost = torch.empty((V, 3, 3), **f64), torch.empty((V, 3), **f64), torch.empty((N, 3), **f64), torch.empty((2,), **f64)
    mask = torch.empty((V, N), dtype=torch.uint8, device=dev)
    ints = torch.empty((3,), dtype=torch.int32, device=dev)                       # count, steps, status
    check(_lib.load().roma_bundle_adjust(ctypes.cast(obs_tab, ctypes.c_void_p), None, None if vis_tab is None else ctypes.cast(vis_tab, ctypes.c_void_p),
                                         2, Kp.data_ptr(), Rp.data_ptr(), tp.data_ptr(), Xp.data_ptr(), V, N, bits, thr, iters, Ro.data_ptr(),
                                         to.data_ptr(), Xo.data_ptr(), mask.data_ptr(), cost.data_ptr(), ints.data_ptr(), ints.data_ptr() + 4,
                                         ints.data_ptr() + 8, ws.data_ptr(), need, _stream()),
          "roma_bundle_adjust")
    res = BundleResult(Ro, to, Xo, mask.bool(), cost[1], cost[0], ints[1], ints[0], ints[2])
    return (res, {"status": ints[2]}) if return_info else res


# ------------------------------------------------------------------------------------------------------------ motion averaging
_POSITIONS_REGIONS = 11
_MAX_EDGES = 4096


class RotationAverage:
    """What average_rotations returns, device tensors: R (V,3,3) fp64, NaN for a view the pose graph does not reach from the root; valid
    (V) bool; residual_deg (M) fp64, the angle left on every edge under R (NaN for an edge that is not usable or not reached: an
    outlier pair stands out by tens of degrees); status int32 (0, or 1: a pivot failed and R is the spanning-tree start)."""
    __slots__ = ("R", "valid", "residual_deg", "status")

    def __init__(self, R, valid, residual_deg, status):
        self.R, self.valid, self.residual_deg, self.status = R, valid, residual_deg, status

    def __repr__(self):
        return f"RotationAverage(R={tuple(self.R.shape)}, edges={tuple(self.residual_deg.shape)}, device={self.R.device})"


class GlobalPositions:
    """What global_positions returns, device tensors: t (V,3) and centres (V,3) fp64, NaN for a view that is not placed; points (N,3) fp64,
    NaN where a track is not solved; mask (V,N) bool, the observations that agree with the result; count int32, the set mask entries;
    eigenvalues (2) fp64, the two smallest of the reduced matrix (their ratio says how well the centres are determined); status int32
    (include/roma_hip.h: bit 0 and bit 2 mean no result, bit 1 that a view was not placed)."""
    __slots__ = ("t", "centres", "points", "mask", "count", "eigenvalues", "status")

    def __init__(self, t, centres, points, mask, count, eigenvalues, status):
        self.t, self.centres, self.points, self.mask, self.count, self.eigenvalues, self.status = t, centres, points, mask, count, eigenvalues, status

    def __repr__(self):
        return f"GlobalPositions(t={tuple(self.t.shape)}, points={tuple(self.points.shape)}, device={self.t.device})"


class CameraStart:
    """What initialize_cameras returns: R (V,3,3), t (V,3), points (N,3) fp64, mask (V,N) bool, valid (V) bool, and the two status words
    rotation_status, position_status (int32) — ready for bundle_adjust(x, R, t, K, points, visible=mask, threshold=8.0)."""
    __slots__ = ("R", "t", "points", "mask", "valid", "rotation_status", "position_status")

    def __init__(self, R, t, points, mask, valid, rotation_status, position_status):
        self.R, self.t, self.points, self.mask, self.valid = R, t, points, mask, valid
        self.rotation_status, self.position_status = rotation_status, position_status

    def __repr__(self):
        return f"CameraStart(R={tuple(self.R.shape)}, points={tuple(self.points.shape)}, device={self.R.device})"


def _edges(pairs, M, device):
    """(M,2) view indices, tensor or numpy -> contiguous int32 on the device"""
    if not torch.is_tensor(pairs):
        pairs = torch.as_tensor(pairs, dtype=torch.int32).to(device)
    _need_gpu(pairs)
    if pairs.shape != (M, 2) or pairs.is_floating_point():
        raise ValueError(f"pairs {tuple(pairs.shape)} {pairs.dtype}: expected integer ({M},2)")
    return pairs.to(torch.int32).contiguous()


def _view_index(root, V):
    root = int(root)
    if not 0 <= root < V:
        raise ValueError(f"root must be one of the {V} views, got {root}")
    return root


def average_rotations(R_rel, pairs, V, *, weights=None, root=0, sigma_deg=5.0, iters=12):
    """Global rotations of V views (2 to 32) from the M pairwise rotations of a pose graph (csrc/motion_average.hip, one launch of one
    workgroup): the maximum-weight spanning tree from `root` as the start, then `iters` rounds (0 to 50) of re-weighted least squares on
    the Lie algebra — the first half with L1 weights, which gets out of a tree that contains an outlier edge, the second half with
    Geman-McClure weights at sigma_deg — each a weighted graph Laplacian solved by Cholesky.
    R_rel: (M,3,3), pairs: (M,2) with pairs[m] = (a, b) and X_b = R_rel[m] X_a + t (estimate_pose's convention), 1 <= M <= 4096; weights:
    (M) or None (all 1), e.g. the inlier count of the pair's RANSAC.  Returns a RotationAverage; R[root] = I, and R follows
    triangulate_nview / bundle_adjust: x_v ~ K_v (R_v X + t_v).  No host synchronisation: the call can be captured in a graph."""
    V, iters, sigma = int(V), int(iters), float(sigma_deg)
    if not 2 <= V <= _MAX_VIEWS:
        raise ValueError(f"{V} views: 2 to {_MAX_VIEWS} are supported")
    root = _view_index(root, V)
    if not 0 <= iters <= 50:
        raise ValueError(f"iters must be in [0, 50], got {iters}")
    if not 0.0 < sigma < 1e18:
        raise ValueError(f"sigma_deg must be positive, got {sigma_deg}")
    _need_gpu(R_rel, weights)
    if R_rel.dim() != 3 or R_rel.shape[1:] != (3, 3) or not R_rel.is_floating_point():
        raise ValueError(f"R_rel {tuple(R_rel.shape)} {R_rel.dtype}: expected floating-point (M,3,3)")
    M = R_rel.shape[0]
    if not 1 <= M <= _MAX_EDGES:
        raise ValueError(f"{M} edges: 1 to {_MAX_EDGES} are supported")
    dev = R_rel.device
    pr = _edges(pairs, M, dev)
    if weights is not None and weights.shape != (M,):
        raise ValueError(f"weights {tuple(weights.shape)}: expected ({M},)")
    Rr = R_rel.to(torch.float64).contiguous()
    wt = None if weights is None else weights.to(torch.float64).contiguous()
    R = torch.empty((V, 3, 3), dtype=torch.float64, device=dev)
    valid = torch.empty((V,), dtype=torch.uint8, device=dev)
    res = torch.empty((M,), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    check(_lib.load().roma_rotation_average(Rr.data_ptr(), pr.data_ptr(), None if wt is None else wt.data_ptr(), V, M, root, sigma, iters,
                                            R.data_ptr(), valid.data_ptr(), res.data_ptr(), status.data_ptr(), _stream()),
          "roma_rotation_average")
    return RotationAverage(R, valid.bool(), torch.rad2deg(res), status[0])


def positions_workspace_layout(V, N, M):
    """-> (bytes, offsets of the 11 regions) of roma_positions_workspace; raises ValueError on a bad shape"""
    return _workspace_layout("roma_positions_workspace", _POSITIONS_REGIONS, int(V), int(N), int(M))


def global_positions(x, R, K, pairs, t_rel, *, visible=None, threshold=4.0, rounds=4, root=0):
    """Camera centres and points of one reconstruction under KNOWN rotations (csrc/motion_average.hip): with R from average_rotations the
    problem is linear — every observation asks its point to lie on the ray from its camera —, the points are eliminated one by one and
    the centres are the smallest eigenvector of the reduced 3 V x 3 V matrix (the Schur pattern of bundle_adjust), re-weighted over
    `rounds` rounds (2 to 8).  The first weights are a majority vote of the pairwise translation directions: an observation counts when
    at least half of the edges that join its view to another view of its track agree with it.
    x: (V,N,2) pixels and visible (V,N), read exactly as bundle_adjust reads them (`Tracks.x`, `Tracks.visible` as they come), 3 <= V <=
    32; R: (V,3,3), NaN for a view that has none; K: (3,3) or (V,3,3); pairs (M,2) and t_rel (M,3): the edges, of which only the
    direction of t_rel is used (X_b = R_rel X_a + t_rel); threshold in pixels; root: the view at the origin.  The scale is fixed by
    sum |C_v|^2 = 1.  Returns a GlobalPositions.  Sums in a fixed order, no floating-point atomics: bitwise reproducible; no host
    synchronisation: the call can be captured in a graph."""
    thr, rounds = _threshold_px(threshold), int(rounds)
    if not 2 <= rounds <= 8:
        raise ValueError(f"rounds must be in [2, 8], got {rounds}")
    _need_gpu(x, visible)
    xs, vis, V, N, obs_tab, vis_tab = _observations(x, visible, 3)
    root = _view_index(root, V)
    dev = x.device
    if not torch.is_tensor(t_rel):
        t_rel = torch.as_tensor(t_rel, dtype=torch.float64).to(dev)
    _need_gpu(t_rel)
    if t_rel.dim() != 2 or t_rel.shape[1] != 3:
        raise ValueError(f"t_rel {tuple(t_rel.shape)}: expected (M,3)")
    M = t_rel.shape[0]
    if not 1 <= M <= _MAX_EDGES:
        raise ValueError(f"{M} edges: 1 to {_MAX_EDGES} are supported")
    pr = _edges(pairs, M, dev)
    tr = t_rel.to(torch.float64).contiguous()
    Rp, _ = _poses(R, torch.zeros((V, 3), dtype=torch.float64, device=dev), V, dev)
    Kp = _intrinsics(K, V, dev, "K")
    need, _ = positions_workspace_layout(V, N, M)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    t, centres, points, lam = torch.empty((V, 3), **f64), torch.empty((V, 3), **f64), torch.empty((N, 3), **f64), torch.empty((2,), **f64)
    mask = torch.empty((V, N), dtype=torch.uint8, device=dev)
    ints = torch.empty((2,), dtype=torch.int32, device=dev)                       # count, status
    check(_lib.load().roma_global_positions(ctypes.cast(obs_tab, ctypes.c_void_p), None, None if vis_tab is None else ctypes.cast(vis_tab, ctypes.c_void_p),
                                            2, Kp.data_ptr(), Rp.data_ptr(), pr.data_ptr(), tr.data_ptr(), V, N, M, root, thr, rounds, t.data_ptr(),
                                            centres.data_ptr(), points.data_ptr(), mask.data_ptr(), ints.data_ptr(), lam.data_ptr(),
                                            ints.data_ptr() + 4, ws.data_ptr(), need, _stream()),
          "roma_global_positions")
    return GlobalPositions(t, centres, points, mask.bool(), ints[0], lam, ints[1])


def initialize_cameras(x, K, pairs, R_rel, t_rel, *, visible=None, weights=None, threshold=4.0, root=0):
    """The V cameras and the points of a reconstruction from its tracks and the pairwise poses of its image pairs — average_rotations,
    then global_positions under those rotations: the start that bundle_adjust asks for.  x, visible: `Tracks.x`, `Tracks.visible`; K:
    (3,3) or (V,3,3); pairs (M,2), R_rel (M,3,3), t_rel (M,3): what estimate_pose returned for pairs[m] = (a, b); weights: (M), e.g.
    the pairs' inlier counts.  Returns a CameraStart: R, t, points, mask, valid and both status words.  The frame is that of `root`
    (R = I, t = 0) and the scale that of sum |C_v|^2 = 1."""
    if x.dim() != 3:
        raise ValueError(f"expected observations (V,N,2), got {tuple(x.shape)}")
    rot = average_rotations(R_rel, pairs, x.shape[0], weights=weights, root=root)
    pos = global_positions(x, rot.R, K, pairs, t_rel, visible=visible, threshold=threshold, root=root)
    return CameraStart(rot.R, pos.t, pos.points, pos.mask, rot.valid, rot.status, pos.status)


# ------------------------------------------------------------------------------------------------------------ depth-map fusion
class FusedDepth:
    """What fuse_depth_maps returns, device tensors.  Per view and pixel — lists of (H_v, W_v) tensors when the maps came as a list, (V,H,W)
    tensors when they came stacked: depth fp32, the mean of the pixel's own depth and the depths the consistent views give it, 0 where
    not valid; valid bool; views int32, the bit pattern of the pixel's own view and the consistent ones, (views >> v) & 1; num_views
    uint8.  The cloud, T = max_points rows: points (T,3) fp32 in the frame of the poses; view (T) uint8 and pixel (T) int32 = row * W_v +
    column, where a point comes from; point_views (T) int32; rows from min(counts[0], T) on are 0 with pixel = -1.  counts (4) int32:
    pixels emitted before truncation to T rows, valid pixels, duplicates, and a status word that is 0."""
    __slots__ = ("depth", "valid", "views", "num_views", "points", "view", "pixel", "point_views", "counts")

    def __init__(self, depth, valid, views, num_views, points, view, pixel, point_views, counts):
        self.depth, self.valid, self.views, self.num_views = depth, valid, views, num_views
        self.points, self.view, self.pixel, self.point_views, self.counts = points, view, pixel, point_views, counts

    def __repr__(self):
        return f"FusedDepth(views={len(self.depth)}, points={tuple(self.points.shape)}, device={self.points.device})"


def depth_fuse_workspace(V, total_pixels):
    """-> bytes of roma_depth_fuse_workspace; raises ValueError on a bad shape"""
    need = _lib.load().roma_depth_fuse_workspace(int(V), int(total_pixels), None)
    if need < 0:
        check(int(need), "roma_depth_fuse_workspace")
    return int(need)


def fuse_depth_maps(depths, R, t, K, *, sizes=None, max_reproj_error=1.0, max_depth_error=0.01, min_views=2, max_points):
    """The depth maps of V posed views (2 <= V <= 32) checked against one another and merged into ONE cloud (csrc/depth_fuse.hip) — the
    geometric consistency filter and fusion that multi-view stereo runs after its depth maps, and the step after depth_from_warps,
    which gives every image a map of its own.  Convention of find_absolute_pose / triangulate_nview: x_v ~ K_v (R_v X + t_v); pixel (row
    i, column j) of a map is at (j + 0.5, i + 0.5), as in lift_keypoints.
    depths: a list or tuple of V maps (H_v, W_v), shapes free per view, or one (V,H,W) tensor: contiguous fp32 on the device, read in
    place; anything else is refused (make it .float().contiguous()).  A depth that is 0, negative or not finite is a hole.  R (V,3,3), t
    (V,3); K (3,3) shared or (V,3,3); sizes: V pairs (H_img, W_img), the image size K_v refers to, default the map's own shape — K_v is
    scaled by diag(W_v / W_img, H_v / H_img, 1), so a depth_from_warps map at match resolution goes in with the K_A that made it.  A
    view whose K is singular or not upper triangular, or whose pose is not finite, sees nothing and is seen by nothing.
    Consistency: a pixel of view r with depth d is lifted and projected into every other usable view s (ascending; in front of s only);
    the depth of s is sampled bilinearly there, only where all four taps are inside the map and none is a hole; that sample is lifted
    from s and projected back into r; s is consistent when it comes back in front of r within max_reproj_error pixels (of map r) of
    where it started and its depth p.z has |p.z - d| / d < max_depth_error.  views = the pixel's own bit and the consistent views',
    valid = num_views >= min_views (2 <= min_views <= V), depth = the mean of d and the consistent p.z.
    Ownership: a valid pixel is a duplicate when a consistent view s < r has, at the pixel the projection falls into, a valid pixel that
    counts r as consistent.  Pixels of the lowest view are never duplicates and every duplicate points to a lower view, so every surface
    point is emitted at least once.
    Cloud: the valid pixels that are not duplicates, in the order (view, row, column); max_points = T fixes the shape, rows beyond it are
    dropped and counts[0] still has the full number.  Returns a FusedDepth.  fp64 per pixel from the fp32 depths, on pair constants in
    which the world's origin has cancelled; no atomics, so two calls agree bit for bit; tests/fuse_depth_ref.py restates it exactly.  No
    host synchronisation: the call can be captured in a hipGraph."""
    reproj, rel, min_views = float(max_reproj_error), float(max_depth_error), int(min_views)
    if not 0.0 < reproj < math.inf:
        raise ValueError(f"max_reproj_error must be positive finite pixels, got {max_reproj_error}")
    if not 0.0 < rel < math.inf:
        raise ValueError(f"max_depth_error must be positive and finite, got {max_depth_error}")
    try:
        T = int(max_points)
    except (TypeError, ValueError):
        raise ValueError(f"max_points: expected an int, got {max_points!r}") from None
    if not 1 <= T < 1 << 31:
        raise ValueError(f"max_points must be in [1, 2^31), got {max_points}")
    stacked = torch.is_tensor(depths)
    if stacked:
        if depths.dim() != 3:
            raise ValueError(f"depths: expected a list or tuple of (H,W) maps or one (V,H,W) tensor, got {tuple(depths.shape)}")
        maps = [depths[v] for v in range(depths.shape[0])]
    elif isinstance(depths, (list, tuple)) and all(torch.is_tensor(d) for d in depths):
        maps = list(depths)
    else:
        raise ValueError("depths: expected a list or tuple of (H,W) tensors, or one (V,H,W) tensor")
    V = len(maps)
    if not 2 <= V <= _MAX_VIEWS:
        raise ValueError(f"{V} views: 2 to {_MAX_VIEWS} are supported")
    if not 2 <= min_views <= V:
        raise ValueError(f"min_views must be in [2, V={V}], got {min_views}")
    for i, d in enumerate(maps):
        if d.dim() != 2 or not (1 <= d.shape[0] <= 32768 and 1 <= d.shape[1] <= 32768):
            raise ValueError(f"depth map {i}: expected (H,W) with sides in [1, 32768], got {tuple(d.shape)}")
    dims = [(int(d.shape[0]), int(d.shape[1])) for d in maps]
    total = sum(h * w for h, w in dims)
    if total >= 1 << 31:
        raise ValueError(f"the maps have {total} pixels in all, at most 2^31 - 1 are supported")
    if sizes is None:
        scale = [(1.0, 1.0)] * V
    else:
        try:
            sizes = [(int(h), int(w)) for h, w in sizes]
        except (TypeError, ValueError):
            raise ValueError("sizes: expected V pairs (H_img, W_img) of ints") from None
        if len(sizes) != V or any(h < 1 or w < 1 for h, w in sizes):
            raise ValueError(f"sizes: expected {V} pairs (H_img, W_img) of positive ints, got {sizes}")
        scale = [(w / wi, h / hi) for (h, w), (hi, wi) in zip(dims, sizes)]
    for name, v, shapes in (("R", R, ((V, 3, 3),)), ("t", t, ((V, 3),)), ("K", K, ((3, 3), (V, 3, 3)))):
        if tuple(getattr(v, "shape", ())) not in shapes:
            raise ValueError(f"{name}: expected {' or '.join(str(s) for s in shapes)}, got {tuple(getattr(v, 'shape', ()))}")
    _need_gpu(*maps)
    dev = maps[0].device
    for i, d in enumerate(maps):
        if d.dtype != torch.float32 or not d.is_contiguous() or d.data_ptr() % 4:
            raise ValueError(f"depth map {i}: {d.dtype} with strides {d.stride()} cannot be read in place (contiguous float32); pass "
                             ".float().contiguous() maps")
    Rp, tp = _poses(R, t, V, dev)
    Kp = _intrinsics(K, V, dev, "K")
    if any(sc != (1.0, 1.0) for sc in scale):
        Kp = Kp.clone()                                       # _intrinsics may have handed back the caller's own tensor
    for v, (sx, sy) in enumerate(scale):                      # Python scalars: kernel arguments, no copy from the host
        if sx != 1.0:
            Kp[v, 0] *= sx
        if sy != 1.0:
            Kp[v, 1] *= sy
    need = depth_fuse_workspace(V, total)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    depth = torch.empty((total,), dtype=torch.float32, device=dev)
    valid = torch.empty((total,), dtype=torch.bool, device=dev)
    views = torch.empty((total,), dtype=torch.int32, device=dev)
    num_views = torch.empty((total,), dtype=torch.uint8, device=dev)
    points = torch.empty((T, 3), dtype=torch.float32, device=dev)
    view = torch.empty((T,), dtype=torch.uint8, device=dev)
    pixel = torch.empty((T,), dtype=torch.int32, device=dev)
    point_views = torch.empty((T,), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    ptr_tab = (ctypes.c_void_p * V)(*[d.data_ptr() for d in maps])
    dim_tab = (ctypes.c_int * (2 * V))(*[s for hw in dims for s in hw])
    check(_lib.load().roma_depth_fuse(ctypes.cast(ptr_tab, ctypes.c_void_p), ctypes.cast(dim_tab, ctypes.c_void_p), Kp.data_ptr(), Rp.data_ptr(),
                                      tp.data_ptr(), V, reproj, rel, min_views, T, depth.data_ptr(), valid.data_ptr(), views.data_ptr(),
                                      num_views.data_ptr(), points.data_ptr(), view.data_ptr(), pixel.data_ptr(), point_views.data_ptr(),
                                      counts.data_ptr(), ws.data_ptr(), need, _stream()),
          "roma_depth_fuse")
    del maps                                                  # alive until the launches are queued; the stream orders the rest

    def per_view(flat):
        if stacked:
            return flat.view(V, *dims[0])
        out, at = [], 0
        for h, w in dims:
            out.append(flat[at:at + h * w].view(h, w))
            at += h * w
        return out

    return FusedDepth(per_view(depth), per_view(valid), per_view(views), per_view(num_views), points, view, pixel, point_views, counts)


# --------------------------------------------------------------------------------------------------------- point-cloud rendering
RenderedViews = collections.namedtuple("RenderedViews", ("depth", "index", "visible", "num_views", "counts", "attributes"))
RenderedViews.__doc__ = """What render_points returns, device tensors.  depth (V,H,W) fp32, the camera-frame z of the nearest point drawn
into the pixel, and index (V,H,W) int32, its row in the cloud (the lowest row among exactly equal depths); 0 and -1 where nothing was
drawn.  visible (N) int32: (visible >> v) & 1 says that view v sees point n, num_views (N) uint8 its popcount.  counts (4) int32:
projections inside a map, covered pixels, set visibility bits, points that are not live.  attributes: (V,H,W,C) or None."""


def render_points_workspace(V, H, W):
    """-> bytes of roma_render_points_workspace; raises ValueError on a bad shape"""
    need = _lib.load().roma_render_points_workspace(int(V), int(H), int(W), None)
    if need < 0:
        check(int(need), "roma_render_points_workspace")
    return int(need)


def render_points(points, R, t, K, shape, *, sizes=None, radius=0, depth_tol=0.05, mask=None, attributes=None):
    """A cloud drawn into the depth maps of V posed views (1 <= V <= 32) by a z-buffered point splat, and per point the views that see
    it (csrc/render_points.hip) — what looks at the cloud of fuse_depth_maps again from a camera: a depth map of the dense model for
    lift_keypoints and find_absolute_pose, for warp_kpts and dense_match_metrics, and occlusion-aware visibility of every point in every
    view.  Convention of fuse_depth_maps: x_v ~ K_v (R_v X + t_v); pixel (row i, column j) covers [j, j+1) x [i, i+1).
    points: (N,3) contiguous fp32 on the device, read in place; anything else is refused (make it .float().contiguous()).  R (V,3,3), t
    (V,3), or one pose (3,3), (3,) for V = 1; K (3,3) shared or (V,3,3); shape = (H, W), the same for all views; sizes: V pairs (H_img,
    W_img), the image size K_v refers to, default the maps' shape — K_v is scaled by diag(W / W_img, H / H_img, 1).  mask: (N) bool or
    uint8, a row with 0 is not drawn; for a fused cloud pass `fused.pixel >= 0`, since the rows past counts[0] are zeros and would draw
    the world's origin.  A row that is not finite is not drawn either.  A view whose K is singular or not upper triangular, or whose
    pose is not finite, gets an empty map and sees nothing.
    A point is drawn where it projects in front of the view and inside the map, into every pixel within `radius` (0 to 4) of its own in
    rows and columns; a pixel keeps the nearest point, in fp32, and among exactly equal depths the lowest row — by a 64-bit integer
    atomic minimum, so the maps do not depend on the order the points arrive in and two calls agree bit for bit.  A view sees a point
    when the point's depth is at most (1 + depth_tol) times the depth drawn at its own pixel.  With radius 0 the holes between splats
    let hidden points through; radius 1 closes them at the resolution the cloud was made at.
    attributes: (N,C), any dtype -> (V,H,W,C) = attributes[index], 0 where nothing was drawn (a torch gather).  Returns a RenderedViews.
    tests/render_points_ref.py restates it.  No host synchronisation: the call can be captured in a hipGraph."""
    try:
        H, W = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape: expected (H, W), got {shape!r}") from None
    if not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"shape: expected (H, W) with sides in [1, 32768], got {shape!r}")
    try:
        rad, tol = int(radius), float(depth_tol)
    except (TypeError, ValueError):
        raise ValueError(f"radius: expected an int and depth_tol a float, got {radius!r} and {depth_tol!r}") from None
    if rad != radius or not 0 <= rad <= 4:
        raise ValueError(f"radius must be an int in [0, 4], got {radius}")
    if not 0.0 <= tol < math.inf:
        raise ValueError(f"depth_tol must be finite and not negative, got {depth_tol}")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or not 1 <= points.shape[0] < 1 << 31:
        raise ValueError(f"points: expected a (N,3) tensor with 1 <= N < 2^31, got {tuple(getattr(points, 'shape', ()))}")
    N = int(points.shape[0])
    single = tuple(getattr(R, "shape", ())) == (3, 3)
    V = 1 if single else (int(R.shape[0]) if len(getattr(R, "shape", ())) == 3 else 0)
    if not 1 <= V <= _MAX_VIEWS:
        raise ValueError(f"R: expected (V,3,3) with 1 <= V <= {_MAX_VIEWS} or one (3,3), got {tuple(getattr(R, 'shape', ()))}")
    for name, v, shapes in (("R", R, ((3, 3),) if single else ((V, 3, 3),)), ("t", t, ((3,),) if single else ((V, 3),)),
                            ("K", K, ((3, 3), (V, 3, 3)))):
        if tuple(getattr(v, "shape", ())) not in shapes:
            raise ValueError(f"{name}: expected {' or '.join(str(s) for s in shapes)}, got {tuple(getattr(v, 'shape', ()))}")
    if V * H * W >= 1 << 31:
        raise ValueError(f"{V} maps of {H}x{W} have {V * H * W} pixels in all, at most 2^31 - 1 are supported")
    if sizes is None:
        scale = [(1.0, 1.0)] * V
    else:
        try:
            sizes = [(int(h), int(w)) for h, w in sizes]
        except (TypeError, ValueError):
            raise ValueError("sizes: expected V pairs (H_img, W_img) of ints") from None
        if len(sizes) != V or any(h < 1 or w < 1 for h, w in sizes):
            raise ValueError(f"sizes: expected {V} pairs (H_img, W_img) of positive ints, got {sizes}")
        scale = [(W / wi, H / hi) for hi, wi in sizes]
    if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != (N,) or mask.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"mask: expected a ({N},) bool or uint8 tensor, got {tuple(getattr(mask, 'shape', ()))} {getattr(mask, 'dtype', None)}")
    if attributes is not None and (not torch.is_tensor(attributes) or attributes.dim() != 2 or attributes.shape[0] != N):
        raise ValueError(f"attributes: expected a ({N},C) tensor, got {tuple(getattr(attributes, 'shape', ()))}")
    _need_gpu(points, mask, attributes)
    dev = points.device
    if points.dtype != torch.float32 or not points.is_contiguous() or points.data_ptr() % 4:
        raise ValueError(f"points: {points.dtype} with strides {points.stride()} cannot be read in place (contiguous float32); pass "
                         ".float().contiguous() points")
    if single:
        R, t = R[None], t[None]
    Rp, tp = _poses(R, t, V, dev)
    Kp = _intrinsics(K, V, dev, "K")
    if any(sc != (1.0, 1.0) for sc in scale):
        Kp = Kp.clone()                                       # _intrinsics may have handed back the caller's own tensor
    for v, (sx, sy) in enumerate(scale):                      # Python scalars: kernel arguments, no copy from the host
        if sx != 1.0:
            Kp[v, 0] *= sx
        if sy != 1.0:
            Kp[v, 1] *= sy
    mk = None if mask is None else mask.contiguous().view(torch.uint8)
    need = render_points_workspace(V, H, W)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    index = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    visible = torch.empty((N,), dtype=torch.int32, device=dev)
    num_views = torch.empty((N,), dtype=torch.uint8, device=dev)
    counts = torch.empty((4,), dtype=torch.int32, device=dev)
    check(_lib.load().roma_render_points(points.data_ptr(), None if mk is None else mk.data_ptr(), N, Kp.data_ptr(), Rp.data_ptr(),
                                         tp.data_ptr(), V, H, W, rad, tol, depth.data_ptr(), index.data_ptr(), visible.data_ptr(),
                                         num_views.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, _stream()),
          "roma_render_points")
    drawn = None
    if attributes is not None:
        drawn = attributes[index.clamp(min=0).to(torch.int64)]
        drawn = torch.where((index >= 0)[..., None], drawn, torch.zeros((), dtype=drawn.dtype, device=dev))
    return RenderedViews(depth, index, visible, num_views, counts, drawn)


def reconstruction_error(R, t, X, R_gt, t_gt, X_gt):
    """A reconstruction (R (V,3,3), t (V,3), X (N,3)) against the truth, whatever frame and unit it is in: the camera centres C_v =
    -R_v^T t_v are aligned to the true ones by the closed-form similarity (Umeyama: C_gt ~ s Q C + tau, what similarity.hip's
    refinement computes), then -> (the worst rotation error of a view in degrees, the worst distance of an aligned centre from the true
    one, the median distance of an aligned point from the true one; rows of X or X_gt that are not finite are left out), fp64 scalars.
    torch ops only, CPU or device tensors (the 3 x 3 SVD runs on the host).  Three views or more whose centres are not collinear
    determine the alignment; with fewer the rotation about the baseline is free and the figures mean little."""
    R, t, X, R_gt, t_gt, X_gt = (torch.as_tensor(v).to(torch.float64) for v in (R, t, X, R_gt, t_gt, X_gt))
    dev = R.device
    R_gt, t_gt, X_gt = R_gt.to(dev), t_gt.to(dev), X_gt.to(dev)
    C = -(R.transpose(-1, -2) @ t[..., None]).squeeze(-1)
    Cg = -(R_gt.transpose(-1, -2) @ t_gt[..., None]).squeeze(-1)
    mc, mg = C.mean(0), Cg.mean(0)
    A, B = C - mc, Cg - mg
    U, S, Vh = torch.linalg.svd((B.T @ A).cpu())
    d = torch.ones(3, dtype=torch.float64)
    d[2] = torch.sign(torch.linalg.det(U @ Vh))
    Q = (U @ torch.diag(d) @ Vh).to(dev)
    s = (S * d).sum().to(dev) / (A * A).sum()
    tau = mg - s * (Q @ mc)
    cos = (((R @ Q.T) * R_gt).sum((-1, -2)) - 1.0) / 2.0
    e_R = torch.rad2deg(torch.acos(torch.clamp(cos, -1.0, 1.0))).max()
    e_C = torch.linalg.norm(s * (C @ Q.T) + tau - Cg, dim=-1).max()
    dX = torch.linalg.norm(s * (X @ Q.T) + tau - X_gt, dim=-1)
    e_X = dX[torch.isfinite(dX)].median()
    return e_R, e_C, e_X
