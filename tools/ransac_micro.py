# roma_amd.geometry call times with device events after warm-up: F at P = 1 (N = 10 000, 10 000 samples), F at P = 64 (N = 5 000,
# MegaDepth-style), H at P = 1 (N = 5 000, 2 000 samples), E (find_essential) and pose (estimate_pose = find_essential +
# recover_pose) at P = 1 / N = 10 000 and P = 64 / N = 5 000 with 2 000 samples.  Model-point evaluations = P * samples * valid
# slots * N (the scoring work).  `ransac_micro.py [reps] [kinds]`, e.g. `ransac_micro.py 3 E,pose` for a kernel trace of the E path.
# refine = refine_pose alone from the pose of estimate_pose (seed 0), relpose = estimate_relative_pose (find_essential +
# recover_pose + refine_pose), at the two pose shapes; their lines give the kept steps instead of model-point evaluations.
# refineF = refine_fundamental alone from the model of find_fundamental (seed 0), Fref = find_fundamental(refine_iters=15), at the
# two F shapes: the extra cost of the refinement inside the estimator is Fref minus F of the same run.
# refineH = refine_homography alone from the model of find_homography (seed 0), Href = find_homography(refine_iters=15), at the H
# shape and at P = 64 / N = 5 000: the extra cost of the refinement inside the estimator is Href minus H of the same run.
# `ransac_micro.py 10 F,H,E msac,magsac` adds the MAGSAC++ scoring: every F / H / E / pose case is then timed with each scoring named,
# at its threshold and at the generous one of DESIGN.md §3.4 (WIDE: where MAGSAC++ is meant to be used, and where it looks up more
# inliers), and the magsac lines end with their time over the msac time of the same case and threshold.
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import geometry  # noqa: E402
from tests import geometry_ref as G  # noqa: E402
from tests import pose_ref as PR  # noqa: E402

CASES = [("F", 1, 10000, 10000, 1.5), ("F", 64, 5000, 10000, 1.5), ("H", 1, 5000, 2000, 3.0), ("H", 64, 5000, 2000, 3.0),
         ("E", 1, 10000, 2000, 1.5 / 800), ("E", 64, 5000, 2000, 1.5 / 800), ("pose", 1, 10000, 2000, 1.5 / 800),
         ("pose", 64, 5000, 2000, 1.5 / 800), ("refine", 1, 10000, 2000, 1.5 / 800), ("refine", 64, 5000, 2000, 1.5 / 800),
         ("relpose", 1, 10000, 2000, 1.5 / 800), ("relpose", 64, 5000, 2000, 1.5 / 800),
         ("refineF", 1, 10000, 10000, 1.5), ("refineF", 64, 5000, 10000, 1.5), ("Fref", 1, 10000, 10000, 1.5), ("Fref", 64, 5000, 10000, 1.5),
         ("refineH", 1, 5000, 2000, 3.0), ("refineH", 64, 5000, 2000, 3.0), ("Href", 1, 5000, 2000, 3.0), ("Href", 64, 5000, 2000, 3.0)]
MODEL = {"F": "fundamental", "H": "homography", "E": "essential", "pose": "essential", "Fref": "fundamental",
         "Href": "homography"}
CAMERA = {"model": "PINHOLE", "params": [800.0, 800.0, G.W_IMG / 2, G.H_IMG / 2]}
PLANAR = ("H", "refineH", "Href")
WIDE = {"F": 6.0, "H": 25.0, "E": 6.0 / 800, "pose": 6.0 / 800}


_SCENES = {}


def scene(kind, P, N):
    key = (kind in PLANAR, P, N)
    if key not in _SCENES:
        _SCENES[key] = _scene(kind, P, N)
    return _SCENES[key]


def _scene(kind, P, N):
    make = G.planar_scene if kind in PLANAR else G.two_view_scene
    pts = [make(100 + i, N=N)[:2] for i in range(P)]
    return (torch.from_numpy(np.stack([p[0] for p in pts])).float().cuda(), torch.from_numpy(np.stack([p[1] for p in pts])).float().cuda())


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    kinds = sys.argv[2].split(",") if len(sys.argv) > 2 else ["F", "H", "E", "pose", "refine", "relpose", "refineF", "Fref", "refineH", "Href"]
    scorings = sys.argv[3].split(",") if len(sys.argv) > 3 else ["msac"]
    K = torch.from_numpy(PR.K_SCENE).cuda()
    runs = [(c, "msac", c[4]) for c in CASES]
    if scorings != ["msac"]:
        runs = [(c, sc, thr) for c in CASES for thr in ((c[4], WIDE[c[0]]) if c[0] in WIDE else (c[4],))
                for sc in (scorings if c[0] in WIDE else ["msac"])]
    base = {}
    for (kind, P, N, iters, _), scoring, thr in runs:
        if kind not in kinds:
            continue
        xa, xb = scene(kind, P, N)
        score = {} if scoring == "msac" else {"scoring": scoring}
        label = kind if scoring == "msac" and scorings == ["msac"] else f"{kind}/{scoring} thr={thr:.4g}"
        if kind == "E":
            def fn(a, b, threshold, max_iters, seed):
                return geometry.find_essential(a, b, K, K, threshold, max_iters=max_iters, seed=seed, **score)
        elif kind == "pose":
            def fn(a, b, threshold, max_iters, seed):
                return geometry.estimate_pose(a, b, K, K, threshold, max_iters=max_iters, seed=seed, **score)
        elif kind == "refine":
            R0, t0, _ = geometry.estimate_pose(xa, xb, K, K, thr, max_iters=iters, seed=0)

            def fn(a, b, threshold, max_iters, seed):
                return geometry.refine_pose(R0, t0, a, b, K, K, threshold, return_info=True)
        elif kind == "relpose":
            def fn(a, b, threshold, max_iters, seed):
                return geometry.estimate_relative_pose(a, b, CAMERA, CAMERA, {"max_epipolar_error": threshold * 800,
                                                                              "max_iterations": max_iters}, seed=seed)
        elif kind == "refineF":
            F0, _ = geometry.find_fundamental(xa, xb, threshold=thr, max_iters=iters, seed=0)

            def fn(a, b, threshold, max_iters, seed):
                return geometry.refine_fundamental(F0, a, b, threshold, return_info=True)
        elif kind == "Fref":
            def fn(a, b, threshold, max_iters, seed):
                return geometry.find_fundamental(a, b, threshold=threshold, max_iters=max_iters, seed=seed, refine_iters=15)
        elif kind == "refineH":
            H0, _ = geometry.find_homography(xa, xb, threshold=thr, max_iters=iters, seed=0)

            def fn(a, b, threshold, max_iters, seed):
                return geometry.refine_homography(H0, a, b, threshold, return_info=True)
        elif kind == "Href":
            def fn(a, b, threshold, max_iters, seed):
                return geometry.find_homography(a, b, threshold=threshold, max_iters=max_iters, seed=seed, refine_iters=15)
        else:
            def fn(a, b, threshold, max_iters, seed):
                return (geometry.find_fundamental if kind == "F" else geometry.find_homography)(a, b, threshold=threshold,
                                                                                                max_iters=max_iters, seed=seed, **score)
        for _ in range(3):
            fn(xa, xb, threshold=thr, max_iters=iters, seed=0)
        torch.cuda.synchronize()
        times = []
        for r in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(xa, xb, threshold=thr, max_iters=iters, seed=r)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        ms = float(np.median(times))
        if kind in ("refine", "relpose", "refineF", "refineH"):
            out = fn(xa, xb, threshold=thr, max_iters=iters, seed=0)
            steps = (out[1]["refinements"] if kind == "relpose" else out[-1]["steps"]).float()
            print(f"{kind:7s} P={P:3d} N={N:5d} iters={iters:5d}: {ms:8.3f} ms/call (median of {reps}, min {min(times):.3f})  "
                  f"{ms / P:7.3f} ms/pair  kept LM steps: mean {float(steps.mean()):.2f}, max {int(steps.max())} of 15")
            continue
        # valid models at seed 0, counted on slices of 16 pairs (score_hypotheses keeps a whole batch's hypotheses)
        extra = {"K_A": K, "K_B": K} if MODEL[kind] == "essential" else {}
        valid = sum(int(geometry.score_hypotheses(xa[a:a + 16], xb[a:a + 16], MODEL[kind], thr, iters, seed=0, **extra)["valid"].sum())
                    for a in range(0, P, 16))
        evals = valid * N
        if scoring == "msac":
            base[(kind, P, thr)] = ms
        ratio = f"  {ms / base[(kind, P, thr)]:.2f} x msac" if scoring != "msac" and (kind, P, thr) in base else ""
        print(f"{label:4s} P={P:3d} N={N:5d} iters={iters:5d}: {ms:8.3f} ms/call (median of {reps}, min {min(times):.3f})  "
              f"{ms / P:7.3f} ms/pair  {evals / (ms * 1e-3):.3e} model-point evaluations/s  ({evals:.3e} evaluations, "
              f"{valid} valid models){ratio}")


if __name__ == "__main__":
    main()
