# roma_amd.geometry absolute pose: time per call of find_absolute_pose at its defaults (1 000 P3P samples, 3 rounds of local
# optimisation, no refinement), of its two C entry points apart (hypotheses = prepare + P3P + scoring + reduction; select), of
# refine_absolute_pose alone from the RANSAC pose and of find_absolute_pose(refine_iters=15), at P = 1 and P = 64 pairs of N = 10 000
# matches; and, for scale, find_essential at the same P, N and number of samples.  Device events after 3 warm-up calls, the callables
# alternating in one loop, median of `reps` (default 20) with the minimum beside it.  Slot-point evaluations = valid slots * N (the
# scoring work).  Nothing to compare with: the numbers are reported as measured.
# `absolute_pose_micro.py [reps]` runs every case as a child process of its own under a time limit, stops at the first that fails,
# and writes what they printed to profiles/absolute_pose_micro.txt; `absolute_pose_micro.py --case P [reps]` is one case, to stdout
# (e.g. under a kernel trace).
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (1, 64)
N, ITERS, THR = 10000, 1000, 2.0
CASE_LIMIT_S = 240


def scenes(P):
    import numpy as np
    from tests import absolute_pose_ref as A
    from tests import general_scenes as GS
    motions = tuple(GS.MOTIONS)
    ap = [A.scene(motions[p % 4], 100 + p, N=N)[:2] for p in range(P)]
    tv = [GS.general_scene(motions[p % 4], 100 + p, N=N)[:2] for p in range(P)]
    return (np.stack([s[0] for s in ap]), np.stack([s[1] for s in ap]), np.stack([s[0] for s in tv]), np.stack([s[1] for s in tv]))


def case(P, reps):
    import ctypes
    import numpy as np
    import torch
    from roma_amd import _lib, geometry
    from tests import general_scenes as GS
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    X, x, xa, xb = (dev(a) for a in scenes(P))
    K, KA = dev(GS.K_B), dev(GS.K_A)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    total, _ = geometry.absolute_pose_workspace_layout(P, N, ITERS)
    ws = torch.empty((total,), dtype=torch.uint8, device=X.device)
    Kp = K.expand(P, 3, 3).contiguous()
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=X.device)
    t = torch.empty((P, 3), dtype=torch.float64, device=X.device)
    mask = torch.empty((P, N), dtype=torch.uint8, device=X.device)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731

    def hypotheses():
        _lib.check(lib.roma_absolute_pose_hypotheses(ptr(X), ptr(x), ptr(Kp), P, N, ITERS, THR, 0, 0, 0, ptr(ws), total, stream), "hypotheses")

    def select():
        _lib.check(lib.roma_absolute_pose_select(ptr(X), ptr(x), ptr(Kp), P, N, ITERS, THR, 0, 3, ptr(ws), total, ptr(R), ptr(t), ptr(mask),
                                                 stream), "select")

    R0, t0, _ = geometry.find_absolute_pose(X, x, K, THR, ITERS, seed=0)
    calls = {
        "find_absolute_pose": lambda: geometry.find_absolute_pose(X, x, K, THR, ITERS, seed=0),
        "  hypotheses": hypotheses,
        "  select": select,
        "refine_absolute_pose": lambda: geometry.refine_absolute_pose(R0, t0, X, x, K, THR, 15),
        "find_absolute_pose(refine_iters=15)": lambda: geometry.find_absolute_pose(X, x, K, THR, ITERS, seed=0, refine_iters=15),
        "find_absolute_pose(scoring='magsac')": lambda: geometry.find_absolute_pose(X, x, K, THR, ITERS, seed=0, scoring="magsac"),
        "find_essential": lambda: geometry.find_essential(xa, xb, KA, K, GS.THR_G, ITERS, seed=0),
    }
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    hyp = geometry.absolute_pose_hypotheses(X[:8], x[:8], K, THR, ITERS, seed=0)
    slots = float(hyp["valid"].float().sum(dim=(1, 2)).mean())
    steps = geometry.refine_absolute_pose(R0, t0, X, x, K, THR, 15, return_info=True)[3]["steps"].float()
    print(f"P={P:3d} N={N} samples={ITERS}: {slots:.0f} valid slots per pair = {slots * N:.3e} slot-point evaluations; "
          f"inliers {float(mask.float().mean()):.3f}; refinement keeps {float(steps.mean()):.2f} steps of 15 (max {int(steps.max())})")
    for name, ts in times.items():
        med = float(np.median(ts))
        rate = f"  {P * slots * N / (med * 1e-3):.3e} slot-point evaluations/s" if name.strip() == "hypotheses" else ""
        print(f"  {name:38s} {med:9.3f} ms/call (median of {reps}, min {min(ts):.3f})  {med / P:8.4f} ms/pair{rate}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        case(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 20)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "20"
    lines = [f"find_absolute_pose / refine_absolute_pose / find_essential, device events, median of {reps} alternating calls after 3 "
             f"warm-up calls; threshold {THR} px, 30 % outliers, sigma 0.5 px"]
    status = 0
    for P in CASES:                                        # one process and one time limit per case; nothing follows a failure
        r = subprocess.run(["timeout", "-k", "10", str(CASE_LIMIT_S), sys.executable, os.path.abspath(__file__), "--case", str(P), reps],
                           capture_output=True, text=True, cwd=ROOT)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append(f"P={P}: the case ended with status {r.returncode}; the cases after it were not run")
            sys.stderr.write(r.stderr[-2000:])
            status = r.returncode
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if status == 0:
        with open(os.path.join(ROOT, "profiles", "absolute_pose_micro.txt"), "w") as f:
            f.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
