# roma_amd.geometry similarity registration: time per call of find_similarity at its defaults (1 000 three-point samples, 3 rounds of
# local optimisation, no refinement), of its two C entry points apart (hypotheses = prepare + solver + scoring + reduction; select),
# of refine_similarity alone from the RANSAC model and of find_similarity(scoring="magsac"), at (P, N) = (1, 10 000), (64, 10 000)
# and (1, 1 492 992) — the last is two lifted depth maps of an 864 x 1 728 warp — and, as the yardstick, find_absolute_pose at the
# first two shapes in the same run.  Device events after 3 warm-up calls, the callables alternating in one loop, median of `reps`
# (default 20) with the minimum beside it.  Slot-point evaluations = valid slots * N (the scoring work).  Nothing is fixed in advance:
# the numbers are reported as measured.
# `similarity_micro.py [reps]` runs every case as a child process of its own under a time limit, stops at the first that fails, and
# writes what they printed to profiles/similarity_micro.txt; `similarity_micro.py --case P N [reps]` is one case, to stdout (e.g.
# under a kernel trace).
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((1, 10000), (64, 10000), (1, 864 * 1728))
ITERS = 1000
CASE_LIMIT_S = 300


def scenes(P, N):
    import numpy as np
    from tests import similarity_ref as S
    sim = [S.scene(100 + p, (0.05, 1.0, 20.0)[p % 3], N=N) for p in range(min(P, 3))]
    X, Y = np.stack([sim[p % len(sim)][0] for p in range(P)]), np.stack([sim[p % len(sim)][1] for p in range(P)])
    Y = Y / np.array([sim[p % len(sim)][3][0] for p in range(P)])[:, None, None]      # one threshold per call: Y in X's unit
    return X, Y, sim[0][4] / sim[0][3][0]


def absolute_pose_scenes(P, N):
    import numpy as np
    from tests import absolute_pose_ref as A
    from tests import general_scenes as GS
    motions = tuple(GS.MOTIONS)
    ap = [A.scene(motions[p % 4], 100 + p, N=N)[:2] for p in range(min(P, 4))]
    return np.stack([ap[p % len(ap)][0] for p in range(P)]), np.stack([ap[p % len(ap)][1] for p in range(P)])


def case(P, N, reps):
    import ctypes
    import numpy as np
    import torch
    from roma_amd import _lib, geometry
    from tests import general_scenes as GS
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    Xn, Yn, thr = scenes(P, N)
    X, Y = dev(Xn), dev(Yn)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    total, _ = geometry.similarity_workspace_layout(P, N, ITERS)
    ws = torch.empty((total,), dtype=torch.uint8, device=X.device)
    s = torch.empty((P,), dtype=torch.float64, device=X.device)
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=X.device)
    t = torch.empty((P, 3), dtype=torch.float64, device=X.device)
    mask = torch.empty((P, N), dtype=torch.uint8, device=X.device)
    valid = torch.empty((P,), dtype=torch.int32, device=X.device)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731

    def hypotheses():
        _lib.check(lib.roma_similarity_hypotheses(ptr(X), ptr(Y), P, N, ITERS, thr, 0, 1, 0, 0, ptr(ws), total, stream), "hypotheses")

    def select():
        _lib.check(lib.roma_similarity_select(ptr(X), ptr(Y), P, N, ITERS, thr, 0, 1, 3, ptr(ws), total, ptr(s), ptr(R), ptr(t), ptr(mask),
                                              ptr(valid), stream), "select")

    s0, R0, t0, _ = geometry.find_similarity(X, Y, thr, ITERS, seed=0)
    calls = {
        "find_similarity": lambda: geometry.find_similarity(X, Y, thr, ITERS, seed=0),
        "  hypotheses": hypotheses,
        "  select": select,
        "refine_similarity": lambda: geometry.refine_similarity(s0, R0, t0, X, Y, thr, 15),
        "find_similarity(scoring='magsac')": lambda: geometry.find_similarity(X, Y, thr, ITERS, seed=0, scoring="magsac"),
    }
    if N <= 100000:                                        # the yardstick, at the shapes it was measured at before
        Xa, xa = (dev(a) for a in absolute_pose_scenes(P, N))
        K = dev(GS.K_B)
        Ra, ta, _ = geometry.find_absolute_pose(Xa, xa, K, 2.0, ITERS, seed=0)
        calls["find_absolute_pose"] = lambda: geometry.find_absolute_pose(Xa, xa, K, 2.0, ITERS, seed=0)
        calls["refine_absolute_pose"] = lambda: geometry.refine_absolute_pose(Ra, ta, Xa, xa, K, 2.0, 15)
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    hypotheses()
    select()
    hyp = geometry.similarity_hypotheses(X[:1], Y[:1], thr, ITERS, seed=0)
    slots = float(hyp["valid"].float().sum())
    steps = geometry.refine_similarity(s0, R0, t0, X, Y, thr, 15, return_info=True)[4]["steps"].float()
    print(f"P={P:3d} N={N} samples={ITERS}: {slots:.0f} valid slots per pair = {slots * N:.3e} slot-point evaluations; "
          f"inliers {float(mask.float().mean()):.3f}; refinement keeps {float(steps.mean()):.2f} rounds of 15 (max {int(steps.max())}); "
          f"workspace {total / 2 ** 20:.1f} MiB")
    for name, ts in times.items():
        med = float(np.median(ts))
        rate = f"  {P * slots * N / (med * 1e-3):.3e} slot-point evaluations/s" if name.strip() == "hypotheses" else ""
        print(f"  {name:38s} {med:9.3f} ms/call (median of {reps}, min {min(ts):.3f})  {med / P:8.4f} ms/pair{rate}")


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--case":
        case(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 20)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "20"
    lines = [f"find_similarity / refine_similarity, and find_absolute_pose / refine_absolute_pose beside them, device events, median of {reps} "
             "alternating calls after 3 warm-up calls; threshold 4 sqrt 2 sigma, 30 % outliers, sigma 0.01 (absolute pose: 2.0 px, 0.5 px)"]
    status = 0
    for P, N in CASES:                                     # one process and one time limit per case; nothing follows a failure
        r = subprocess.run(["timeout", "-k", "10", str(CASE_LIMIT_S), sys.executable, os.path.abspath(__file__), "--case", str(P), str(N), reps],
                           capture_output=True, text=True, cwd=ROOT)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append(f"P={P} N={N}: the case ended with status {r.returncode}; the cases after it were not run")
            sys.stderr.write(r.stderr[-2000:])
            status = r.returncode
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if status == 0:
        with open(os.path.join(ROOT, "profiles", "similarity_micro.txt"), "w") as f:
            f.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
