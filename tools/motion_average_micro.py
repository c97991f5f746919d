# roma_amd.geometry.average_rotations / global_positions (csrc/motion_average.hip): time of one call of each, the split of
# global_positions by kernel from a rocprofv3 kernel trace, and the same passes of global_positions written as torch ops on the device
# (vote, per round the elimination of the points in chunks of 8192, torch.linalg.eigh, the points, the weights) as the yardstick.
# Device events after 2 warm-up calls, median of `reps` (default 5) calls.
# Shapes: 8 views x 16 384 tracks and 32 views x 131 072 tracks, the scene of tools/bundle_micro.py (cameras on a circle looking at its
# centre, a track seen by about 4 consecutive views, 0.5 px of noise).  The pose graph joins every view to the next three on the circle;
# its edges come from the true poses with 0.2 deg of noise on the rotation and 0.5 deg on the translation direction, every 7th an outlier
# (25 deg, 40 deg).  Threshold 4 px, 4 rounds, 12 rotation rounds, root 0.
# `motion_average_micro.py [reps]` runs every case in child processes of their own under `timeout` (timing, then the kernel trace), one
# after the other, and stops at the first that fails; `--case V N reps` and `--trace V N` are what a child runs.
# The committed output is profiles/motion_average_micro.txt.
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [(8, 1 << 14), (32, 1 << 17)]
THR, ROUNDS = 4.0, 4
CASE_TIMEOUT = 240                                           # seconds, per child
CHUNK = 8192


def device_args(V, N):
    import numpy as np
    import torch
    from bundle_micro import make_scene
    from tests.geometry_ref import rodrigues
    x, K, R, t = make_scene(V, N)[:4]
    rng = np.random.default_rng(7)
    pairs = np.array([(v, (v + k) % V) for v in range(V) for k in (1, 2, 3)], np.int32)
    R_rel, t_rel = [], []
    for m, (a, b) in enumerate(pairs):
        Rab = R[b] @ R[a].T
        tab = t[b] - Rab @ t[a]
        bad = m % 7 == 3
        R_rel.append(rodrigues(np.radians(25.0 if bad else 0.2) * rng.normal(size=3)) @ Rab)
        t_rel.append(rodrigues(np.radians(40.0 if bad else 0.5) * rng.normal(size=3)) @ (tab / np.linalg.norm(tab)))
    dev = lambda a: torch.tensor(np.asarray(a), device="cuda")  # noqa: E731
    return dev(x), dev(K), dev(pairs), dev(np.stack(R_rel)), dev(np.stack(t_rel)), R, t


def torch_positions(x, R, K, pairs, t_rel, thr=THR, rounds=ROUNDS, root=0):
    """the passes of global_positions as torch ops (fp64) -> centres (V,3), points (N,3), mask (V,N)"""
    import torch
    V, N = x.shape[:2]
    x = x.double()
    seen = torch.isfinite(x).all(-1)
    h = torch.cat([torch.nan_to_num(x), torch.ones_like(x[..., :1])], -1) @ torch.linalg.inv(K).T
    d = (h / h.norm(dim=-1, keepdim=True)) @ R                                  # row n of view v: R_v^T h
    ang = thr / (K[0, 0] * K[1, 1]).abs().sqrt()
    a, b = pairs[:, 0].long(), pairs[:, 1].long()
    bm = -torch.einsum("mji,mj->mi", R[b], t_rel / t_rel.norm(dim=-1, keepdim=True))
    both = seen[a] & seen[b]
    agree = both & ((torch.linalg.cross(d[a], d[b]) * bm[:, None]).sum(-1).abs() < 2 * ang)
    cnt, vote = torch.zeros(V, N, dtype=torch.float64, device=x.device), torch.zeros(V, N, dtype=torch.float64, device=x.device)
    for idx in (a, b):
        cnt.index_add_(0, idx, both.double())
        vote.index_add_(0, idx, agree.double())
    w = ((vote >= 1) & (2 * vote >= cnt) & seen).double()
    P = (torch.eye(3, dtype=torch.float64, device=x.device) - d[..., :, None] * d[..., None, :]) * seen[..., None, None]
    alive = torch.ones(N, dtype=torch.bool, device=x.device)
    keep = torch.tensor([i for v in range(V) if v != root for i in (3 * v, 3 * v + 1, 3 * v + 2)], device=x.device)
    for r in range(rounds):
        Q = w[..., None, None] * P
        A = Q.sum(0)
        tr = A.diagonal(dim1=-2, dim2=-1).sum(-1)
        alive = alive & ((w > 0).sum(0) >= 2) & (torch.linalg.det(A) > 1e-12 * tr ** 3)
        w = w * alive
        Q = w[..., None, None] * P
        Ainv = torch.linalg.inv(torch.where(alive[:, None, None], A, torch.eye(3, dtype=torch.float64, device=x.device))) * alive[:, None, None]
        S = torch.zeros(3 * V, 3 * V, dtype=torch.float64, device=x.device)
        S.view(V, 3, V, 3).diagonal(dim1=0, dim2=2).add_(Q.sum(1).permute(1, 2, 0))
        for s in range(0, N, CHUNK):
            QA = torch.einsum("vnij,njk->nvik", Q[:, s:s + CHUNK], Ainv[s:s + CHUNK])
            S -= torch.einsum("nvik,unkl->viul", QA, Q[:, s:s + CHUNK]).reshape(3 * V, 3 * V)
        Sr = S[keep][:, keep]
        lam, vec = torch.linalg.eigh(0.5 * (Sr + Sr.T))
        C = torch.zeros(3 * V, dtype=torch.float64, device=x.device)
        C[keep] = vec[:, 0]
        C = C.view(V, 3)
        X = torch.einsum("nij,nj->ni", Ainv, torch.einsum("vnij,vj->ni", Q, C))
        rel = X[None] - C[:, None]
        depth = (rel * d).sum(-1)
        if (w * depth).sum() < 0:
            C, X, rel, depth = -C, -X, -rel, -depth
        dist = rel.norm(dim=-1)
        a_ = (rel - d * depth[..., None]).norm(dim=-1) / dist
        good = seen & alive[None] & (depth > 0) & (dist > 1e-12)
        if r >= rounds - 2:
            good = good & (a_ < ang)
        w = torch.where(good, 1.0 / (1.0 + (a_ / (ang * 2.0 ** max(rounds - 2 - r, 0))) ** 2), torch.zeros_like(a_))
    return C, X, w > 0


def run_case(V, N, reps):
    import numpy as np
    import torch
    from roma_amd import geometry
    from tests import motion_ref as MR
    x, K, pairs, R_rel, t_rel, R_true, t_true = device_args(V, N)

    def timed(fn):
        times = []
        for i in range(reps + 2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn()
            e.record()
            torch.cuda.synchronize()
            if i >= 2:
                times.append(s.elapsed_time(e))
        return float(np.median(times)), min(times), r

    t_rot, m_rot, rot = timed(lambda: geometry.average_rotations(R_rel, pairs, V))
    t_pos, m_pos, pos = timed(lambda: geometry.global_positions(x, rot.R, K, pairs, t_rel, threshold=THR, rounds=ROUNDS))
    t_ref, m_ref, ref = timed(lambda: torch_positions(x, rot.R, K, pairs, t_rel))
    need, _ = geometry.positions_workspace_layout(V, N, len(pairs))
    obs = int(torch.isfinite(x[..., 0]).sum())
    er = MR.rotation_error_deg(rot.R.cpu().numpy(), R_true)
    ec = MR.centre_error(pos.centres.cpu().numpy(), R_true, t_true)
    gap = float((pos.centres - ref[0]).abs().max())
    same = float((pos.mask == ref[2]).double().mean())
    res = rot.residual_deg.cpu().numpy()
    bad = np.arange(len(res)) % 7 == 3
    print(f"V = {V:2d}, N = {N:6d} ({obs} observations, {len(pairs)} edges, {3 * (V - 1)} unknowns, workspace {need / 2 ** 20:5.1f} MiB): "
          f"average_rotations {t_rot:7.3f} ms (min {m_rot:.3f}), global_positions {t_pos:8.3f} ms (min {m_pos:.3f}), the torch passes {t_ref:9.3f} ms "
          f"(min {m_ref:.3f}): {t_ref / t_pos:.1f} x", flush=True)
    print(f"    worst rotation error {er:.3f} deg (edge residuals: outliers >= {res[bad].min():.1f} deg, the rest <= {res[~bad].max():.2f} deg), worst centre "
          f"error {ec:.5f} of the extent, mask {int(pos.count)} of {obs}, eigenvalues {float(pos.eigenvalues[0]):.3e}, {float(pos.eigenvalues[1]):.3e}, "
          f"status {int(rot.status)} / {int(pos.status)}; against the torch passes: centres differ by {gap:.1e}, {100 * same:.3f} % of the mask equal",
          flush=True)


def run_trace_child(V, N):
    import torch
    from roma_amd import geometry
    x, K, pairs, R_rel, t_rel, _, _ = device_args(V, N)
    for _ in range(2):
        geometry.initialize_cameras(x, K, pairs, R_rel, t_rel, threshold=THR)
    torch.cuda.synchronize()


def trace(V, N):
    """the kernels of two calls from a rocprofv3 kernel trace of a child: average time per launch and the share of a round"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print("    rocprofv3 is not on this machine: no split by kernel", flush=True)
        return 0
    out = tempfile.mkdtemp(prefix="motion_micro_")
    try:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT), prof, "--kernel-trace", "--stats", "-d", out, "-o", "motion", "--output-format",
                             "csv", "--", sys.executable, os.path.abspath(__file__), "--trace", str(V), str(N)], stdout=subprocess.DEVNULL,
                            stderr=subprocess.DEVNULL).returncode
        if rc != 0:
            return rc
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("    the trace left no kernel_stats.csv: no split by kernel", flush=True)
            return 0
        rows = list(csv.DictReader(open(files[0])))
        step = ("accumulate", "reduce", "solve", "points", "sign")
        avg = {n: float(r["AverageNs"]) / 1e3 for r in rows for n in step + ("init", "vote", "final") if f"positions_{n}_kernel" in r["Name"]}
        avg.update({"rotations": float(r["AverageNs"]) / 1e3 for r in rows if "rotation_average_kernel" in r["Name"]})
        total = sum(avg.get(n, 0.0) for n in step)
        print("    per launch, us: " + ", ".join(f"{n} {avg[n]:.1f}" for n in ("rotations", "init", "vote") + step + ("final",) if n in avg) +
              f";  one round {total:.1f} us of kernel time: " + ", ".join(f"{n} {100 * avg.get(n, 0.0) / total:.0f} %" for n in step), flush=True)
        return 0
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] in ("--case", "--trace"):
        V, N = int(sys.argv[2]), int(sys.argv[3])
        if sys.argv[1] == "--case":
            run_case(V, N, int(sys.argv[4]) if len(sys.argv) > 4 else 5)
        else:
            run_trace_child(V, N)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    print(f"average_rotations (12 rounds) and global_positions (threshold {THR} px, {ROUNDS} rounds); device events, median of {reps} calls after 2 "
          f"warm-up calls", flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    for V, N in CASES:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT)] + me + ["--case", str(V), str(N), reps]).returncode
        if rc == 0:
            rc = trace(V, N)
        if rc != 0:
            print(f"V = {V}, N = {N}: the child ended with status {rc}; stopping", flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
