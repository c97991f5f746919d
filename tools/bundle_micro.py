# roma_amd.geometry.bundle_adjust: time of one call and of one Levenberg-Marquardt step (six launches, csrc/bundle.hip), the split by
# kernel from a rocprofv3 kernel trace, and, where scipy is importable, scipy.optimize.least_squares with a sparse Jacobian on the
# smaller problem as the host yardstick.  Device events after 2 warm-up calls, median of `reps` (default 5) calls of ITERS = 10 steps;
# the time of a step is (call with 10 steps - call with 0 steps) / 10: every launch of a step runs whether the step is kept or not,
# unless the state record says finished (a call that finished early is reported as such).
# Shapes: V = 8 and 32 views, N = 2^14 and 2^17 tracks of about 4 views each.  The scene: cameras on a circle of radius 6 looking at
# its centre, points uniform in a ball of radius 2, a track seen by 4 consecutive views from a random first one (3 to 5 with V = 32:
# one in five tracks gains or loses a view), 0.5 px of noise, no outliers; the start: every view but 0 and 1 turned by 0.1 deg about
# each axis and moved by 0.01, every point moved by 0.5 % of its depth; threshold 2 px, views 0 and 1 held.
# `bundle_micro.py [reps]` runs every case in child processes of their own under `timeout` (timing, then the kernel trace, then scipy),
# one after the other, and stops at the first that fails; `--case V N reps`, `--trace V N` and `--scipy V N` are what a child runs.
# The committed output is profiles/bundle_micro.txt.
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(8, 1 << 14), (32, 1 << 14), (8, 1 << 17), (32, 1 << 17)]
ITERS, THR, FIXED = 10, 2.0, (0, 1)
CASE_TIMEOUT, SCIPY_TIMEOUT = 240, 420                       # seconds, per child
F = 800.0


def make_scene(V, N, seed=0):
    """-> x (V,N,2) fp32 with NaN where not seen, K (3,3), the true R, t, X and the start R0, t0, X0 (numpy)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    K = np.array([[F, 0.0, 512.0], [0.0, F, 384.0], [0.0, 0.0, 1.0]])
    R, t = [], []
    for v in range(V):
        a = 2 * np.pi * v / V
        C = 6.0 * np.array([np.sin(a), 0.1 * np.cos(3 * a), -np.cos(a)])
        z = -C / np.linalg.norm(C)
        xax = np.cross([0.0, 1.0, 0.0], z)
        xax /= np.linalg.norm(xax)
        Rv = np.stack([xax, np.cross(z, xax), z])
        R.append(Rv)
        t.append(-Rv @ C)
    R, t = np.stack(R), np.stack(t)
    d = rng.normal(size=(N, 3))
    X = 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.random((N, 1)) ** (1 / 3)
    first, length = rng.integers(0, V, N), np.full(N, 4)
    if V >= 32:
        length = length + rng.choice([-1, 0, 0, 0, 1], N)
    seen = ((np.arange(V)[:, None] - first[None, :]) % V) < length[None, :]
    q = np.einsum("vij,nj->vni", R, X) + t[:, None, :]
    px = np.stack([F * q[..., 0] / q[..., 2] + 512.0, F * q[..., 1] / q[..., 2] + 384.0], -1) + 0.5 * rng.normal(size=(V, N, 2))
    x = np.where(seen[..., None], px, np.nan).astype(np.float32)
    from tests.bundle_ref import exp_so3
    R0, t0 = R.copy(), t.copy()
    for v in range(2, V):
        R0[v] = exp_so3(np.radians(0.1) * np.sign(rng.normal(size=3))) @ R[v]
        u = rng.normal(size=3)
        t0[v] = t[v] + 0.01 * u / np.linalg.norm(u)
    C0 = -R[0].T @ t[0]
    X0 = C0 + (1 + 0.005 * rng.normal(size=(N, 1))) * (X - C0)
    return x, K, R, t, X, R0, t0, X0


def device_args(V, N):
    import torch
    x, K, _, _, _, R0, t0, X0 = make_scene(V, N)
    return [torch.tensor(a, device="cuda") for a in (x, R0, t0, K, X0)]


def run_case(V, N, reps):
    import numpy as np
    import torch
    from roma_amd import geometry
    args = device_args(V, N)

    def timed(iters):
        times = []
        for i in range(reps + 2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = geometry.bundle_adjust(*args, threshold=THR, iters=iters, fixed=FIXED)
            e.record()
            torch.cuda.synchronize()
            if i >= 2:
                times.append(s.elapsed_time(e))
        return float(np.median(times)), min(times), r

    full, full_min, r = timed(ITERS)
    none, _, _ = timed(0)
    need, _ = geometry.bundle_workspace_layout(V, N)
    obs = int(torch.isfinite(args[0][..., 0]).sum())
    print(f"V = {V:2d}, N = {N:6d} ({obs} observations, reduced system {6 * (V - 2)} x {6 * (V - 2)}, workspace {need / 2 ** 20:5.1f} MiB): "
          f"bundle_adjust(iters={ITERS}) {full:8.3f} ms (min {full_min:.3f}), iters=0 {none:6.3f} ms, per step {(full - none) / ITERS:7.3f} ms;  "
          f"{int(r.steps)} steps kept, cost {float(r.cost0):.0f} -> {float(r.cost):.0f}, status {int(r.status)}", flush=True)


def run_trace_child(V, N):
    import torch
    from roma_amd import geometry
    args = device_args(V, N)
    for _ in range(2):
        geometry.bundle_adjust(*args, threshold=THR, iters=ITERS, fixed=FIXED)
    torch.cuda.synchronize()


def trace(V, N):
    """the kernels of two calls from a rocprofv3 kernel trace of a child: average time per launch and the share of a step"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print("    rocprofv3 is not on this machine: no split by kernel", flush=True)
        return 0
    out = tempfile.mkdtemp(prefix="bundle_micro_")
    try:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT), prof, "--kernel-trace", "--stats", "-d", out, "-o", "bundle", "--output-format",
                             "csv", "--", sys.executable, os.path.abspath(__file__), "--trace", str(V), str(N)], stdout=subprocess.DEVNULL,
                            stderr=subprocess.DEVNULL).returncode
        if rc != 0:
            return rc
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("    the trace left no kernel_stats.csv: no split by kernel", flush=True)
            return 0
        rows = [r for r in csv.DictReader(open(files[0])) if "bundle_" in r["Name"]]
        step = ("accumulate", "reduce", "solve", "propose", "evaluate", "decide")
        avg = {n: float(r["AverageNs"]) / 1e3 for r in rows for n in step + ("init", "centre", "final") if f"bundle_{n}_kernel" in r["Name"]}
        total = sum(avg.get(n, 0.0) for n in step)
        print("    per launch, us: " + ", ".join(f"{n} {avg[n]:.1f}" for n in step + ("init", "centre", "final") if n in avg) +
              f";  one step {total:.1f} us of kernel time: " + ", ".join(f"{n} {100 * avg.get(n, 0.0) / total:.0f} %" for n in step), flush=True)
        return 0
    finally:
        shutil.rmtree(out, ignore_errors=True)


def run_scipy(V, N):
    """scipy.optimize.least_squares (trf, sparse finite-difference Jacobian) on the squared error of the observations that are inside the
    threshold at the start — the same cost as long as that set does not change — from the same start, views 0 and 1 held"""
    import numpy as np
    try:
        from scipy.optimize import least_squares
        from scipy.sparse import lil_matrix
    except ImportError:
        print("    scipy is not importable: no host yardstick was run", flush=True)
        return
    from tests import bundle_ref as B
    x, K, R, t, X, R0, t0, X0 = make_scene(V, N)
    xs = x.astype(np.float64)
    e = B.terms(np.broadcast_to(K, (V, 3, 3)), R0, t0, X0, xs)[0]
    with np.errstate(invalid="ignore"):
        vs, ns = np.nonzero(e < THR * THR)
    free = np.arange(2, V)

    def residuals(p):
        w, tt = p[:6 * len(free)].reshape(-1, 6), t0.copy()
        Rr = R0.copy()
        for i, v in enumerate(free):
            E = B.exp_so3(w[i, :3])
            Rr[v], tt[v] = E @ R0[v], E @ t0[v] + w[i, 3:]
        Xp = p[6 * len(free):].reshape(-1, 3)
        q = np.einsum("kij,kj->ki", Rr[vs], Xp[ns]) + tt[vs]
        return np.stack([F * q[:, 0] / q[:, 2] + 512.0 - xs[vs, ns, 0], F * q[:, 1] / q[:, 2] + 384.0 - xs[vs, ns, 1]], -1).reshape(-1)

    m, npar = len(vs), 6 * len(free) + 3 * N
    S = lil_matrix((2 * m, npar), dtype=np.int8)
    k = np.arange(m)
    for d in range(2):
        for j in range(3):
            S[2 * k + d, 6 * len(free) + 3 * ns + j] = 1
        sel = vs >= 2
        for j in range(6):
            S[2 * k[sel] + d, 6 * (vs[sel] - 2) + j] = 1
    p0 = np.concatenate([np.zeros(6 * len(free)), X0.reshape(-1)])
    c0 = float((residuals(p0) ** 2).sum())
    t1 = time.perf_counter()
    res = least_squares(residuals, p0, jac_sparsity=S, method="trf", x_scale="jac", max_nfev=ITERS)
    t2 = time.perf_counter()
    print(f"    host: scipy least_squares (trf, sparse 2-point Jacobian, max_nfev = {ITERS}) on the same {m} observations: {t2 - t1:.1f} s, "
          f"{res.nfev} evaluations, squared error {c0:.0f} -> {2 * res.cost:.0f}", flush=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] in ("--case", "--trace", "--scipy"):
        V, N = int(sys.argv[2]), int(sys.argv[3])
        if sys.argv[1] == "--case":
            run_case(V, N, int(sys.argv[4]) if len(sys.argv) > 4 else 5)
        elif sys.argv[1] == "--trace":
            run_trace_child(V, N)
        else:
            run_scipy(V, N)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    print(f"bundle_adjust: threshold {THR} px, views 0 and 1 held, {ITERS} steps; device events, median of {reps} calls after 2 warm-up calls",
          flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    for V, N in CASES:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT)] + me + ["--case", str(V), str(N), reps]).returncode
        if rc == 0:
            rc = trace(V, N)
        if rc != 0:
            print(f"case V = {V}, N = {N} ended with status {rc}; stopping here")
            sys.exit(rc)
    V, N = CASES[0]
    rc = subprocess.run(["timeout", "-k", "10", str(SCIPY_TIMEOUT)] + me + ["--scipy", str(V), str(N)]).returncode
    if rc != 0:
        print(f"the scipy yardstick ended with status {rc}")


if __name__ == "__main__":
    main()
