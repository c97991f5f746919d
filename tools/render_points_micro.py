# roma_amd.geometry.render_points: time of one call (wrapper and allocations included), the split by launch from a rocprofv3 kernel
# trace collected in runs of its own, and the same passes written as torch ops on the device as the yardstick: per view the fp64
# projection, one scatter_reduce_("amin") of int64 keys per footprint offset, and the gathers for the maps and the visibility.
# Device events after 2 warm-up calls, median of `reps` (default 5) calls.
# The cloud: fuse_depth_maps on the V = 8 scene of tools/fuse_depth_micro.py at 864 x 864 (max_points = a quarter of the pixels), tail
# rows masked by pixel >= 0.  It is drawn into the first V = 1, 8 and 32 cameras of tests/depth_scenes.cameras(32, 0, (864, 864)) — the
# first 8 are the cameras the cloud came from — at radius 0, 1 and 2, once in the order fuse_depth_maps emits (view, row, column), in
# which the 64 atomics of a wave fall on neighbouring pixels of a row, and once randomly permuted, which scatters them.
# The torch yardstick forms P_v = K_v [R_v | t_v] and the projection with addcmul in the kernel's order of operations; whether its maps,
# indices, visibility and counts EQUAL the kernel's is printed for every timed case.
# `render_points_micro.py [reps]` runs the timing in one child process and each kernel trace in a child of its own, all under
# `timeout`, one after the other, and stops at the first that fails; `--time reps` and `--trace V radius order` are what a child runs.
# The committed output is profiles/render_points_micro.txt.
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, V_CLOUD = 864, 8
VIEWS, RADII, ORDERS = (1, 8, 32), (0, 1, 2), ("emitted", "permuted")
TRACES = [(8, 0), (8, 2)]                                    # (V, radius), both orders each
TOL = 0.05
CHILD_TIMEOUT = 420                                          # seconds


def device_cloud():
    """-> points (T,3) fp32, mask (T) bool, R, t, K (32, ...) fp64 on the device"""
    import torch
    from roma_amd import geometry
    from tests import depth_scenes as DS
    from tools.fuse_depth_micro import device_args
    depths, R, t, K, T = device_args(V_CLOUD, S)
    fused = geometry.fuse_depth_maps(depths, R, t, K, max_points=T)
    K32, R32, t32 = (torch.tensor(a, device="cuda") for a in DS.cameras(32, 0, (S, S)))
    assert torch.equal(K32[:V_CLOUD], K) and torch.equal(R32[:V_CLOUD], R) and torch.equal(t32[:V_CLOUD], t)
    return fused.points, fused.pixel >= 0, R32, t32, K32


def ordered(points, mask, order):
    import torch
    if order == "emitted":
        return points, mask
    g = torch.Generator(device="cpu").manual_seed(1)
    perm = torch.randperm(points.shape[0], generator=g).to(points.device)
    return points[perm].contiguous(), mask[perm].contiguous()


def timed(fn, reps):
    import numpy as np
    import torch
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


def torch_render(points, mask, R, t, K, shape, radius, tol):
    """the passes as torch ops -> depth (V,H,W) fp32, index (V,H,W) int32, visible (N) int32, counts (4) int64"""
    import torch
    H, W = shape
    V, N, dev = R.shape[0], points.shape[0], points.device
    X = points.double()
    live = torch.isfinite(X).all(1) & mask
    n = torch.arange(N, device=dev, dtype=torch.int64)
    far = torch.iinfo(torch.int64).max
    keys = torch.full((V, H * W), far, dtype=torch.int64, device=dev)
    Rt = torch.cat([R, t[:, :, None]], 2)                    # (V,3,4)
    P = torch.addcmul(torch.addcmul(K[:, :, 0:1] * Rt[:, 0:1], K[:, :, 1:2], Rt[:, 1:2]), K[:, :, 2:3], Rt[:, 2:3])
    kept, n_in = [], torch.zeros((), dtype=torch.int64, device=dev)
    for v in range(V):
        q = [torch.addcmul(torch.addcmul(torch.addcmul(P[v, i, 3], X[:, 0], P[v, i, 0]), X[:, 1], P[v, i, 1]), X[:, 2], P[v, i, 2])
             for i in range(3)]
        iz = 1.0 / q[2]
        u, w, zf = q[0] * iz, q[1] * iz, q[2].float()
        ok = live & torch.isfinite(q[0]) & torch.isfinite(q[1]) & torch.isfinite(q[2]) & (q[2] > 0) & (u >= 0) & (u < W) & (w >= 0) & (w < H) \
            & torch.isfinite(zf) & (zf > 0)
        col, row = torch.floor(u).nan_to_num(0.0).clamp(0, W - 1).long(), torch.floor(w).nan_to_num(0.0).clamp(0, H - 1).long()
        key = (zf.view(torch.int32).long() << 32) | n
        for di in range(-radius, radius + 1):
            for dj in range(-radius, radius + 1):
                ii, jj = row + di, col + dj
                on = ok & (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                keys[v].scatter_reduce_(0, torch.where(on, ii * W + jj, torch.zeros_like(ii)), torch.where(on, key, torch.full_like(key, far)),
                                        "amin")
        kept.append((ok, row * W + col, zf))
        n_in += ok.sum()
    covered = keys != far
    depth = torch.where(covered, (keys >> 32).int().view(torch.float32), torch.zeros((), device=dev))
    index = torch.where(covered, keys & 0xFFFFFFFF, torch.full_like(keys, -1)).int()
    visible = torch.zeros(N, dtype=torch.int64, device=dev)
    for v, (ok, at, zf) in enumerate(kept):
        see = ok & (zf.double() <= depth[v][at].double() * (1.0 + tol))
        visible |= see.long() << v
    bits = sum(((visible >> b) & 1) for b in range(V))
    counts = torch.stack([n_in, covered.sum(), bits.sum(), (~live).sum()])
    visible = torch.where(visible >= 1 << 31, visible - (1 << 32), visible).int()
    return depth.view(V, H, W), index.view(V, H, W), visible, counts


def run_time(reps):
    import torch
    from roma_amd import geometry
    points, mask, R, t, K = device_cloud()
    N, live = points.shape[0], int(mask.sum())
    print(f"cloud: {live} fused points in {N} rows (fuse_depth_maps, V = {V_CLOUD}, {S} x {S}); maps of {S} x {S}, depth_tol {TOL}", flush=True)
    print("  V  radius  order     kernels ms (min)    torch ms (min)     ratio  equal   inside   covered      bits  footprint pixels", flush=True)
    for V in VIEWS:
        for radius in RADII:
            for order in ORDERS:
                p, m = ordered(points, mask, order)
                med, best, out = timed(lambda: geometry.render_points(p, R[:V], t[:V], K[:V], (S, S), radius=radius, depth_tol=TOL, mask=m), reps)
                tmed, tbest, ref = timed(lambda: torch_render(p, m, R[:V], t[:V], K[:V], (S, S), radius, TOL), reps)
                diff = [int((a != b).sum()) for a, b in ((out.depth, ref[0]), (out.index, ref[1]), (out.visible, ref[2]),
                                                         (out.counts.long(), ref[3]))]
                c = out.counts.tolist()
                same = "yes" if not any(diff) else "NO " + str(diff)
                print(f" {V:2d}  {radius:6d}  {order:8s}  {med:8.3f} ({best:7.3f})  {tmed:9.3f} ({tbest:8.3f})  {tmed / med:7.1f}x  {same:5s} "
                      f"{c[0]:9d} {c[1]:9d} {c[2]:9d}  {c[0] * (2 * radius + 1) ** 2 / 1e6:8.1f} M", flush=True)
                del out, ref
                torch.cuda.empty_cache()


def run_trace_child(V, radius, order):
    import torch
    from roma_amd import geometry
    points, mask, R, t, K = device_cloud()
    p, m = ordered(points, mask, order)
    for _ in range(3):
        out = geometry.render_points(p, R[:V], t[:V], K[:V], (S, S), radius=radius, depth_tol=TOL, mask=m)
    torch.cuda.synchronize()
    print(int(out.counts[0]))


def trace(V, radius, order):
    """the kernels of three calls from a rocprofv3 kernel trace of a child: average time per launch and its share of the call"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print("    rocprofv3 is not on this machine: no split by launch", flush=True)
        return 0
    out = tempfile.mkdtemp(prefix="render_points_micro_")
    try:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), prof, "--kernel-trace", "--stats", "-d", out, "-o", "render",
                            "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--trace", str(V), str(radius), order],
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        if r.returncode != 0:
            return r.returncode
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("    the trace left no kernel_stats.csv: no split by launch", flush=True)
            return 0
        names = ("clear", "splat", "resolve", "visible")
        avg = {n: float(row["AverageNs"]) / 1e3 for row in csv.DictReader(open(files[0])) for n in names if f"render_{n}_kernel" in row["Name"]}
        total = sum(avg.values())
        line = f"  V = {V}, radius {radius}, {order}: per launch, us: " + ", ".join(f"{n} {avg[n]:.1f}" for n in names if n in avg) + \
            f";  {total:.1f} us of kernel time"
        digits = [w for w in r.stdout.split() if w.isdigit()]
        if digits and "splat" in avg:
            tests = int(digits[-1]) * (2 * radius + 1) ** 2
            line += f";  splat: {tests / 1e6:.1f} M footprint pixels (load, compare, atomic min where nearer), {tests / avg['splat'] / 1e3:.2f} G/s"
        print(line, flush=True)
        return 0
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        run_time(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
        return
    if len(sys.argv) > 4 and sys.argv[1] == "--trace":
        run_trace_child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    print(f"render_points: device events, median of {reps} calls after 2 warm-up calls, wrapper and allocations included; `torch` is the same "
          "passes as torch ops", flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT)] + me + ["--time", reps]).returncode
    if rc != 0:
        print(f"the timing child ended with status {rc}; stopping here")
        sys.exit(rc)
    print("split by launch (rocprofv3 --kernel-trace --stats, a run of its own per line, average of three calls):", flush=True)
    for V, radius in TRACES:
        for order in ORDERS:
            rc = trace(V, radius, order)
            if rc != 0:
                print(f"the trace of V = {V}, radius {radius}, {order} ended with status {rc}; stopping here")
                sys.exit(rc)


if __name__ == "__main__":
    main()
