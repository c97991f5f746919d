# roma_amd.geometry.fuse_depth_maps: time of one call (wrapper and allocations included), the split by launch from a rocprofv3 kernel
# trace, and the same three passes written as torch ops on the device as the yardstick: per pair of views the projection, four index
# gathers and the bilinear blend in fp64, boolean masks, the ownership lookup, and `nonzero` for the cloud (which synchronises with the
# host, as it has to).  Device events after 2 warm-up calls, median of `reps` (default 5) calls.
# Shapes: V = 4, 8 and 32 views of 432 x 432 and 864 x 864.  The scene: tests/depth_scenes.py (a slanted plane behind a nearer rectangle,
# rendered by ray intersection, 0.3 % noise, 5 % wrong depths, 5 % holes; general motions of about 0.35 at depth 8, which is 18 or 36 px
# of disparity), default thresholds, max_points = a quarter of the pixels.
# `fuse_depth_micro.py [reps]` runs every case in child processes of their own under `timeout` (the kernel path, then the kernel trace,
# then the torch path), one after the other, and stops at the first that fails; `--case V S reps`, `--trace V S` and `--torch V S reps`
# are what a child runs.  The torch child also reports whether its masks and counts equal the kernel's.
# The committed output is profiles/fuse_depth_micro.txt.
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(4, 432), (8, 432), (32, 432), (4, 864), (8, 864), (32, 864)]
REPROJ, REL, MIN_VIEWS = 1.0, 0.01, 2
CASE_TIMEOUT = 300                                           # seconds, per child


def device_args(V, S):
    """-> depths (V,S,S) fp32, R, t, K fp64 on the device, max_points"""
    import numpy as np
    import torch
    from tests import depth_scenes as DS
    K, R, t = DS.cameras(V, 0, (S, S))
    rng = np.random.default_rng(5)
    maps = []
    for v in range(V):
        d, _ = DS.render(K[v], R[v], t[v], (S, S))
        d = d * (1.0 + DS.NOISE * rng.normal(size=d.shape))
        d = np.where(rng.random(d.shape) < DS.WRONG_FRAC, DS.WRONG_SCALE * d, d)
        maps.append(np.where(rng.random(d.shape) < DS.HOLE_FRAC, 0.0, d).astype(np.float32))
    return [torch.tensor(a, device="cuda") for a in (np.stack(maps), R, t, K)] + [V * S * S // 4]


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


def run_case(V, S, reps):
    from roma_amd import geometry
    depths, R, t, K, T = device_args(V, S)
    med, best, f = timed(lambda: geometry.fuse_depth_maps(depths, R, t, K, max_reproj_error=REPROJ, max_depth_error=REL, min_views=MIN_VIEWS,
                                                          max_points=T), reps)
    c = f.counts.tolist()
    pairs = V * (V - 1) * S * S
    print(f"V = {V:2d}, {S} x {S} ({pairs / 1e6:6.1f} M reprojections, workspace {geometry.depth_fuse_workspace(V, V * S * S) / 2 ** 20:5.1f} MiB): "
          f"fuse_depth_maps {med:9.3f} ms (min {best:.3f}), {pairs / med / 1e6:6.2f} G reprojections/s;  {c[1]} valid, {c[2]} duplicates, "
          f"{c[0]} emitted of max_points = {T}", flush=True)


def run_trace_child(V, S):
    import torch
    from roma_amd import geometry
    depths, R, t, K, T = device_args(V, S)
    for _ in range(2):
        geometry.fuse_depth_maps(depths, R, t, K, max_reproj_error=REPROJ, max_depth_error=REL, min_views=MIN_VIEWS, max_points=T)
    torch.cuda.synchronize()


def trace(V, S):
    """the kernels of two calls from a rocprofv3 kernel trace of a child: average time per launch and its share of the call"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print("    rocprofv3 is not on this machine: no split by launch", flush=True)
        return 0
    out = tempfile.mkdtemp(prefix="fuse_depth_micro_")
    try:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT), prof, "--kernel-trace", "--stats", "-d", out, "-o", "fuse", "--output-format",
                             "csv", "--", sys.executable, os.path.abspath(__file__), "--trace", str(V), str(S)], stdout=subprocess.DEVNULL,
                            stderr=subprocess.DEVNULL).returncode
        if rc != 0:
            return rc
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("    the trace left no kernel_stats.csv: no split by launch", flush=True)
            return 0
        names = ("consistency", "ownership", "scan", "clear", "cloud")
        avg = {n: float(r["AverageNs"]) / 1e3 for r in csv.DictReader(open(files[0])) for n in names if f"fuse_{n}_kernel" in r["Name"]}
        total = sum(avg.values())
        print("    per launch, us: " + ", ".join(f"{n} {avg[n]:.1f}" for n in names if n in avg) + f";  {total:.1f} us of kernel time: " +
              ", ".join(f"{n} {100 * avg[n] / total:.1f} %" for n in names if n in avg), flush=True)
        return 0
    finally:
        shutil.rmtree(out, ignore_errors=True)


def torch_fuse(depths, R, t, K, reproj, rel, min_views):
    """the three passes as torch ops, fp64 -> depth (V,H,W) fp32, valid, views (int64 bit patterns), points (n,3) fp32, view, pixel"""
    import torch
    V, H, W = depths.shape
    dev = depths.device
    d64 = depths.double()
    has = torch.isfinite(d64) & (d64 > 0)
    flat = torch.where(has, d64, torch.zeros_like(d64)).view(V, -1)
    hole = (~has).view(V, -1)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64) + 0.5, torch.arange(W, device=dev, dtype=torch.float64) + 0.5,
                          indexing="ij")
    pix = torch.stack([u, v, torch.ones_like(u)], -1).view(-1, 3)
    Kinv = torch.linalg.inv(K)

    def transfer(r, s, uvd):
        """pixels (n,3) = (u d, v d, d) of r -> q (n,3) in s"""
        X = (uvd @ Kinv[r].T - t[r]) @ R[r]
        return (X @ R[s].T + t[s]) @ K[s].T

    def project(r, s):
        q = transfer(r, s, pix * d64[r].view(-1, 1))
        return q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], q[:, 2]

    views = torch.zeros((V, H * W), dtype=torch.int64, device=dev)
    total = torch.zeros((V, H * W), dtype=torch.float64, device=dev)
    for r in range(V):
        views[r] = has[r].view(-1).long() << r
        total[r] = flat[r]
        for s in range(V):
            if s == r:
                continue
            us, vs, qz = project(r, s)
            ix, iy = us - 0.5, vs - 0.5
            inside = (qz > 0) & (ix >= 0) & (ix < W - 1) & (iy >= 0) & (iy < H - 1)
            fx, fy = torch.floor(ix), torch.floor(iy)
            at = (fy.clamp(0, H - 2) * W + fx.clamp(0, W - 2)).nan_to_num(0.0).long()
            wx, wy = ix - fx, iy - fy
            taps = [at, at + 1, at + W, at + W + 1]
            ds = flat[s][taps[0]] * ((1 - wx) * (1 - wy)) + flat[s][taps[1]] * (wx * (1 - wy)) + flat[s][taps[2]] * ((1 - wx) * wy) \
                + flat[s][taps[3]] * (wx * wy)
            full = ~(hole[s][taps[0]] | hole[s][taps[1]] | hole[s][taps[2]] | hole[s][taps[3]])
            p = transfer(s, r, torch.stack([us * ds, vs * ds, ds], -1))
            err = torch.hypot(p[:, 0] / p[:, 2] - pix[:, 0], p[:, 1] / p[:, 2] - pix[:, 1])
            good = has[r].view(-1) & inside & full & (p[:, 2] > 0) & (err < reproj) & ((p[:, 2] - flat[r]).abs() / flat[r] < rel)
            views[r] |= good.long() << s
            total[r] += torch.where(good, p[:, 2], torch.zeros_like(ds))
    num = torch.zeros_like(views)
    for b in range(V):
        num += (views >> b) & 1
    valid = num >= min_views
    depth = torch.where(valid, total / num.clamp(min=1), torch.zeros_like(total)).float()
    dup = torch.zeros_like(valid)
    for r in range(1, V):
        for s in range(r):
            us, vs, _ = project(r, s)
            seen = valid[r] & (((views[r] >> s) & 1) == 1)
            at = (torch.floor(vs).clamp(0, H - 1) * W + torch.floor(us).clamp(0, W - 1)).nan_to_num(0.0).long()
            dup[r] |= seen & valid[s][at] & (((views[s][at] >> r) & 1) == 1)
    emit = valid & ~dup
    idx = torch.nonzero(emit.view(-1)).view(-1)
    view, pixel = idx // (H * W), idx % (H * W)
    ray = (pix[pixel].unsqueeze(1) @ Kinv[view].transpose(1, 2)).squeeze(1) * depth.view(-1)[idx].double().unsqueeze(1)
    points = ((ray - t[view]).unsqueeze(1) @ R[view]).squeeze(1).float()
    return depth.view(V, H, W), valid.view(V, H, W), views.view(V, H, W), points, view, pixel


def run_torch(V, S, reps):
    import torch
    from roma_amd import geometry
    depths, R, t, K, T = device_args(V, S)
    med, best, out = timed(lambda: torch_fuse(depths, R, t, K, REPROJ, REL, MIN_VIEWS), reps)
    f = geometry.fuse_depth_maps(depths, R, t, K, max_reproj_error=REPROJ, max_depth_error=REL, min_views=MIN_VIEWS, max_points=T)
    k = min(int(f.counts[0]), T)
    same = bool(torch.equal(out[1], f.valid)) and bool(torch.equal(out[2].int(), f.views)) and int(f.counts[0]) == len(out[4]) and \
        bool(torch.equal(out[5][:k].int(), f.pixel[:k])) and bool(torch.equal(out[4][:k].to(torch.uint8), f.view[:k]))
    differ = int((out[1] != f.valid).sum()) + int((out[2].int() != f.views).sum())
    print(f"    torch ops (fp64, index gathers, masks, nonzero): {med:9.3f} ms (min {best:.3f});  masks, views and the cloud's order equal the "
          f"kernel's: {same}" + ("" if same else f" ({differ} pixels differ in valid or views)"), flush=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] in ("--case", "--trace", "--torch"):
        V, S = int(sys.argv[2]), int(sys.argv[3])
        reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
        if sys.argv[1] == "--case":
            run_case(V, S, reps)
        elif sys.argv[1] == "--trace":
            run_trace_child(V, S)
        else:
            run_torch(V, S, reps)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    print(f"fuse_depth_maps: max_reproj_error {REPROJ} px, max_depth_error {REL}, min_views {MIN_VIEWS}; device events, median of {reps} calls "
          "after 2 warm-up calls, wrapper and allocations included", flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    for V, S in CASES:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT)] + me + ["--case", str(V), str(S), reps]).returncode
        if rc == 0:
            rc = trace(V, S)
        if rc == 0:
            rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT)] + me + ["--torch", str(V), str(S), reps]).returncode
        if rc != 0:
            print(f"case V = {V}, {S} x {S} ended with status {rc}; stopping here")
            sys.exit(rc)


if __name__ == "__main__":
    main()
