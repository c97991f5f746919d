# roma_amd.geometry dense_match_metrics and get_gt_warp (csrc/depth_warp.hip): time of one call against the same mathematics written as
# a composition of torch ops in fp64 on the device (the reference's warp_kpts / geometric_dist line for line: two grid_sample calls and
# a dozen full-size temporaries), the two alternating in one loop.  Each timed window is `inner` calls between two device events after
# warm-up; the figure is the median over `reps` windows of the time per call.
# Cases: 8 x 384 x 512 — a batch of the dense MegaDepth benchmark — and 1 x 864 x 1152.  The scene is that of tests/depth_warp_ref.py;
# the predicted warp is the ground truth + N(0, 2 px).
# The time is that of the CALL: the Python wrapper, its allocations and every launch behind it (get_gt_warp also builds its grid with
# torch ops), on both sides.  It is no kernel time and no bandwidth is derived from it; the bytes printed are what the algorithm has
# to move by the shapes, each depth map counted once (dense_match_metrics reads 16 per pixel, get_gt_warp reads 8 and writes 17).  The
# kernels alone: `rocprofv3 --kernel-trace --stats -- python tools/depth_warp_micro.py 2 10 <case>`, profiles/depth_warp_kernel_stats.txt.
# `depth_warp_micro.py [reps [inner [case]]]`, case 0 or 1 to run one shape only; the committed output is profiles/depth_warp_micro.txt.
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import geometry  # noqa: E402
from tests import depth_warp_ref as D  # noqa: E402

CASES = [(8, 384, 512), (1, 864, 1152)]
THRESHOLD = 0.05


def scene(P, H, W, device):
    """P pairs of the two-plane scene at H x W in both cameras: depth_A, depth_B fp32, T, K_A, K_B fp64 on the device"""
    pairs = [D.scene(200 + p, H, W, H, W, variant=p % 3) for p in range(P)]
    dev = lambda k: torch.from_numpy(np.stack([q[k] for q in pairs])).to(device)  # noqa: E731
    return dev("depth_A"), dev("depth_B"), dev("T"), dev("K_A"), dev("K_B")


def torch_warp_kpts(k, dA, dB, T, KA, KB):
    """warp_kpts as torch ops, fp64: k (P,N,2) -> valid (P,N), x2 (P,N,2).  No host synchronisation (inv_ex)."""
    k, dA, dB = k.double(), dA.double(), dB.double()
    Ha, Wa = dA.shape[1:]
    Hb, Wb = dB.shape[1:]
    d = F.grid_sample(dA[:, None], k[:, :, None], mode="bilinear", align_corners=False)[:, 0, :, 0]
    px = torch.stack((Wa * (k[..., 0] + 1) / 2, Ha * (k[..., 1] + 1) / 2), dim=-1)
    h = torch.cat([px, torch.ones_like(px[:, :, [0]])], dim=-1) * d[..., None]
    XA = torch.linalg.inv_ex(KA)[0] @ h.transpose(2, 1)
    XB = T[:, :3, :3] @ XA + T[:, :3, [3]]
    z = XB[:, 2, :]
    ph = (KB @ XB).transpose(2, 1)
    uv = ph[:, :, :2] / (ph[:, :, [2]] + 1e-4)
    covisible = (uv[:, :, 0] > 0) * (uv[:, :, 0] < Wb - 1) * (uv[:, :, 1] > 0) * (uv[:, :, 1] < Hb - 1)
    x2 = torch.stack((2 * uv[..., 0] / Wb - 1, 2 * uv[..., 1] / Hb - 1), dim=-1)
    d2 = F.grid_sample(dB[:, None], x2[:, :, None], mode="bilinear", align_corners=False)[:, 0, :, 0]
    rel = ((d2 - z) / d2).abs()
    return (d != 0) * covisible * (rel < THRESHOLD), x2


def torch_gt_warp(dA, dB, T, KA, KB):
    P, H, W = dA.shape
    mask, x2 = torch_warp_kpts(geometry.gt_warp_grid(P, H, W, dA.device), dA, dB, T, KA, KB)
    return x2.reshape(P, H, W, 2), mask.float().reshape(P, H, W)


def torch_metrics(warp, dA, dB, T, KA, KB):
    """geometric_dist as torch ops with per-pair sums instead of the boolean selection: epe_sum (P,), counts (P,4)"""
    P, H, W, _ = warp.shape
    mask, x2 = torch_warp_kpts(warp[..., :2].reshape(P, H * W, 2), dA, dB, T, KA, KB)
    x2 = torch.stack((W * (x2[..., 0] + 1) / 2, H * (x2[..., 1] + 1) / 2), dim=-1)
    hat = warp[..., 2:]
    hat = torch.stack((W * (hat[..., 0] + 1) / 2, H * (hat[..., 1] + 1) / 2), dim=-1).reshape(P, H * W, 2)
    gd = (hat - x2).norm(dim=-1)
    counts = torch.stack([mask.sum(1)] + [(mask & (gd < r)).sum(1) for r in (1.0, 3.0, 5.0)], -1)
    return torch.where(mask, gd, 0.0).sum(1), counts


def timed(fns, reps, inner):
    """{name: [ms per call, one per window]}: the functions alternate, each window is `inner` calls between two events"""
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / inner)
    return times


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    inner = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    cases = CASES if len(sys.argv) <= 3 else [CASES[int(sys.argv[3])]]
    if not torch.cuda.is_available():
        raise SystemExit("depth_warp_micro.py measures on the device; there is none")
    dev = "cuda:0"
    print(f"csrc/depth_warp.hip against the torch composition in fp64: time per CALL (wrapper, allocations and launches included), device "
          f"events, median over {reps} windows of {inner} calls, alternating, after 3 warm-up calls")
    for P, H, W in cases:
        dA, dB, T, KA, KB = scene(P, H, W, dev)
        gt, prob = geometry.get_gt_warp(dA, dB, T, KA, KB)
        noise = torch.randn(gt.shape, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(P)) * 2.0
        noise = noise * torch.tensor([2 / W, 2 / H], dtype=torch.float64, device=dev)
        warp = torch.cat([geometry.gt_warp_grid(P, H, W, dev).reshape(P, H, W, 2), torch.nan_to_num(gt + noise, nan=0.0, posinf=0.0, neginf=0.0).float()], -1)
        maps = 4 * P * (dA[0].numel() + dB[0].numel())
        for what, kernel, composition, per_pixel in (
                ("dense_match_metrics", lambda: geometry.dense_match_metrics(warp, dA, dB, T, KA, KB), lambda: torch_metrics(warp, dA, dB, T, KA, KB), 16),
                ("get_gt_warp", lambda: geometry.get_gt_warp(dA, dB, T, KA, KB), lambda: torch_gt_warp(dA, dB, T, KA, KB), 8 + 17)):
            for _ in range(3):
                k, c = kernel(), composition()
            torch.cuda.synchronize()
            if what == "dense_match_metrics":
                ck = torch.stack([k.n_valid, k.n_pck_1, k.n_pck_3, k.n_pck_5], -1)
                agree = (f"counts differ at {int((ck != c[1]).sum())} of {ck.numel()} (largest difference {int((ck - c[1]).abs().max())} of "
                         f"{int(ck[:, 0].min())} valid pixels), epe_sum to {float((k.epe_sum / c[0] - 1).abs().max()):.1e} relative; epe {float(k.epe):.4f} px, "
                         f"pck {float(k.pck_1):.4f} {float(k.pck_3):.4f} {float(k.pck_5):.4f}")
            else:
                same = k[1] == c[1]
                agree = (f"prob differs at {int((~same).sum())} of {same.numel()} pixels, x2 to {float((k[0] - c[0]).abs()[k[1] == 1].max()):.1e} where valid; "
                         f"{float(k[1].mean()):.3f} valid")
            del k, c
            t = timed({"kernel": kernel, "torch": composition}, reps, inner)
            tk, tc = float(np.median(t["kernel"])), float(np.median(t["torch"]))
            nbytes = P * H * W * per_pixel + maps
            print(f"{what:20s} {P} x {H} x {W}: device path {tk:7.3f} ms per call (min {min(t['kernel']):.3f}, max {max(t['kernel']):.3f}), {nbytes / 1e6:5.1f} MB "
                  f"to move;  torch composition {tc:8.3f} ms (min {min(t['torch']):.3f}, max {max(t['torch']):.3f}) = {tc / tk:5.1f} x;  {agree}")


if __name__ == "__main__":
    main()
