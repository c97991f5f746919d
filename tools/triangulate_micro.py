# roma_amd.geometry triangulation: time of one roma_triangulate call (all six outputs, no mask) against the same mathematics written
# as a composition of torch ops on the device, with device events after warm-up, the two alternating in one loop; median of `reps`.
# Cases: every match of one symmetric 864 x 1728 warp (P = 1), of eight (P = 8), and 10 000 sampled matches of 64 pairs.
# Bytes per call come from the shapes: 16 read + 12 + 4 * 4 + 1 written = 45 per match; the share is of the HBM peak.
# `triangulate_micro.py [reps]`; the committed output is profiles/triangulate_micro.txt.
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import _lib  # noqa: E402
from tests import geometry_ref as G  # noqa: E402
from tests import pose_ref as PR  # noqa: E402
from tests import triangulate_ref as T  # noqa: E402

HBM_PEAK = 8.0e12                                            # bytes/s, the MI355X specification (6.3e12 is what a float4 copy achieves)
CASES = [(1, 864 * 1728), (8, 864 * 1728), (64, 10000)]
BYTES_PER_MATCH = 16 + 12 + 4 * 4 + 1


def scene(P, N):
    """P scenes of N matches: the 5 000 of G.two_view_scene tiled (the kernel's time does not depend on the values)"""
    ms, Rs, ts = [], [], []
    for p in range(P):
        xa, xb = G.two_view_scene(100 + p, N=5000)[:2]
        m = np.concatenate([xa, xb], -1).astype(np.float32)
        ms.append(np.tile(m, (-(-N // 5000), 1))[:N])
        _, R, t = PR.scene_pose(100 + p)
        Rs.append(R), ts.append(t)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dev(np.stack(ms)), dev(np.stack([PR.K_SCENE] * P)), dev(np.stack(Rs)), dev(np.stack(ts))


def constants(K, R, t):
    """fp64 on the device -> fp32: F (P,3,3) unit Frobenius, K^-1, K, R, t"""
    Ki = torch.linalg.inv(K)
    tx = torch.zeros_like(R)
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    F = Ki.transpose(1, 2) @ tx @ R @ Ki
    F = F / torch.linalg.norm(F, dim=(1, 2), keepdim=True)
    return F.float(), Ki.float(), K.float(), R.float(), t.float()


def torch_triangulate(m, F, Ki, K, R, t, method):
    """tests/triangulate_ref.py in torch, fp32, (P,N,...) at once: points, depth_a, depth_b, reproj, cos_parallax, valid"""
    one = torch.ones_like(m[..., :1])
    xa, xb = torch.cat([m[..., :2], one], -1), torch.cat([m[..., 2:], one], -1)                 # (P,N,3)
    reproj = None
    if method == 0:
        Ft = F[:, :2, :2]
        nb, na = (xa @ F.transpose(1, 2))[..., :2], (xb @ F)[..., :2]
        c = (xb * (xa @ F.transpose(1, 2))).sum(-1)
        a = (nb * (na @ Ft.transpose(1, 2))).sum(-1)
        b = 0.5 * ((nb * nb).sum(-1) + (na * na).sum(-1))
        disc = b * b - a * c
        d = torch.sqrt(disc)
        den1 = b + d
        lam = c / den1
        da, db = lam[..., None] * na, lam[..., None] * nb
        nb, na = nb - da @ Ft.transpose(1, 2), na - db @ Ft
        den2 = (nb * nb).sum(-1) + (na * na).sum(-1)
        lam = lam * ((d + d) / den2)
        da, db = lam[..., None] * na, lam[..., None] * nb
        ok = (disc >= 0) & (den1 != 0) & (den2 != 0)
        xa, xb = torch.cat([xa[..., :2] - da, one], -1), torch.cat([xb[..., :2] - db, one], -1)
        reproj = torch.sqrt((da * da).sum(-1) + (db * db).sum(-1))
    ra, rb = xa @ Ki.transpose(1, 2), xb @ Ki.transpose(1, 2)
    q = ra @ R.transpose(1, 2)
    tt = t[:, None, :]
    aa, bb, ab = (q * q).sum(-1), (rb * rb).sum(-1), (q * rb).sum(-1)
    at, bt = (q * tt).sum(-1), (rb * tt).sum(-1)
    det = aa * bb - ab * ab
    la, lb = (ab * bt - bb * at) / det, (aa * bt - ab * at) / det
    cosp = ab / torch.sqrt(aa * bb)
    if method == 0:
        X, za, zb = la[..., None] * ra, la, lb
        fin = ok
    else:
        Xb = 0.5 * (la[..., None] * q + tt + lb[..., None] * rb)
        X = (Xb - tt) @ R
        za, zb = X[..., 2], Xb[..., 2]
        pa, pb = X @ K.transpose(1, 2), Xb @ K.transpose(1, 2)
        ea, eb = pa[..., :2] / pa[..., 2:] - m[..., :2], pb[..., :2] / pb[..., 2:] - m[..., 2:]
        reproj = torch.sqrt((ea * ea).sum(-1) + (eb * eb).sum(-1))
        fin = torch.ones_like(za, dtype=torch.bool)
    fin = fin & torch.isfinite(m).all(-1) & torch.isfinite(X).all(-1) & torch.isfinite(zb) & torch.isfinite(reproj) & torch.isfinite(cosp)
    z = torch.zeros((), device=m.device)
    valid = fin & (za > 0) & (zb > 0)
    return torch.where(fin[..., None], X, z), torch.where(fin, za, z), torch.where(fin, zb, z), torch.where(fin, reproj, z), torch.where(fin, cosp, z), valid


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = _lib.load()
    print(f"roma_triangulate against the torch composition, device events, median of {reps} alternating calls after 3 warm-up calls; "
          f"{BYTES_PER_MATCH} bytes per match; HBM peak {HBM_PEAK / 1e12:.1f} TB/s")
    for P, N in CASES:
        m, K, R, t = scene(P, N)
        consts = constants(K, R, t)
        f32 = dict(dtype=torch.float32, device=m.device)
        outs = [torch.empty((P, N, 3), **f32)] + [torch.empty((P, N), **f32) for _ in range(4)] + [torch.empty((P, N), dtype=torch.uint8, device=m.device)]
        for method, name in enumerate(T.METHODS):
            def kernel():
                _lib.check(lib.roma_triangulate(m.data_ptr(), None, K.data_ptr(), K.data_ptr(), R.data_ptr(), t.data_ptr(), None, P, N, method,
                                                math.inf, 1.0, *(o.data_ptr() for o in outs), torch.cuda.current_stream().cuda_stream),
                           "roma_triangulate")

            def composition():
                return torch_triangulate(m, *consts, method)

            for _ in range(3):
                kernel()
                ref = composition()
            torch.cuda.synchronize()
            # the two compute the same thing (fp32 both, other operation order)
            sel = ref[5] & (ref[4] <= math.cos(math.radians(2.0)))
            dz = float(((outs[1] - ref[1]).abs() / ref[1].abs())[sel].max())
            same = float((outs[5].bool() == ref[5]).float().mean())
            times = {"kernel": [], "torch": []}
            for _ in range(reps):
                for what, fn in (("kernel", kernel), ("torch", composition)):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    times[what].append(s.elapsed_time(e))
            del ref
            k, c = float(np.median(times["kernel"])), float(np.median(times["torch"]))
            nbytes = P * N * BYTES_PER_MATCH
            rate = nbytes / (k * 1e-3)
            print(f"{name:8s} P={P:2d} N={N:7d}: kernel {k:8.3f} ms (min {min(times['kernel']):.3f})  {nbytes / 1e6:8.1f} MB  {rate / 1e12:5.2f} TB/s = "
                  f"{100 * rate / HBM_PEAK:4.1f} % of peak;  torch composition {c:8.3f} ms (min {min(times['torch']):.3f}) = {c / k:5.1f} x the kernel;  "
                  f"depth_a agrees to {dz:.1e} relative where the parallax is >= 2 deg, valid on {100 * same:.3f} %")


if __name__ == "__main__":
    main()
