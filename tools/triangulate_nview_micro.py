# roma_amd.geometry N-view triangulation: time of one roma_triangulate_nview call (all six outputs) against (b) the same mathematics
# written as a composition of torch ops on the device and (c), for the dense cases, k calls of depth_from_warp on the same warps — the
# yardstick: the same observation bytes through a kernel known to run near its traffic (it triangulates both halves of each symmetric
# warp, 2 W columns, where the new call reads the A half only).  Device events after 3 warm-up calls, median of `reps` (default 20).
# Cases: every pixel of an 864 x 864 image against k = 2, 4, 8 symmetric 864 x 1728 warps (V = k + 1 views, read in place), and
# N = 10 000 packed tracks with V = 4 and 32; each robust (max_view_error = 3 px) and not.  The bytes per call are the least traffic:
# one read per observation (8 bytes) and per visibility byte, one write per output (12 + 4 * 4 + 1 = 29 bytes per point).
# `triangulate_nview_micro.py [reps]` runs every case in a child process of its own under `timeout`, one after the other, and stops
# at the first that fails; `--case i [reps]` is what a child runs.  The committed output is profiles/triangulate_nview_micro.txt.
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                                            # bytes/s, the MI355X specification
THR = 3.0
H = W = 864
CASES = [("dense", 2), ("dense", 4), ("dense", 8), ("tracks", 4), ("tracks", 32)]
CASE_TIMEOUT = 300                                           # seconds, per child


def view_constants(K, R, t):
    """fp64 on the device -> fp32: K (V,3,3), K^-1, R, C' = C - c0 (V,3), t' = t + R c0 (V,3); c0 fp64"""
    import torch
    C = -(R.transpose(1, 2) @ t[..., None])[..., 0]
    c0 = C.mean(0)
    return K.float(), torch.linalg.inv(K).float(), R.float(), (C - c0).float(), (t + R @ c0).float(), c0


def _solve_sym3(a00, a01, a02, a11, a12, a22, b0, b1, b2):
    import torch
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    return torch.stack([(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det, (c02 * b0 + c12 * b1 + c22 * b2) / det], -1)


def torch_nview(x, vis, consts, thr, iters=3):
    """tests/triangulate_nview_ref.py in torch, fp32, the views batched: x (V,N,2) pixels, vis (V,N) bool or None -> points, depth
    (view 0), reproj, cos_parallax, views, valid"""
    import torch
    K, Ki, R, C, tp, c0 = consts
    V, N = x.shape[:2]
    obs = torch.isfinite(x).all(-1)
    if vis is not None:
        obs = obs & vis
    x = torch.where(obs[..., None], x, torch.zeros((), device=x.device))
    xh = torch.cat([x, torch.ones_like(x[..., :1])], -1)
    d = torch.nn.functional.normalize((xh @ Ki.transpose(1, 2)) @ R, dim=-1)                # R^T K^-1 x~ as row vectors

    def project(X):
        """X (N,3) -> q (V,N,3), residual (V,N,2)"""
        q = X[None] @ R.transpose(1, 2) + tp[:, None]
        p = q @ K.transpose(1, 2)
        return q, p[..., :2] / p[..., 2:] - x

    member = obs
    if thr is not None:
        thr2 = thr * thr
        best = torch.full((N,), math.inf, device=x.device)
        member = torch.zeros_like(obs)
        for a in range(V - 1):
            for b in range(a + 1, V):
                w = (C[a] - C[b])[None]
                ab, aw, bw = (d[a] * d[b]).sum(-1), (d[a] * w).sum(-1), (d[b] * w).sum(-1)
                den = 1 - ab * ab
                sa, sb = (ab * bw - aw) / den, (bw - ab * aw) / den
                M = 0.5 * ((C[a] + sa[:, None] * d[a]) + (C[b] + sb[:, None] * d[b]))
                q, r = project(M)
                e2 = (r * r).sum(-1)
                inl = obs & (q[..., 2] > 0) & (e2 <= thr2)
                score = torch.where(obs, torch.where(inl, e2, thr2), 0.0).sum(0)
                better = inl[a] & inl[b] & (score < best)
                best = torch.where(better, score, best)
                member = torch.where(better[None], inl, member)
    m = member.float()
    nset = member.sum(0)
    dc = (d * C[:, None]).sum(-1)
    eye = torch.eye(3, device=x.device)
    A = (m[..., None, None] * (eye - d[..., :, None] * d[..., None, :])).sum(0)
    rhs = (m[..., None] * (C[:, None] - d * dc[..., None])).sum(0)
    X = _solve_sym3(A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2], rhs[:, 0], rhs[:, 1], rhs[:, 2])

    def evaluate(X):
        q, r = project(X)
        iz = 1 / q[..., 2]
        fx, s, fy = K[:, 0, 0, None], K[:, 0, 1, None], K[:, 1, 1, None]
        zero = torch.zeros_like(iz)
        ju = torch.stack([fx * iz, s * iz, -(fx * q[..., 0] + s * q[..., 1]) * iz * iz], -1)[..., None, :] @ R[:, None]
        jv = torch.stack([zero, fy * iz, -(fy * q[..., 1]) * iz * iz], -1)[..., None, :] @ R[:, None]
        J = torch.cat([ju, jv], -2)                                                       # (V,N,2,3)
        w = m[..., None, None]
        cost = (m * (r * r).sum(-1)).sum(0)
        return cost, (w * (J.transpose(-1, -2) @ J)).sum(0), (w * (J.transpose(-1, -2) @ r[..., None])).sum(0)[..., 0], q

    cost, Hm, g, q = evaluate(X)
    lam = torch.full((N,), 1e-3, device=x.device)
    for _ in range(iters):
        step = _solve_sym3(Hm[:, 0, 0] * (1 + lam), Hm[:, 0, 1], Hm[:, 0, 2], Hm[:, 1, 1] * (1 + lam), Hm[:, 1, 2], Hm[:, 2, 2] * (1 + lam),
                           g[:, 0], g[:, 1], g[:, 2])
        Xn = X - step
        cn, Hn, gn, qn = evaluate(Xn)
        keep = cn < cost
        X, cost = torch.where(keep[:, None], Xn, X), torch.where(keep, cn, cost)
        Hm, g, q = torch.where(keep[:, None, None], Hn, Hm), torch.where(keep[:, None], gn, g), torch.where(keep[None, :, None], qn, q)
        lam = torch.where(keep, lam * 0.1, lam * 10)
    reproj = torch.sqrt(cost / nset)
    minz = torch.where(member, q[..., 2], math.inf).min(0).values
    rays = torch.nn.functional.normalize(C[:, None] - X[None], dim=-1)
    cosp = torch.full((N,), 2.0, device=x.device)
    for a in range(V - 1):
        dots = (rays[a][None] * rays[a + 1:]).sum(-1)
        cosp = torch.minimum(cosp, torch.where(member[a][None] & member[a + 1:], dots, 2.0).min(0).values)
    P = (X.double() + c0).float()
    fin = (nset >= 2) & torch.isfinite(P).all(-1) & torch.isfinite(reproj) & torch.isfinite(minz) & (cosp <= 1.5)
    views = (member.int() << torch.arange(V, device=x.device, dtype=torch.int32)[:, None]).sum(0).int()
    z = torch.zeros((), device=x.device)
    return (torch.where(fin[:, None], P, z), torch.where(fin, q[0, :, 2], z), torch.where(fin, reproj, z), torch.where(fin, cosp, z),
            torch.where(fin, views, 0), fin & (minz > 0))


def dense_case(k):
    """k symmetric warps (H,2W,4) of one depth map of A against the cameras 1 .. k of tests/multiview_scenes.py, 10 % wrong rows in
    each, certainties uniform in [0, 1]"""
    import numpy as np
    import torch
    from tests import multiview_scenes as MS
    Kn, Rn, tn, sizes = MS.cameras(k + 1, 0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    K, R, t = dev(Kn), dev(Rn), dev(tn)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gx, gy = torch.linspace(-1 + 1 / W, 1 - 1 / W, W, device="cuda", dtype=torch.float64), torch.linspace(-1 + 1 / H, 1 - 1 / H, H, device="cuda", dtype=torch.float64)
    g = torch.stack(torch.meshgrid(gx, gy, indexing="xy"), -1)
    HA, WA = int(sizes[0, 1]), int(sizes[0, 0])
    pa = torch.stack([WA / 2 * (g[..., 0] + 1), HA / 2 * (g[..., 1] + 1), torch.ones_like(g[..., 0])], -1)
    depth = 4 + 8 * torch.rand((H, W), generator=gen, device="cuda", dtype=torch.float64)
    X = (pa @ torch.linalg.inv(K[0]).T) * depth[..., None]
    warps, certs = [], []
    for v in range(1, k + 1):
        p = (X @ R[v].T + t[v]) @ K[v].T
        pb = p[..., :2] / p[..., 2:] + 0.5 * torch.randn((H, W, 2), generator=gen, device="cuda", dtype=torch.float64)
        nb = torch.stack([2 / sizes[v, 0] * pb[..., 0] - 1, 2 / sizes[v, 1] * pb[..., 1] - 1], -1)
        wrong = torch.rand((H, W), generator=gen, device="cuda") < 0.1
        nb = torch.where(wrong[..., None], 2 * torch.rand((H, W, 2), generator=gen, device="cuda", dtype=torch.float64) - 1, nb)
        left = torch.cat([g, nb], -1)
        warps.append(torch.cat([left, left.flip(-1)], 1).float().contiguous())             # the right half: [x_A, grid_B]-shaped filler
        certs.append(torch.rand((H, 2 * W), generator=gen, device="cuda"))
    return warps, certs, depth, K, R, t, [(int(sizes[v, 1]), int(sizes[v, 0])) for v in range(k + 1)]


def timed(fns, reps):
    """{name: median ms, min ms} of callables alternating in one loop, after 3 warm-up rounds"""
    import numpy as np
    import torch
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    return {name: (float(np.median(v)), float(min(v))) for name, v in times.items()}


def run_case(index, reps):
    import ctypes
    import numpy as np
    import torch
    from roma_amd import _lib, geometry
    from tests import multiview_scenes as MS
    kind, n = CASES[index]
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "dense":
        k, V, N = n, n + 1, H * W
        warps, certs, depth, K, R, t, sizes = dense_case(k)
        keep = [(c[:, :W] > 0.05).to(torch.uint8).contiguous() for c in certs]
        obs = [warps[0].data_ptr()] + [w.data_ptr() + 8 for w in warps]
        vis = [None] + [v.data_ptr() for v in keep]
        px = [(s[1] / 2, s[1] / 2, s[0] / 2, s[0] / 2) for s in sizes]
        layout = (H, W, 8 * W, 4, W)
        vis_bytes = k
        xs = torch.stack([torch.stack([w[:, :W, 2 * (v > 0)] * px[v][0] + px[v][1], w[:, :W, 2 * (v > 0) + 1] * px[v][2] + px[v][3]], -1)
                          for v, w in enumerate([warps[0]] + warps)]).reshape(V, N, 2).contiguous()
        vs = torch.stack([torch.ones((H, W), dtype=torch.bool, device="cuda")] + [v.bool() for v in keep]).reshape(V, N)
        what = f"dense {H} x {W}, k = {k} warps (V = {V})"
    else:
        V, N = n, 10000
        s = MS.multiview_scene(V, 0, N=N)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        xs, K, R, t = dev(s["x"]), dev(s["K"]), dev(s["R"]), dev(s["t"])
        obs, vis, px, layout, vis_bytes, vs = [xs.data_ptr() + 8 * N * v for v in range(V)], None, None, (1, N, 0, 2, 0), 0, None
        what = f"tracks N = {N}, V = {V}"
    consts = view_constants(K, R, t)
    f32 = dict(dtype=torch.float32, device="cuda")
    outs = [torch.empty((N, 3), **f32)] + [torch.empty((N,), **f32) for _ in range(3)] + [torch.empty((N,), dtype=torch.int32, device="cuda"),
                                                                                         torch.empty((N,), dtype=torch.uint8, device="cuda")]
    obs_tab = (ctypes.c_void_p * V)(*obs)
    vis_tab = None if vis is None else (ctypes.c_void_p * V)(*vis)
    px_tab = None if px is None else (ctypes.c_float * (4 * V))(*[float(v) for row in px for v in row])
    nbytes = N * (8 * V + vis_bytes + 29)
    print(f"{what}: {nbytes / 1e6:.1f} MB of least traffic per call; device events, median of {reps} after 3 warm-up calls")
    for robust in (False, True):
        mve = THR if robust else math.inf

        def kernel():
            _lib.check(lib.roma_triangulate_nview(ctypes.cast(obs_tab, ctypes.c_void_p), None if px_tab is None else ctypes.cast(px_tab, ctypes.c_void_p),
                                                  None if vis_tab is None else ctypes.cast(vis_tab, ctypes.c_void_p), layout[4], K.data_ptr(),
                                                  R.data_ptr(), t.data_ptr(), V, layout[0], layout[1], layout[2], layout[3], mve, 3, 2, 0, math.inf,
                                                  1.0, *(o.data_ptr() for o in outs), stream), "roma_triangulate_nview")

        fns = {"kernel": kernel, "torch": lambda: torch_nview(xs, vs, consts, THR if robust else None)}
        if kind == "dense" and not robust:
            fns["two_view"] = lambda: [geometry.depth_from_warp(warps[i], certs[i], R[i + 1], t[i + 1], K[0], K[i + 1], sizes[0][0], sizes[0][1],
                                                                sizes[i + 1][0], sizes[i + 1][1]) for i in range(k)]
        res = timed(fns, reps)
        ref = torch_nview(xs, vs, consts, THR if robust else None)
        torch.cuda.synchronize()
        same = outs[4] == ref[4]
        sel = same & ref[5] & outs[5].bool() & (ref[3] <= math.cos(math.radians(2.0)))
        dz = float(((outs[1] - ref[1]).abs() / ref[1].abs())[sel].max())
        km, kmin = res["kernel"]
        rate = nbytes / (km * 1e-3)
        line = (f"  {'robust' if robust else 'all views':9s}: kernel {km:8.3f} ms (min {kmin:.3f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of "
                f"peak;  torch composition {res['torch'][0]:9.3f} ms = {res['torch'][0] / km:6.1f} x the kernel")
        if "two_view" in res:
            line += f";  {k} x depth_from_warp {res['two_view'][0]:7.3f} ms = {res['two_view'][0] / km:5.2f} x the kernel"
        print(line + f";  views agree with the composition on {100 * float(same.float().mean()):.3f} %, depth to {dz:.1e} relative there (parallax >= 2 deg)")
        if kind == "dense" and robust:
            dA = torch.where(outs[5].bool(), outs[1], 0.0).reshape(H, W)
            ok = outs[5].bool().reshape(H, W)
            two = geometry.depth_from_warp(warps[0], certs[0], R[1], t[1], K[0], K[1], sizes[0][0], sizes[0][1], sizes[1][0], sizes[1][1],
                                           max_reproj_error=2.0)
            e_all = float((dA / depth.float() - 1).abs()[ok].median())
            e_two = float((two.depth_A / depth.float() - 1).abs()[two.valid_A].median())
            print(f"             median relative depth error {e_all:.5f} over {100 * float(ok.float().mean()):.1f} % of the pixels; depth_from_warp on the "
                  f"first warp alone (max_reproj_error 2 px) {e_two:.5f} over {100 * float(two.valid_A.float().mean()):.1f} %")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        run_case(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 20)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "20"
    print(f"roma_triangulate_nview against the torch composition and against k two-view calls; HBM peak {HBM_PEAK / 1e12:.1f} TB/s", flush=True)
    for i in range(len(CASES)):
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT), sys.executable, os.path.abspath(__file__), "--case", str(i), reps]).returncode
        if rc != 0:
            print(f"case {i} {CASES[i]} ended with status {rc}; stopping here")
            sys.exit(rc)


if __name__ == "__main__":
    main()
