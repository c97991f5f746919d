# Old against new for everything that feeds the nine ConvRefiners of one 560 -> 864 step (B = 2, fp16): the two skinny projections
# (GEMM library vs ops.project_skinny), the input assembly (zero_ + ops.warp_bilinear + ops.disp_emb vs ops.refiner_assemble) and the
# flow / certainty upsample (two ops.interp_bilinear vs ops.interp_bilinear_pair).  python tools/refiner_inputs_micro.py [iters]
# Bytes are the algorithmic ones: projection = rows in + N columns out; assembly = flow + (C + E + padding) channels out + C in.
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import ops
from roma_amd.matcher import padded_width

torch.set_grad_enabled(False)
DEV, B, DT = "cuda", 2, torch.float16
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
# scale -> (C, E, local-correlation channels), and the map sizes of the coarse (560) and the upsample (864) pass
LEVEL = {16: (512, 128, 225), 8: (512, 64, 49), 4: (256, 32, 25), 2: (64, 16, 0), 1: (9, 6, 0)}
MAPS = [(16, 40), (8, 70), (4, 140), (2, 280), (1, 560), (8, 108), (4, 216), (2, 432), (1, 864)]
PROJ = {2: (128, 64), 1: (64, 9)}


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e-3


def line(what, shape, nbytes, t_old, t_new):
    print(f"{what:10s} {shape:28s} {nbytes / 1e6:7.1f} MB   old {t_old * 1e6:7.1f} us {nbytes / t_old / 1e12:5.2f} TB/s   "
          f"new {t_new * 1e6:7.1f} us {nbytes / t_new / 1e12:5.2f} TB/s   x{t_old / t_new:.2f}", flush=True)
    return t_old, t_new


tot_old = tot_new = 0.0
for scale, h in MAPS:
    C, E, Kc = LEVEL[scale]
    D = 2 * C + E + Kc
    Dp = padded_width(D)
    buf = torch.randn((B, h, h, Dp), device=DEV).to(DT)
    d = buf.permute(0, 3, 1, 2)
    flow = (torch.rand((B, 2, h, h), device=DEV) * 2.2 - 1.1)
    we, be = torch.randn((E, 2), device=DEV), torch.randn((E,), device=DEV)
    if scale in PROJ:
        K, N = PROJ[scale]
        f = torch.randn((B, K, h, h), device=DEV).to(DT).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn((K, N), device=DEV) / K ** 0.5).to(DT)
        b = torch.randn((N,), device=DEV).to(DT)
        wt16, b16 = (torch.nn.functional.pad(wt, (0, 16 - N)).contiguous(), torch.nn.functional.pad(b, (0, 16 - N)).contiguous()) if N < 16 else (wt, b)
        tgt = buf.as_strided((B, h * h, wt16.shape[1]), (h * h * Dp, Dp, 1))
        a = f.flatten(2).transpose(1, 2)
        wp, bp = ops.project_skinny_pack(wt, b)
        rows, out = f.permute(0, 2, 3, 1).reshape(B * h * h, K), buf.as_strided((B * h * h, N), (Dp, 1))
        t = line("project", f"{K}->{N} {h}x{h}", B * h * h * (K + N) * 2,
                 timed(lambda: torch.baddbmm(b16, a, wt16.unsqueeze(0).expand(B, -1, -1), out=tgt)),
                 timed(lambda: ops.project_skinny(rows, wp, bp, N, out)))
        tot_old, tot_new = tot_old + t[0], tot_new + t[1]

    def old():
        if Dp > D:
            buf[..., D:].zero_()
        ops.warp_bilinear(d[:, :C], flow, out=d[:, C:2 * C], batch_shift=1)
        ops.disp_emb(flow, we, be, 1.25, out=d[:, 2 * C:2 * C + E])

    t = line("assemble", f"C={C} E={E} Dp={Dp} {h}x{h}", B * h * h * (8 + (2 * C + E + Dp - D) * 2), timed(old),
             timed(lambda: ops.refiner_assemble(buf, d[:, :C], flow, we, be, 1.25, C, D, batch_shift=1)))
    tot_old, tot_new = tot_old + t[0], tot_new + t[1]
    if scale != 1:                                               # the upsample to the next level (864: 108 -> 216 -> 432 -> 864)
        cert = torch.randn((B, 1, h, h), device=DEV)
        nxt = {40: 70, 70: 140, 140: 280, 280: 560, 108: 216, 216: 432, 432: 864}[h]
        t = line("interp", f"{h}x{h} -> {nxt}x{nxt}", B * 3 * (h * h + nxt * nxt) * 4,
                 timed(lambda: (ops.interp_bilinear(flow, (nxt, nxt)), ops.interp_bilinear(cert, (nxt, nxt)))),
                 timed(lambda: ops.interp_bilinear_pair(flow, cert, (nxt, nxt))))
        tot_old, tot_new = tot_old + t[0], tot_new + t[1]
print(f"sum over one step (projections of scales 1 and 2 once per map, x is y): old {tot_old * 1e3:.3f} ms, new {tot_new * 1e3:.3f} ms")
