#!/usr/bin/env python3
"""The one-launch D = 144 refiner block (ops.refiner_block_mid) against the two calls it joins (ops.dwconv5x5_bn_relu +
ops.pointwise_mfma), fp16, B = 2: python tools/mid_micro.py [h ...]   (default: the product shapes 280 and 432)
Device events, the two forms alternating, median of several windows; bytes are the 2 * C * 2 B per pixel a block has to move."""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import ops
C, B, WINDOWS, ITERS = 144, 2, 9, 20
for h in [int(a) for a in sys.argv[1:]] or [280, 432]:
    g = torch.Generator().manual_seed(h)
    x = torch.randn(B, h, h, C, generator=g).cuda().half()
    w25 = (torch.randn(25, C, generator=g) * 0.2).cuda()
    sc, sh = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    wt = torch.zeros(160, 160)
    wt[:C, :C] = torch.randn(C, C, generator=g) / C ** 0.5
    wt = wt.cuda().half()
    bias = torch.zeros(160)
    bias[:C] = torch.randn(C, generator=g) * 0.1
    bias = bias.cuda()
    t, out1, out2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

    def one():
        ops.refiner_block_mid(x, w25, sc, sh, wt, bias, C, out=out1)

    def two():
        ops.dwconv5x5_bn_relu(x.permute(0, 3, 1, 2), w25, sc, sh, out=t.permute(0, 3, 1, 2))
        ops.pointwise_mfma(t.view(-1, C), wt, bias, C, out=out2.view(-1, C))

    forms = (("one launch", one), ("two calls", two))
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = torch.equal(out1.view(torch.int16), out2.view(torch.int16))
    times = {name: [] for name, _ in forms}
    for _ in range(WINDOWS):
        for name, fn in forms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(ITERS):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / ITERS * 1e3)
    nbytes = 2 * x.numel() * 2
    for name, _ in forms:
        ts = sorted(times[name])
        med = statistics.median(ts)
        print(f"h={h} B={B} C={C} {name:10s} median {med:7.1f} us  (min {ts[0]:7.1f}, max {ts[-1]:7.1f}; {WINDOWS} windows x {ITERS})"
              f"  {nbytes / 1e6:6.1f} MB in+out  {nbytes / med / 1e6:5.2f} TB/s", flush=True)
    print(f"h={h} one / two = {statistics.median(times['one launch']) / statistics.median(times['two calls']):.3f}   same bits: {same}", flush=True)
