#!/usr/bin/env python3
"""Fill encoders.VGG_CONV_TABLE: for every 3x3 layer beyond the stem of the 560^2 and 864^2 VGG19 pyramids (B = 2, fp16, channels-last)
time each instance of ops.conv3x3_bias_relu against what it replaces, F.conv2d (MIOpen solver search on) + ops.bias_relu_ — for a
layer that a pool follows, + ops.maxpool2_nhwc against + ops.bias_relu_pool2_.  Device events, the sides alternating inside every
window, median of WINDOWS windows of CALLS calls.  Each shape runs in a child process of its own under `timeout`; a child that
faults, aborts or runs out of time ends the whole run.

    python tools/vgg_conv_tune.py                 # all shapes, then the table
    python tools/vgg_conv_tune.py --shape 64 64 2 560 560 1     # one child: Cin Cout B H W pooled
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS, CALLS = 9, 10


def shapes(B=2):
    out = []
    for side in (560, 864):
        for cin, cout, div, pooled in ((64, 64, 1, 1), (64, 128, 2, 0), (128, 128, 2, 1), (128, 256, 4, 0), (256, 256, 4, 0),
                                       (256, 256, 4, 1), (256, 512, 8, 0), (512, 512, 8, 0)):
            out.append((cin, cout, B, side // div, side // div, pooled))
    return out


def child(cin, cout, B, H, W, pooled):
    import torch
    import torch.nn.functional as F
    from roma_amd import ops
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    dev = "cuda:0"
    x = torch.randn(B, cin, H, W, device=dev).half().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5).half().contiguous(memory_format=torch.channels_last)
    b = (torch.randn(cout, device=dev) * 0.1).half()
    names = ops.conv3x3_instances()

    def library():
        y = F.conv2d(x, w, None, padding=1)
        return ops.bias_relu_pool2_(y, b) if pooled else ops.bias_relu_(y, b)

    def fused(i):
        def run():
            y = ops.conv3x3_bias_relu(x, w, b, i)
            return ops.maxpool2_nhwc(y) if pooled else y
        return run

    sides = {"library": library}
    for i in range(len(names)):
        try:
            fused(i)()
            sides[i] = fused(i)
        except ValueError:                                       # the instance does not support the shape
            pass
    for f in sides.values():                                     # warm-up (and MIOpen's search for the library side)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(WINDOWS):
        for k, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    res = {str(k): (statistics.median(v), min(v), max(v)) for k, v in times.items()}
    print("RESULT " + json.dumps({"shape": [cin, cout, B, H, W, pooled], "us": res}), flush=True)


def main():
    if "--shape" in sys.argv:
        child(*[int(v) for v in sys.argv[sys.argv.index("--shape") + 1:][:6]])
        return
    results = []
    for sh in shapes():
        cmd = ["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--shape"] + [str(v) for v in sh]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:])
            sys.exit(f"shape {sh}: child ended with status {p.returncode}; nothing more is run")
        r = json.loads(line[0][7:])
        results.append(r)
        lib = r["us"]["library"]
        best = min((k for k in r["us"] if k != "library"), key=lambda k: r["us"][k][0])
        fu = r["us"][best]
        wins = fu[2] < lib[1]                                    # the fused side's slowest window below the library's fastest
        r["best"], r["wins"] = int(best), wins
        print(f"Cin={sh[0]:3d} Cout={sh[1]:3d} {sh[3]:3d}x{sh[4]:3d} pooled={sh[5]}  library {lib[0]:7.1f} us ({lib[1]:.1f} - {lib[2]:.1f})  "
              f"best fused #{best} {fu[0]:7.1f} us ({fu[1]:.1f} - {fu[2]:.1f})  {'FUSED' if wins else 'library'}   all: "
              + " ".join(f"#{k}:{v[0]:.1f}" for k, v in r["us"].items() if k != "library"), flush=True)
    # a (Cin, Cout, pixels) key takes the fused path only if every measured variant of it (plain and pooled) does, with the plain
    # variant's instance
    keys = {}
    for r in results:
        cin, cout, B, H, W, pooled = r["shape"]
        keys.setdefault((cin, cout, B * H * W), []).append(r)
    table = {}
    for (cin, cout, px), rs in sorted(keys.items()):
        if all(r["wins"] for r in rs):
            plain = min(rs, key=lambda r: r["shape"][5])
            table.setdefault((cin, cout), []).append((px, plain["best"]))
    print("\nVGG_CONV_TABLE = {")
    for (cin, cout), rows in table.items():
        if len(rows) == 2 and rows[0][1] == rows[1][1]:
            ent = [(rows[0][0], rows[1][0], rows[0][1])]
        else:
            ent = [(px, px, i) for px, i in rows]
        print(f"    ({cin}, {cout}): ({', '.join(str(e) for e in ent)},),")
    print("}")


if __name__ == "__main__":
    main()
