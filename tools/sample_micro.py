# RegressionMatcher.sample_batch against the loop of P sample() calls it replaces, and the stages of sample_batch on their own.
# Shapes: P certainty maps of 864 x 1728 (N = 1 492 992 items per pair), num = 10 000 (k1 = 40 000, k2 = 10 000), P = 1 and P = 8.
#   (a) loop     P calls of sample(matches[p], certainty[p], num, seed=...): per pair two race_keys launches, two 1-D torch.topk,
#                one KDE launch, four gathers
#   (b) batch    one sample_batch call
#   (c) stages   the pieces of (b), each timed alone on the tensors (b) hands it
# Method: time per CALL (wrapper, allocations and every launch behind it) between two device events, each call timed on its own;
# a figure is the median of `inner` (>= 20) calls after warm-up, (a) and (b) alternating call by call; the whole is repeated `reps`
# (5) times, and the spread of a figure is max - min of its `reps` medians.  At the end, (b)'s rows are compared with (a)'s.
# The inputs are synthetic: 15 % of the certainties are 0 (out of bounds), 60 % are above sample_thresh; the matches are an
# identity grid plus a smooth warp, so the KDE sees the clustered coordinates a real warp has.
# `python tools/sample_micro.py [--out FILE]` runs every GPU step as a child process of its own under `timeout -k 10` and stops at
# the first that fails; the committed output is profiles/sample_batch_micro.txt.
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, NUM = 864, 1728, 10_000
STEP_LIMIT_S = 420


def inputs(P, dev):
    import torch
    g = torch.Generator().manual_seed(100 + P)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    m = torch.empty((P, H, W, 4))
    c = torch.empty((P, H, W))
    for p in range(P):
        a, b = (torch.rand(2, generator=g) * 0.2 - 0.1).tolist()
        m[p] = torch.stack((xs, ys, xs * (1 + a) + 0.05 * torch.sin(3 * ys + p), ys * (1 + b) + 0.05 * torch.cos(2 * xs)), -1)
        u = torch.rand((H, W), generator=g)
        c[p] = torch.where(u < 0.15, torch.zeros_like(u), torch.where(u < 0.40, (u - 0.15) * 0.2, u))
    return m.to(dev), c.to(dev)


def time_calls(fns, inner):
    """{name: median ms per call over `inner` calls}; the functions alternate call by call, each call between its own two events"""
    import numpy as np
    import torch
    ev = {name: [] for name in fns}
    for _ in range(inner):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[name].append((s, e))
    torch.cuda.synchronize()
    return {name: float(np.median([s.elapsed_time(e) for s, e in v])) for name, v in ev.items()}


def child(P, reps, inner):
    import numpy as np
    import torch
    from roma_amd import ops
    from roma_amd.matcher import RegressionMatcher
    if not torch.cuda.is_available():
        raise SystemExit("sample_micro.py measures on the device; there is none")
    dev = "cuda:0"
    torch.set_grad_enabled(False)
    model = RegressionMatcher(torch.nn.Identity(), torch.nn.Identity())
    m, c = inputs(P, dev)
    seeds = list(range(11, 11 + P))
    seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=dev)
    thresh = model.sample_thresh

    def loop():
        return [model.sample(m[p], c[p], num=NUM, seed=seeds[p]) for p in range(P)]

    def batch():
        return model.sample_batch(m, c, num=NUM, seeds=seeds_dev)

    # the tensors each stage of (b) works on
    mm, cc = m.reshape(P, -1, 4), c.reshape(P, -1)
    good = ops.race_select(cc, 4 * NUM, thresh, seeds_dev)
    density = ops.kde_batch(mm, std=0.1, half=True, down=1, index=good)
    p2 = torch.where(density < 10, torch.full_like(density, 1e-7), 1 / (density + 1))
    bal = ops.race_select(p2, NUM, -1.0, seeds_dev, counter=good, stage=1)
    keys40 = torch.randint(-2 ** 62, 2 ** 62, (P, 4 * NUM), device=dev)

    def elementwise():
        gc = cc.gather(1, good)
        gc = torch.where(gc > thresh, torch.ones_like(gc), gc)
        q = 1 / (density + 1)
        q = torch.where(density < 10, torch.full_like(q, 1e-7), q)
        sel = good.gather(1, bal)
        return mm.gather(1, sel[..., None].expand(-1, -1, 4)), gc.gather(1, bal), q

    stages = {
        "select 1 (N -> 40 000)": lambda: ops.race_select(cc, 4 * NUM, thresh, seeds_dev),
        "  of it: torch.sort of (P, 40 000) int64": lambda: torch.sort(keys40, dim=1, descending=True),
        "kde_batch (40 000, gathering)": lambda: ops.kde_batch(mm, std=0.1, half=True, down=1, index=good),
        "select 2 (40 000 -> 10 000)": lambda: ops.race_select(p2, NUM, -1.0, seeds_dev, counter=good, stage=1),
        "gathers and element-wise ops": elementwise,
    }
    for _ in range(5):
        la, lb = loop(), batch()
        for fn in stages.values():
            fn()
    torch.cuda.synchronize()
    same = sum(int(torch.equal(lb[0][p], la[p][0]) and torch.equal(lb[1][p], la[p][1])) for p in range(P))
    del la, lb
    meds = {}
    for _ in range(reps):
        for name, v in {**time_calls({"(a) loop of sample()": loop, "(b) sample_batch": batch}, inner), **time_calls(stages, inner)}.items():
            meds.setdefault(name, []).append(v)
    print(f"P = {P}: {H} x {W} maps, num = {NUM}; ms per call, median of {inner} calls, {reps} repetitions")
    for name, v in meds.items():
        print(f"  {name:44s} {np.median(v):8.3f} ms   (medians {' '.join(f'{x:.3f}' for x in v)}; spread {max(v) - min(v):.3f})")
    a, b = meds["(a) loop of sample()"], meds["(b) sample_batch"]
    ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
    print(f"  per pair: (a) {ma / P:.3f} ms, (b) {mb / P:.3f} ms; (a) - (b) = {ma - mb:.3f} ms per call, spread of (a) {spread:.3f} ms")
    if P == 1:
        print(f"  P = 1 condition, (b) not slower than (a) beyond the spread of (a): "
              f"{'holds' if mb <= ma + spread else 'FAILS: at one pair the launches of the two selections and their sorts cost more than the two top-k calls; sample() stays the one-pair path'}")
    else:
        print(f"  P = {P} condition, (b) below (a) by more than the spread of (a): {'holds' if ma - mb > spread else 'FAILS'}")
    print(f"  rows of (b) bitwise equal to sample() of the same seed: {same} of {P} (they may differ only where keys tie: sample() leaves "
          f"the choice among equal keys to torch.topk)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0, help="run the measurement for this P in this process")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_batch_micro.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner)
    lines = ["tools/sample_micro.py: sample_batch against the loop of sample() calls, time per CALL between device events "
             "(wrapper, allocations and launches included), (a) and (b) alternating"]
    for P in (1, 8):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(P),
                            "--reps", str(args.reps), "--inner", str(args.inner)], capture_output=True, text=True, cwd=ROOT)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:                                   # a failed GPU step ends the run: nothing more is started on the device
            lines.append(f"P = {P}: the step ended with status {r.returncode}; stopping")
            lines += r.stderr.splitlines()[-15:]
            break
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 1 if "stopping" in lines[-1] or any("ended with status" in ln for ln in lines) else 0


if __name__ == "__main__":
    sys.exit(main())
