# roma_amd.geometry.build_tracks: time of one call (eight launches, csrc/tracks.hip) on synthetic pairwise matches, and, where scipy is
# importable, scipy.sparse.csgraph.connected_components on the same edges as the host yardstick (the component step alone: the host
# would still have to quantise, pick representatives and write the tracks).  Device events after 3 warm-up calls, median of `reps`
# (default 20).  Shapes: M = 64 and 1024 pairs of k = 10 000 matches over V = 32 views of 864 x 1152, cell = 2, 4, 8 pixels,
# max_tracks = 2^18.  The matches: 200 000 scene points, each at a pixel centre of a common plane shifted by up to 100 px per view; a
# pair draws k points, the A end exact (a sampled match's grid-anchored end), the B end with 0.5 px of noise; certainty uniform in
# (0.05, 1); the pairs cycle through all 496 pairs a < b in a seeded random order.
# `tracks_micro.py [reps]` runs every case in a child process of its own under `timeout`, one after the other, and stops at the first
# that fails; `--case M cell [reps]` is what a child runs.  The committed output is profiles/tracks_micro.txt.
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, H, W, K_MATCHES, POINTS, MAX_TRACKS = 32, 864, 1152, 10000, 200000, 1 << 18
CASES = [(M, cell) for M in (64, 1024) for cell in (2, 4, 8)]
CASE_TIMEOUT = 240                                           # seconds, per child


def make_matches(M, seed=0):
    """-> matches (M,k,4) fp32 normalised, certainty (M,k) fp32, pairs (M,2) int32, on the device"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *shape: torch.rand(shape, generator=gen, device="cuda")  # noqa: E731
    base = torch.stack([torch.floor(rand(POINTS) * W), torch.floor(rand(POINTS) * H)], -1) + 0.5
    shift = torch.round((rand(V, 2) * 2 - 1) * 100)
    every = torch.tensor([(a, b) for a in range(V) for b in range(a + 1, V)], dtype=torch.int32, device="cuda")
    pairs = every[torch.randperm(len(every), generator=gen, device="cuda")][torch.arange(M, device="cuda") % len(every)]
    pick = torch.randint(0, POINTS, (M, K_MATCHES), generator=gen, device="cuda")
    half = torch.tensor([W / 2, H / 2], device="cuda")
    ends = []
    for side in range(2):
        px = base[pick] + shift[pairs[:, side].long()][:, None, :]
        if side:
            px = px + 0.5 * torch.randn(px.shape, generator=gen, device="cuda")
        ends.append(px / half - 1)
    return torch.cat(ends, -1).float().contiguous(), 0.05 + 0.95 * rand(M, K_MATCHES), pairs.contiguous()


def run_case(M, cell, reps):
    import numpy as np
    import torch
    from roma_amd import _lib, geometry
    from tests import tracks_ref as TR
    _lib.load()
    sizes = [(H, W)] * V
    matches, certainty, pairs = make_matches(M)
    call = lambda: geometry.build_tracks(matches, certainty, pairs, sizes, cell=cell, max_tracks=MAX_TRACKS)  # noqa: E731
    for _ in range(3):
        tr = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        tr = call()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    counts = tr.counts.cpu().numpy()
    assert counts[3] == 0, "the union's retry cap was reached"
    cells = int(TR.grid(sizes, cell)[0][-1])
    usable = int((tr.track_of_match >= 0).sum())
    line = (f"M = {M:4d} pairs x k = {K_MATCHES}, cell = {cell}: {cells / 1e6:5.2f} M cells, workspace {21 * cells / 2 ** 20:6.1f} MiB;  build_tracks "
            f"{float(np.median(times)):7.3f} ms (min {min(times):.3f});  {counts[0]} tracks ({min(int(counts[0]), MAX_TRACKS)} kept), {counts[1]} conflicting, "
            f"{counts[2]} below min_views, {usable} of {M * K_MATCHES} matches in a kept track")
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        print(line + ";  scipy is not importable: no host yardstick was run", flush=True)
        return
    m, c, p = matches.cpu().numpy(), certainty.cpu().numpy(), pairs.cpu().numpy().astype(np.int64)
    va, vb = np.broadcast_to(p[:, :1], c.shape), np.broadcast_to(p[:, 1:], c.shape)
    _, _, ina, ca = TR.endpoints(m[..., 0:2], va, sizes, cell)
    _, _, inb, cb = TR.endpoints(m[..., 2:4], vb, sizes, cell)
    ok = ina & inb & (c > 0)
    ua, ub = ca[ok], cb[ok]
    t0 = time.perf_counter()
    graph = sp.coo_matrix((np.ones(len(ua), np.int8), (ua, ub)), shape=(cells, cells)).tocsr()
    t1 = time.perf_counter()
    n, labels = connected_components(graph, directed=False)
    t2 = time.perf_counter()
    nodes = np.zeros(cells, bool)
    nodes[ua] = nodes[ub] = True
    total = int(counts[:3].sum())
    assert len(np.unique(labels[nodes])) == total, (len(np.unique(labels[nodes])), total)
    print(line + f";  host: scipy connected_components on the same {len(ua)} edges {1e3 * (t2 - t1):8.1f} ms after {1e3 * (t1 - t0):8.1f} ms of CSR "
          f"assembly, the same {total} components", flush=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--case":
        run_case(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 20)
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "20"
    print(f"build_tracks: V = {V} views of {H} x {W}, max_tracks = {MAX_TRACKS}; device events, median of {reps} calls after 3 warm-up calls", flush=True)
    for M, cell in CASES:
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT), sys.executable, os.path.abspath(__file__), "--case", str(M), str(cell),
                             reps]).returncode
        if rc != 0:
            print(f"case M = {M}, cell = {cell} ended with status {rc}; stopping here")
            sys.exit(rc)


if __name__ == "__main__":
    main()
