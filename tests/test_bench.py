"""bench.py's --dump-outputs and argument checks, on the CPU: the writer itself, and the launcher / gather / dump plumbing through the
ROMA_BENCH_STUB stand-in step (see tests/test_dist_gloo.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=300)


def test_dump_outputs_writes_the_gathered_result_of_the_last_step(tmp_path):
    """--gpus 2 over the stub: rank 0 writes the (warp, certainty) it gathered, both ranks' pairs in order, as float32 .npy."""
    r = _bench(["--gpus", "2", "--steps", "2", "--warmup", "0", "--pairs", "3", "--dump-outputs", str(tmp_path)],
               ROMA_BENCH_STUB="1", ROMA_BENCH_BACKEND="gloo")
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["certainty.npy", "warp.npy"]
    warp, cert = np.load(tmp_path / "warp.npy"), np.load(tmp_path / "certainty.npy")
    assert warp.dtype == cert.dtype == np.float32 and warp.shape == (6, 4, 8, 4) and cert.shape == (6, 4, 8)
    assert [float(warp[i].max()) for i in range(6)] == [0, 0, 0, 1, 1, 1]


def test_dump_outputs_samples_large_outputs_under_64_mb(tmp_path):
    """Over the budget every array becomes the same seeded sample of its elements: under 64 MB in all, identical from call to
    call, and made of the array's own values in order; float64 stays float64, float16 becomes float32."""
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    warp = torch.arange(2 * 1000 * 2000 * 4, dtype=torch.float32).reshape(2, 1000, 2000, 4)        # 64 MB alone
    cert = torch.rand(2, 1000, 2000, generator=g, dtype=torch.float64)
    samples = [(torch.rand(100, 4, generator=g).half(), torch.rand(100, generator=g).half())]
    for d in ("a", "b"):
        bench.dump_outputs((warp, cert, samples), str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["certainty.npy", "sample_certainty_0.npy", "sample_matches_0.npy", "warp.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    w = np.load(tmp_path / "a" / "warp.npy")
    assert w.dtype == np.float32 and w.ndim == 1 and 0 < w.size < warp.numel() and np.all(np.diff(w) > 0)
    assert np.load(tmp_path / "a" / "certainty.npy").dtype == np.float64
    assert np.load(tmp_path / "a" / "sample_matches_0.npy").dtype == np.float32


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_no_timed_steps(args):
    r = _bench(args, ROMA_BENCH_STUB="1")
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_plain_stub_run_prints_the_headline_fields(tmp_path):
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)], ROMA_BENCH_STUB="1")
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and {"metric", "value", "unit", "higher_is_better", "dtype"} <= set(d)
    assert np.load(tmp_path / "warp.npy").shape == (1, 4, 8, 4)
