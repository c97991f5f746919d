"""sample_batch: fixed-shape, deterministic sampling for P pairs (ops.race_select, ops.kde_batch, *.sample_batch).

The rule under test: both selections rank by (key descending, item index ascending); keys and densities are bitwise those of
ops.race_keys / ops.kde.  tests/sample_batch_ref.py restates sample() with that rule on the host and no arithmetic of its own, so
every comparison here is exact (torch.equal), never a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import sample_batch_ref as R

H, W, NUM = 24, 80, 300
MODES = ("threshold_balanced", "threshold", "balanced")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _first_tie_free_seed(run):
    """First seed in range(16) at which run(seed) -> (..., keys1, keys2) has no two equal keys in either vector."""
    for seed in range(16):
        out = run(seed)
        if all(R.tie_free(k1) and R.tie_free(k2) for (_, _, k1, k2) in out):
            return seed, out
    return None, None


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_rule_equals_oracle_where_keys_are_tie_free():
    from oracle import roma_oracle as O
    g = _gen(1)
    m = R.distinct_matches(1, H, W, g)[0]
    c = torch.rand((H, W), generator=g) * 0.9 + 0.01                      # strictly positive: no key is 0
    seed, out = _first_tie_free_seed(lambda s: [R.sample_by_rule(m, c, NUM, s, race_keys=O.race_keys, kde=O.kde, return_keys=True)])
    assert seed is not None, "no tie-free seed in range(16)"
    gm, gc, _, _ = out[0]
    want_m, want_c = O.sample_seeded(m, c, NUM, seed)
    assert gm.shape == (NUM, 4) and torch.equal(gm, want_m) and torch.equal(gc, want_c)


def test_rule_takes_lowest_zero_key_indices_at_the_cut():
    from oracle import roma_oracle as O
    N, k = 500, 200
    pos = torch.randperm(N, generator=_gen(2))[:60]                        # certainty positive on fewer than k items
    c = torch.zeros(N)
    c[pos] = 0.5
    m = torch.arange(N, dtype=torch.float32)[:, None].expand(N, 4).contiguous()      # a match row names its item
    gm, gc = R.sample_by_rule(m, c, k, 3, mode="threshold", race_keys=O.race_keys, kde=O.kde)
    idx = gm[:, 0].long()
    assert sorted(idx[:60].tolist()) == sorted(pos.tolist()) and (gc[:60] == 1).all()
    zeros = [i for i in range(N) if i not in set(pos.tolist())]
    assert idx[60:].tolist() == zeros[: k - 60] and (gc[60:] == 0).all()


def test_entry_points_validate_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.roma_race_select(None, None, None, 1, 8, 2, -1.0, 0, None, None, None, 0, None) == _lib.ROMA_E_ARG
    assert b"roma_race_select: null pointer" in lib.roma_last_error()
    for P, N, k in ((1, 8, 9), (1, 8, 0), (0, 8, 2), (1, (1 << 24) + 1, 2)):             # k > N, k < 1, P < 1, N too large
        assert lib.roma_race_select(a, None, a, P, N, k, -1.0, 0, a, a, a, 1 << 20, None) == _lib.ROMA_E_SHAPE, (P, N, k)
        assert b"bad shape" in lib.roma_last_error()
        assert lib.roma_race_select_workspace(P, N, k) < 0
    need = lib.roma_race_select_workspace(2, 100, 10)
    assert need > 0
    assert lib.roma_race_select(a, None, a, 2, 100, 10, -1.0, 0, a, a, a, need - 1, None) == _lib.ROMA_E_ARG
    assert b"workspace" in lib.roma_last_error()
    assert lib.roma_kde_density_batch(None, None, None, 1, 8, 8, 1, 0.1, 1, None) == _lib.ROMA_E_ARG
    assert b"roma_kde_density_batch: null pointer" in lib.roma_last_error()
    for P, N, n, down, std in ((0, 8, 8, 1, 0.1), (1, 8, 0, 1, 0.1), (1, 8, 4, 1, 0.1), (1, 8, 8, 0, 0.1), (1, 8, 8, 1, 0.0)):
        assert lib.roma_kde_density_batch(a, None, a, P, N, n, down, std, 1, None) == _lib.ROMA_E_SHAPE, (P, N, n, down, std)


def test_ops_refuse_cpu_tensors():
    from roma_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.race_select(torch.rand(2, 16), 4, seeds=[1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kde_batch(torch.zeros(2, 8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_batch(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4), 4, seeds=[1, 2])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

DEV = "cuda:0"


def _weights(kind, P, N, g):
    """-> (weights (P,N), thresh)"""
    if kind == "continuous":
        return torch.rand((P, N), generator=g) * 0.98 + 0.01, -1.0
    if kind == "all_one":                                                   # every weight above the threshold: w = 1, 24-bit u ties
        return torch.rand((P, N), generator=g) * 0.9 + 0.1, 0.05
    if kind == "few_positive":                                              # key-0 ties sit at the cut for k > 100
        w = torch.zeros((P, N))
        for r in range(P):
            w[r, torch.randperm(N, generator=g)[:100]] = torch.rand(100, generator=g) * 0.9 + 0.05
        return w, -1.0
    assert kind == "all_zero"
    return torch.zeros((P, N)), -1.0


def _select_ref(ops, w, k, thresh, seeds, counter=None, stage=0):
    rows = []
    for r in range(w.shape[0]):
        keys = ops.race_keys(w[r], thresh, seeds[r], counter=None if counter is None else counter[r], stage=stage)
        index = np.arange(w.shape[1]) if counter is None else counter[r]
        rows.append(torch.from_numpy(R.select_by_rule(keys, index, k)))
    return torch.stack(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["continuous", "all_one", "few_positive", "all_zero"])
def test_race_select_matches_lexsort_of_race_keys(kind):
    from roma_amd import ops
    P, N, seeds = 3, 3001, [7, 2 ** 31 + 5, 123456789]
    w, thresh = _weights(kind, P, N, _gen(11))
    w = w.to(DEV)
    for k in (1, 257, 3001):
        got = ops.race_select(w, k, thresh, seeds)
        assert got.shape == (P, k) and got.dtype == torch.int64
        assert torch.equal(got.cpu(), _select_ref(ops, w, k, thresh, seeds)), (kind, k)


@pytest.mark.gpu
def test_race_select_with_a_counter_permutation_at_stage_1():
    from roma_amd import ops
    P, N, k, seeds = 3, 3001, 257, [1, 2, 3]
    g = _gen(12)
    w, thresh = _weights("all_one", P, N, g)
    counter = torch.stack([torch.randperm(N, generator=g) for _ in range(P)])
    got = ops.race_select(w.to(DEV), k, thresh, torch.tensor(seeds, device=DEV), counter=counter.to(DEV), stage=1)
    assert torch.equal(got.cpu(), _select_ref(ops, w.to(DEV), k, thresh, seeds, counter=counter.to(DEV), stage=1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["continuous", "all_one"])
def test_race_select_when_the_prefix_bin_spans_many_workgroups(kind):
    from roma_amd import ops
    w, thresh = _weights(kind, 1, 70_000, _gen(13))
    got = ops.race_select(w.to(DEV), 4096, thresh, [99])
    assert torch.equal(got.cpu(), _select_ref(ops, w.to(DEV), 4096, thresh, [99]))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("down", [1, 3])
def test_kde_batch_is_bitwise_kde_per_pair(half, down):
    from roma_amd import ops
    g = _gen(14)
    for n in (1, 63, 64, 65, 256, 257, 1000):
        x = (torch.rand((3, n, 4), generator=g) * 0.6 - 0.3).to(DEV)
        got = ops.kde_batch(x, std=0.1, half=half, down=down)
        assert got.shape == (3, n) and got.dtype == (torch.float16 if half else torch.float32)
        for r in range(3):
            assert torch.equal(got[r], ops.kde(x[r], std=0.1, half=half, down=down)), (n, r)
    big = (torch.rand((3, 1500, 4), generator=g) * 0.6 - 0.3).to(DEV)       # the gathering form: rows index[r] of a larger set
    index = torch.stack([torch.randperm(1500, generator=g)[:257] for _ in range(3)]).to(DEV)
    got = ops.kde_batch(big, std=0.1, half=half, down=down, index=index)
    for r in range(3):
        assert torch.equal(got[r], ops.kde(big[r][index[r]], std=0.1, half=half, down=down))


def _model(cls_name, mode):
    if cls_name == "tiny":
        from roma_amd.tiny import TinyRoMa
        return TinyRoMa(xfeat=torch.nn.Identity(), sample_mode=mode)
    from roma_amd.matcher import RegressionMatcher
    return RegressionMatcher(torch.nn.Identity(), torch.nn.Identity(), sample_mode=mode)


def _inputs(P, h, w, seed, kind="general"):
    g = _gen(seed)
    m = R.distinct_matches(P, h, w, g)
    if kind == "general":                                                    # zeros (out of bounds), values on both sides of 0.05
        c = torch.rand((P, h, w), generator=g)
        c = torch.where(c < 0.2, torch.zeros_like(c), (c - 0.2) * 0.2)
        c[P - 1] = 0                                                         # one pair with an all-zero certainty map
    elif kind == "all_one":
        c = torch.rand((P, h, w), generator=g) * 0.9 + 0.1
    else:                                                                    # strictly positive, continuous, below the threshold too
        c = torch.rand((P, h, w), generator=g) * 0.9 + 0.01
    return m.to(DEV), c.to(DEV)


def _check_against_rule(model, m, c, num, seeds):
    from roma_amd import ops
    gm, gc = model.sample_batch(m, c, num=num, seeds=seeds)
    N = c[0].numel()
    balanced = "balanced" in model.sample_mode
    k1 = min((4 if balanced else 1) * num, N)
    k2 = min(num, k1) if balanced else k1
    assert gm.shape == (m.shape[0], k2, 4) and gc.shape == (m.shape[0], k2)
    assert torch.isfinite(gm).all() and torch.isfinite(gc).all()
    for r in range(m.shape[0]):
        want_m, want_c = R.sample_by_rule(m[r], c[r], num, seeds[r], mode=model.sample_mode, thresh=model.sample_thresh,
                                          race_keys=ops.race_keys, kde=ops.kde)
        assert torch.equal(gm[r], want_m) and torch.equal(gc[r], want_c), (model.sample_mode, r)
    return gm, gc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_sample_batch_equals_the_rule(mode):
    model = _model("roma", mode)
    m, c = _inputs(3, H, W, 21)
    _check_against_rule(model, m, c, NUM, [5, 6, 7])
    m, c = _inputs(3, 12, 40, 22)                                            # N = 480 < 4 * num: k1 = N
    _check_against_rule(model, m, c, NUM, [8, 9, 10])


@pytest.mark.gpu
def test_sample_batch_all_zero_pair_returns_lowest_indices():
    model = _model("roma", "threshold")
    m, c = _inputs(3, H, W, 21)
    gm, gc = model.sample_batch(m, c, num=NUM, seeds=[5, 6, 7])
    assert torch.equal(gm[2], m[2].reshape(-1, 4)[:NUM]) and (gc[2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_tiny_sample_batch_equals_the_rule(mode):
    m, c = _inputs(3, H, W, 23)
    _check_against_rule(_model("tiny", mode), m, c, NUM, [1, 2, 3])


@pytest.mark.gpu
def test_sample_batch_equals_sample_where_keys_are_tie_free():
    from roma_amd import ops
    model = _model("roma", "threshold_balanced")
    m, c = _inputs(3, H, W, 24, kind="positive")
    seed, _ = _first_tie_free_seed(lambda s: [R.sample_by_rule(m[r], c[r], NUM, s, race_keys=ops.race_keys, kde=ops.kde, return_keys=True)
                                              for r in range(3)])
    assert seed is not None, "no tie-free seed in range(16)"
    gm, gc = model.sample_batch(m, c, num=NUM, seeds=[seed] * 3)
    for r in range(3):
        want_m, want_c = model.sample(m[r], c[r], num=NUM, seed=seed)
        assert torch.equal(gm[r], want_m) and torch.equal(gc[r], want_c), r


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_batch():
    model = _model("roma", "threshold_balanced")
    m, c = _inputs(3, H, W, 25, kind="all_one")                              # every weight 1: ties by the hundred
    gm3, gc3 = model.sample_batch(m, c, num=NUM, seeds=torch.tensor([4, 5, 6], device=DEV))
    gm1, gc1 = model.sample_batch(m[1:2], c[1:2], num=NUM, seeds=[5])
    assert torch.equal(gm3[1], gm1[0]) and torch.equal(gc3[1], gc1[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_output_size_is_fixed_and_items_are_distinct(mode):
    model = _model("roma", mode)
    for kind in ("general", "all_one"):
        m, c = _inputs(3, H, W, 26, kind=kind)
        gm, gc = model.sample_batch(m, c, num=NUM)                           # seeds from torch's CPU generator
        k2 = NUM if "balanced" in mode else min(NUM, H * W)
        assert gm.shape == (3, k2, 4) and gc.shape == (3, k2)
        for r in range(3):
            assert torch.unique(gm[r], dim=0).shape[0] == k2                 # distinct match rows: no item drawn twice
