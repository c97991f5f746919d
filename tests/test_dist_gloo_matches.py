"""gather="matches" on CPU: world_size-2 gloo processes sample (a fake, deterministic stand-in for sample_batch) on their shard and
gather the fixed-shape (p, num, 4) / (p, num) results to rank 0 in pair order — dist.gather_matches, also through match_sharded."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NUM = 6


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fake_match(pairs):
    """(pair index i) -> a dense warp filled with i and a certainty filled with i / 100"""
    w = torch.stack([torch.full((3, 4, 4), float(i)) for i in pairs]) if pairs else torch.zeros(0, 3, 4, 4)
    c = torch.stack([torch.full((3, 4), i / 100.0) for i in pairs]) if pairs else torch.zeros(0, 3, 4)
    return w, c


def _fake_sample(warp, cert):
    """NUM items per pair; item j of pair i is (i, j, i, j) with certainty i / 100 + j / 1000: order errors show in both axes."""
    P = warp.shape[0]
    j = torch.arange(NUM, dtype=torch.float32)
    i = warp[:, 0, 0, 0]
    m = torch.stack((i[:, None].expand(P, NUM), j[None].expand(P, NUM), i[:, None].expand(P, NUM), j[None].expand(P, NUM)), dim=-1)
    return m.contiguous(), cert[:, 0, 0, None] + j[None] / 1000.0


def _worker(rank, world, port, npairs, q, through_match_sharded):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from roma_amd.dist import gather_matches, match_sharded, shard_range
        lo, hi = shard_range(npairs, world, rank)
        if through_match_sharded:
            m, c = match_sharded(_fake_match, list(range(npairs)), gather="matches", sample_fn=_fake_sample)
        else:
            m, c = gather_matches(*_fake_sample(*_fake_match(list(range(lo, hi)))), npairs)
        q.put((rank, None if m is None else m.clone(), None if c is None else c.clone(), (lo, hi)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("npairs,through_match_sharded", [(3, False), (4, False), (3, True)])
def test_two_rank_gather_of_sampled_matches(npairs, through_match_sharded):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, npairs, q, through_match_sharded)) for r in range(world)]
    for p in procs:
        p.start()
    results = {r[0]: r for r in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert results[1][1] is None and results[1][2] is None                  # non-destination ranks get (None, None)
    _, m, c, _ = results[0]
    assert m.shape == (npairs, NUM, 4) and c.shape == (npairs, NUM) and m.dtype == torch.float32
    want_m, want_c = _fake_sample(*_fake_match(list(range(npairs))))
    assert torch.equal(m, want_m) and torch.equal(c, want_c)               # pair order and item order preserved, padding trimmed
    assert results[0][3][1] == results[1][3][0] and results[1][3][1] == npairs


def test_single_process_samples_without_a_gather():
    from roma_amd.dist import match_sharded
    m, c = match_sharded(_fake_match, [0, 1, 2], gather="matches", sample_fn=_fake_sample)
    assert m.shape == (3, NUM, 4) and float(m[2, 1, 0]) == 2.0 and float(m[2, 1, 1]) == 1.0
    with pytest.raises(ValueError, match="sample_fn"):
        match_sharded(_fake_match, [0], gather="matches")
