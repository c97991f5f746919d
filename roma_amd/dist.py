"""Multi-GPU sharding of image-pair batches: one process per GPU, contiguous blocks of pairs per rank, no data-path
collective except ONE order-preserving gather of the results at the end.  `backend="nccl"` is RCCL
over xGMI on ROCm; the same code runs on gloo for the CPU tests."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist


def shard_range(num_pairs: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous block [lo, hi) of pair indices for `rank`; the first (num_pairs % world_size) ranks get one extra."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    q, r = divmod(num_pairs, world_size)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def gather_results(warp: torch.Tensor, certainty: torch.Tensor, num_pairs: int, dst: int = 0, group=None, wire_dtype=None):
    """Gather each rank's stacked results (p_rank, H, W2, 4) / (p_rank, H, W2) to `dst`, in pair order.
    Uneven shards are padded to the largest shard for the collective and trimmed afterwards.  Returns
    (warp, certainty) on dst, (None, None) elsewhere.  One direct gather of one packed tensor: every peer sends its shard
    over its own xGMI link (no ring).

    wire_dtype=torch.float16 halves the 29.9 MB/pair on the links: warp coordinates live in [-1, 1]
    (fp16 spacing <= 4.9e-4 there = 0.2 px at 864) and certainty in [0, 1]; the result on dst is cast back to the input
    dtype.  Default: the exact fp32 tensors."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if world == 1:
        return warp, certainty
    out_dtype = (warp.dtype, certainty.dtype)
    if wire_dtype is not None:
        warp, certainty = warp.to(wire_dtype), certainty.to(wire_dtype)
    counts = [shard_range(num_pairs, world, r) for r in range(world)]
    pmax = max(hi - lo for lo, hi in counts)
    H, W2 = warp.shape[1], warp.shape[2]
    # ONE collective per step: a pair travels as one packed (H, W2, 5) record — 4 warp coordinates + certainty — in the wire dtype
    # (round 2 issued two gathers per step); an uneven shard is padded up to the largest one inside the packed buffer
    wire = torch.promote_types(warp.dtype, certainty.dtype)
    packed = torch.zeros((pmax, H, W2, 5), dtype=wire, device=warp.device) if warp.shape[0] < pmax else \
        torch.empty((pmax, H, W2, 5), dtype=wire, device=warp.device)
    n = warp.shape[0]
    packed[:n, ..., :4] = warp
    packed[:n, ..., 4] = certainty
    parts = [torch.empty_like(packed) for _ in range(world)] if rank == dst else None
    dist.gather(packed, parts, dst=dst, group=group)
    if rank != dst:
        return None, None
    full = torch.cat([parts[r][: hi - lo] for r, (lo, hi) in enumerate(counts)], dim=0)
    return full[..., :4].to(out_dtype[0]).contiguous(), full[..., 4].to(out_dtype[1]).contiguous()


def gather_matches(matches: torch.Tensor, certainty: torch.Tensor, num_pairs: int, dst: int = 0, group=None):
    """Gather each rank's sampled matches (p_rank, num, 4) / (p_rank, num) — sample_batch's fixed-shape result — to `dst`, in pair
    order: about 200 KB per pair at num = 10 000 on the links, where gather_results ships the 29.9 MB dense warp.  Uneven shards
    are padded to the largest shard inside one packed (num, 5) record per pair, as gather_results pads them.  Returns
    (matches, certainty) on dst, (None, None) elsewhere."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if world == 1:
        return matches, certainty
    counts = [shard_range(num_pairs, world, r) for r in range(world)]
    pmax = max(hi - lo for lo, hi in counts)
    n, num = matches.shape[0], matches.shape[1]
    wire = torch.promote_types(matches.dtype, certainty.dtype)
    packed = torch.zeros((pmax, num, 5), dtype=wire, device=matches.device)
    packed[:n, :, :4] = matches
    packed[:n, :, 4] = certainty
    parts = [torch.empty_like(packed) for _ in range(world)] if rank == dst else None
    dist.gather(packed, parts, dst=dst, group=group)
    if rank != dst:
        return None, None
    full = torch.cat([parts[r][: hi - lo] for r, (lo, hi) in enumerate(counts)], dim=0)
    return full[..., :4].to(matches.dtype).contiguous(), full[..., 4].to(certainty.dtype).contiguous()


def match_sharded(match_fn: Callable, pairs: Sequence, dst: int = 0, group=None, wire_dtype=None, gather: str = "dense",
                  sample_fn: Optional[Callable] = None):
    """Run `match_fn(list_of_local_pairs) -> (warp, certainty)` on this rank's contiguous shard of `pairs` and gather.
    gather="matches": `sample_fn(warp, certainty) -> (matches (p,num,4), certainty (p,num))` (e.g. model.sample_batch) runs on
    the local shard first and only the samples travel (gather_matches)."""
    if gather not in ("dense", "matches"):
        raise ValueError(f"gather must be 'dense' or 'matches', got {gather!r}")
    if gather == "matches" and sample_fn is None:
        raise ValueError("gather='matches' needs a sample_fn")
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_range(len(pairs), world, rank)
    warp, cert = match_fn(list(pairs[lo:hi]))
    if gather == "matches":
        m, c = sample_fn(warp, cert)
        return (m, c) if world == 1 else gather_matches(m, c, len(pairs), dst=dst, group=group)
    if world == 1:
        return warp, cert
    return gather_results(warp, cert, len(pairs), dst=dst, group=group, wire_dtype=wire_dtype)
