"""sample() for one pair, restated with both selections done on the host by the rule sample_batch promises: rank by
(key descending, item index ascending), a total order.  The keys and the densities come from injected functions — the CPU
oracle's (oracle.race_keys / oracle.kde) or the device's (ops.race_keys / ops.kde) — so this file adds no arithmetic of its own."""
import numpy as np
import torch


def select_by_rule(keys, index, k):
    """Positions of the k best items under (key descending, index ascending); np.lexsort's LAST key is the primary one."""
    keys = np.asarray(torch.as_tensor(keys).detach().cpu().numpy(), dtype=np.float64)
    index = np.asarray(torch.as_tensor(index).detach().cpu().numpy(), dtype=np.int64)
    return np.lexsort((index, -keys))[:k].copy()


def sample_by_rule(matches, certainty, num, seed, mode="threshold_balanced", thresh=0.05, race_keys=None, kde=None,
                   return_keys=False):
    t = thresh if "threshold" in mode else -1.0
    m, c = matches.reshape(-1, 4), certainty.reshape(-1)
    N = c.numel()
    balanced = "balanced" in mode
    k1 = min((4 if balanced else 1) * num, N)
    keys1 = race_keys(c, t, seed)
    good = torch.from_numpy(select_by_rule(keys1, np.arange(N), k1)).to(c.device)
    gm, gc = m[good], c[good]
    if t >= 0:
        gc = torch.where(gc > t, torch.ones_like(gc), gc)
    if not balanced:
        return (gm, gc, keys1, None) if return_keys else (gm, gc)
    density = kde(gm, std=0.1)
    p = 1 / (density + 1)
    p[density < 10] = 1e-7
    keys2 = race_keys(p.float(), -1.0, seed, counter=good, stage=1)
    bal = torch.from_numpy(select_by_rule(keys2, good, min(num, k1))).to(c.device)
    return (gm[bal], gc[bal], keys1, keys2) if return_keys else (gm[bal], gc[bal])


def tie_free(keys):
    return keys is None or torch.unique(torch.as_tensor(keys)).numel() == torch.as_tensor(keys).numel()


def distinct_matches(P, H, W, gen):
    """(P,H,W,4) matches in [-1, 1] whose rows are pairwise distinct within a pair (the first coordinate is a strictly increasing
    ramp), clustered enough that the KDE sees densities on both sides of sample()'s `density < 10` cut."""
    N = H * W
    ramp = torch.linspace(-1, 1, N).reshape(1, H, W).expand(P, H, W)
    rest = torch.rand((P, H, W, 3), generator=gen) * 2 - 1
    rest[:, : H // 2] *= 0.05                                   # half of the items sit in a dense cluster
    return torch.cat((ramp[..., None], rest), dim=-1).contiguous()
