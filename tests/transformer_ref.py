"""fp64 restatements, in plain torch on the CPU, of the 16-bit transformer path: ops.add_layernorm (csrc/layernorm.hip), ops.attention
(csrc/attention.hip) and the pre-LN block stack that roma_amd.transformer.run_blocks_fused runs with one fused seam per half-block.

Everything is computed in float64; a value is rounded only where the real data path stores it:
  add_layernorm_ref   the new residual stream is rounded to x's dtype, and the LayerNorm statistics are taken from that ROUNDED stream
                      (what the next seam will read back); the output is rounded to out_dtype.  The float64 sum goes to the stream
                      dtype through float32, where the kernel's registers hold it (to_stream below).
  attention_ref       nothing is rounded: the inputs are the 16-bit values the kernel reads, the result stays float64.
  block_stack_ref     nothing is rounded: the weights are whatever the given modules hold (16-bit copies included), upcast.

The input builders below are shared by the CPU tests (tests/test_transformer_ref.py, which prove that each input separates a right kernel
from a specific wrong one) and the GPU tests (tests/test_transformer_kernels.py)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

ATT_SCALE = 64 ** -0.5

# The tolerances of tests/test_gpu_ops.py (test_add_layernorm_vs_torch, test_attention_vs_torch_sdpa), times max(1, |ref|max); the GPU
# tests apply them and the CPU tests prove that a wrong kernel would exceed them tenfold.
LN_OUT_TOL = {torch.float32: 2e-6, torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6}
ATT_TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}                                   # one unit in the last place, relative


ONE_HOT_SHAPES = [(130, 65), (274, 137), (256, 128)]                                          # (N, Nk) the GPU test runs
RAMP_SHAPES = [(192, 192), (200, 137)]


def ln_out_tolerance(out_dtype, ref, offset=False):
    """Bound on |out - ref| of add_layernorm; on offset_rows the rounding of the fp32 mean itself is added (offset_tolerance)."""
    return LN_OUT_TOL[out_dtype] * max(1.0, float(ref.double().abs().max())) + (offset_tolerance() if offset else 0.0)


def att_tolerance(dtype, ref):
    return ATT_TOL[dtype] * max(1.0, float(ref.double().abs().max()))


# ---- references -------------------------------------------------------------------------------------------------------------------
def layernorm64(x64, gamma, beta, eps):
    """LayerNorm over the last axis in float64, biased variance, two passes."""
    mean = x64.mean(dim=-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * gamma.double() + beta.double()


def to_stream(t64, dtype):
    """float64 -> the stream dtype the way the data path stores it: to float32 (the kernel's registers; torch's own 16-bit addcmul
    computes there too), then to dtype.  torch's float64 -> fp16 / bf16 conversion takes the same two steps; they are spelt out because
    the result differs from a single rounding where the float32 value lands on a 16-bit midpoint (63.734374867 -> 63.734375 -> 63.75,
    not 63.71875; 1 value in 2^13 for fp16), and tests/test_gpu_ops.py::test_add_layernorm_vs_torch pins this route."""
    return t64 if dtype == torch.float64 else t64.float().to(dtype)


def add_layernorm_ref(x, y, ls, gamma, beta, eps, out_dtype):
    """(new_x, out) of ops.add_layernorm: new_x = x + ls * y in float64, one conversion to x's dtype (y None: x itself), out =
    LayerNorm(new_x) in float64 converted to out_dtype (gamma None: new_x cast to out_dtype)."""
    if y is None:
        new_x = x.clone()
    else:
        y64 = y.double()
        new_x = to_stream(x.double() + (y64 if ls is None else ls.double() * y64), x.dtype)
    if gamma is None:
        return new_x, new_x.to(out_dtype)
    return new_x, layernorm64(new_x.double(), gamma, beta, eps).to(out_dtype)


def attention_ref(qkv, n_valid=None):
    """qkv (B, N, 3, H, 64) -> (B, N, H * 64) float64: softmax(q k^T * 64^-0.5) v over the first n_valid keys; every row queries."""
    B, N, three, H, d = qkv.shape
    assert three == 3 and d == 64
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))                    # (B, H, N, 64)
    n = N if n_valid is None else n_valid
    p = torch.softmax(q @ k[:, :, :n].transpose(-1, -2) * ATT_SCALE, dim=-1)
    return (p @ v[:, :, :n]).permute(0, 2, 1, 3).reshape(B, N, H * d)


def _lin64(m, x):
    y = x @ m.weight.detach().double().cpu().t()
    return y if m.bias is None else y + m.bias.detach().double().cpu()


def _ln64(m, x):
    return layernorm64(x, m.weight.detach().cpu(), m.bias.detach().cpu(), m.eps)


def _ls64(m, x):
    g = getattr(m, "gamma", None)                                                              # LayerScale, else nn.Identity
    return x if g is None else x * g.detach().double().cpu()


def block_stack_ref(blocks, x, n_valid=None, final=None):
    """The literal pre-LN stack in float64: x = x + ls1(attn(norm1(x))); x = x + ls2(mlp(norm2(x))) for every block, then the optional
    final LayerNorm module.  Keys / values are the first n_valid tokens; weights are read from the modules as they are."""
    x = x.detach().double().cpu()
    B, N, C = x.shape
    for blk in blocks:
        H = blk.attn.num_heads
        qkv = _lin64(blk.attn.qkv, _ln64(blk.norm1, x)).view(B, N, 3, H, C // H)
        x = x + _ls64(blk.ls1, _lin64(blk.attn.proj, attention_ref(qkv, n_valid)))
        h = _lin64(blk.mlp.fc1, _ln64(blk.norm2, x))
        x = x + _ls64(blk.ls2, _lin64(blk.mlp.fc2, F.gelu(h)))
    return x if final is None else _ln64(final, x)


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def offset_rows(rows, C, mean=64.0, std=0.25, seed=0):
    """(rows, C) float32 rows of mean `mean` and standard deviation `std`: E[x^2] - mean^2 cancels 16 bits on them."""
    g = torch.Generator().manual_seed(1000 + seed)
    return mean + std * torch.randn(rows, C, generator=g)


def offset_tolerance(mean=64.0, std=0.25):
    """What the rounding of an fp32 mean costs the normalised value on offset_rows: a few ulps of |mean|, divided by std."""
    return 8 * 2.0 ** -24 * abs(mean) / std


def one_hot_attention(N, Nk, dtype, H=2, seed=0):
    """qkv (1, N, 3, H, 64) whose softmax is one-hot: u_j in {+-1}^64, k_j = 2.75 u_j, q_i = 2.75 u_(i mod Nk), so query i scores
    2.75^2 * 64 / 8 = 60.5 nats on key i mod Nk and at least 30 nats less on every other valid key (test_transformer_ref asserts it):
    output row i is v[i mod Nk].  Rows >= Nk are poisoned: k = 5.5 u_((j - Nk) mod Nk), which would beat the true key by 60 nats, and
    v = 1000.  All values are exact in fp16 and bf16 except the random v, which is rounded to `dtype` here."""
    g = torch.Generator().manual_seed(2000 + seed)
    u = (torch.randint(0, 2, (Nk, H, 64), generator=g) * 2 - 1).float()
    idx = torch.arange(N) % Nk
    qkv = torch.empty(1, N, 3, H, 64)
    qkv[0, :, 0] = 2.75 * u[idx]
    qkv[0, :Nk, 1] = 2.75 * u
    qkv[0, Nk:, 1] = 5.5 * u[idx[: N - Nk]]
    qkv[0, :Nk, 2] = torch.randn(Nk, H, 64, generator=g)
    qkv[0, Nk:, 2] = 1000.0
    return qkv.to(dtype)


def one_hot_expected(qkv, Nk):
    """(1, N, H * 64): row i is v[i mod Nk], in qkv's dtype."""
    N = qkv.shape[1]
    return qkv[:, torch.arange(N) % Nk, 2].reshape(1, N, -1)


def ramp_attention(N, Nk, dtype, sign, H=2, seed=0):
    """qkv (1, N, 3, H, 64) where the logit of key j is sign * 0.5 * j nats plus noise of 0.25 nat (q[0] = 4, k_j[0] = sign * j, the other
    63 dimensions N(0, 0.5^2)): sign = +1 moves the running maximum in every tile, sign = -1 never after tile 0.  Rows >= Nk continue
    the ramp, so with sign = +1 a leaked key would take the whole weight."""
    g = torch.Generator().manual_seed(3000 + seed + (sign > 0))
    qkv = torch.randn(1, N, 3, H, 64, generator=g)
    qkv[:, :, :2] *= 0.5
    qkv[:, :, 0, :, 0] = 4.0
    qkv[:, :, 1, :, 0] = sign * torch.arange(N, dtype=torch.float32)[None, :, None]
    return qkv.to(dtype)


def noise_attention(B, N, H, dtype, seed=0):
    """The i.i.d. input of tests/test_gpu_ops.py::test_attention_vs_torch_sdpa: 1.5 * N(0, 1)."""
    g = torch.Generator().manual_seed(N * 7 + H + seed)
    return (torch.randn(B, N, 3, H, 64, generator=g) * 1.5).to(dtype)


def init_module(module, seed):
    """Seeded non-trivial parameters: LayerNorm weights and LayerScale gammas in [0.5, 1.5] (a swapped ls1 / ls2 or norm shows), GEMM /
    conv weights N(0, 1.5^2 / fan_in), tokens and position table N(0, 0.5^2), every bias N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(4000 + seed)
    with torch.no_grad():
        for m in module.modules():
            for leaf, p in m.named_parameters(recurse=False):
                if leaf == "gamma" or (isinstance(m, torch.nn.LayerNorm) and leaf == "weight"):
                    p.copy_(torch.rand(p.shape, generator=g) + 0.5)
                elif leaf == "weight" and p.dim() >= 2:
                    p.copy_(torch.randn(p.shape, generator=g) * 1.5 / math.sqrt(p[0].numel()))
                elif leaf in ("cls_token", "pos_embed", "mask_token"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.5)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return module.eval()


def linear64(m, x):
    """nn.Linear in float64 on the CPU, weights as the module holds them"""
    return _lin64(m, x)
