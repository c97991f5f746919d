// Device code that the one-pair and the batched sampling kernels share (sample.hip, kde.hip, sample_batch.hip): the key of the
// exponential race and the KDE term / summation order are each written once, so both families produce the same bits.
#pragma once
#include "common.h"

namespace roma {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// the stream of one (seed, stage) pair: mixed non-linearly, so that neither seed + 1 nor the second draw of the same seed is a
// shifted copy of this one (round 2 hashed ctr * A + seed * B + C and ran the second draw at seed + 1)
__device__ __forceinline__ uint32_t race_stream(uint32_t seed, uint32_t stage) { return fmix32(seed ^ (stage * 0x9E3779B9u)); }

// key of item `ctr` (the item's identity, not its position) with weight w
__device__ __forceinline__ float race_key(float w, float thresh, uint32_t stream, uint32_t ctr) {
  if (thresh >= 0.f && w > thresh) w = 1.f;
  const uint32_t h = fmix32(stream + ctr * 0x9E3779B1u);
  const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);        // (0, 1], 24 bits
  const float e = -logf(u);
  return (w > 0.f) ? w / e : 0.f;
}

// ---- KDE ---------------------------------------------------------------------------------------------------------------------
constexpr int KDE_QP = 64, KDE_SPLIT = 4, KDE_TILE = 256;

__device__ __forceinline__ float r16(float v) { return (float)(half_t)v; }      // round to fp16, keep as float

// One term of the reference's half=True arithmetic (kde.py:6-12 with x.half()): torch.cdist on fp16 takes its matmul route
// (_euclidean_dist: [-2x, |x|^2, 1] . [y, 1, |y|^2] in an fp16 GEMM with fp32 accumulation, rounded to fp16, clamped, sqrt),
// then `** 2`, `/ (2 std^2)`, `exp` are fp16 element-wise ops (fp32 math, fp16 result) — every rounding point reproduced:
//   s = fp16(-2 x.y + |x|^2 + |y|^2);  d = fp16(sqrt(max(s,0)));  q = fp16(d*d);  t = fp16(-q / (2 std^2));  term = fp16(exp(t))
// The cancellation in s is rounded at fp16 resolution (~1e-3 .. 4e-3 absolute), which moves a term by up to ~20 %: a property
// of the reference that sample()'s `density < 10` cut sees, so the product path reproduces it instead of "improving" it.
__device__ __forceinline__ float term_half(const float4_t& xi, float xn, const float4_t& r, float rn, float neg_inv_two_var) {
  float s = (-2.f * xi[0]) * r[0];
  s = __builtin_fmaf(-2.f * xi[1], r[1], s);
  s = __builtin_fmaf(-2.f * xi[2], r[2], s);
  s = __builtin_fmaf(-2.f * xi[3], r[3], s);
  s = (s + xn) + rn;
  // hardware sqrt / exp2 (1-2 fp32 ulp) and a multiplication instead of the division: every intermediate is rounded to fp16
  // right after, so the fp16 value differs from the IEEE-exact evaluation only when the fp32 value sits within ~1e-7 of an fp16
  // rounding boundary (about 1 term in 4 000, each then off by one fp16 ulp OF THAT TERM); 3.2 -> 1.6 ms at N = 40 000
  const float d = r16(__builtin_amdgcn_sqrtf(fmaxf(r16(s), 0.f)));
  const float q = r16(d * d);
  const float t = r16(q * neg_inv_two_var);
  return r16(__builtin_amdgcn_exp2f(t * 1.4426950408889634f));
}

__device__ __forceinline__ float norm_half(const float4_t& v) {              // x.pow(2).sum(-1) in fp16
  return r16(((r16(v[0] * v[0]) + r16(v[1] * v[1])) + r16(v[2] * v[2])) + r16(v[3] * v[3]));
}

// The densities of the 64 query points of workgroup `qblock` of one point set; `load(j)` returns point j of the set, N its size.
// 256 threads: 64 query points x 4 interleaved quarters of each staged 256-point reference tile, the four partial sums combined
// through LDS in a fixed order.
template <bool HALF, typename Load>
__device__ __forceinline__ void kde_body(const Load& load, float* __restrict__ density, int qblock, int N, int down,
                                         float neg_scale_log2, float two_var) {
  __shared__ float4_t tile[KDE_TILE];
  __shared__ float tnorm[KDE_TILE];
  __shared__ float part[KDE_SPLIT][KDE_QP];
  const int tid = threadIdx.x, qi = tid & (KDE_QP - 1), s = tid >> 6;
  const int i = qblock * KDE_QP + qi;
  const float4_t xi = i < N ? load(i) : float4_t{0, 0, 0, 0};
  const float xn = HALF ? norm_half(xi) : 0.f;
  const int nref = (N + down - 1) / down;
  float sum = 0.f;
  for (int j0 = 0; j0 < nref; j0 += KDE_TILE) {
    __syncthreads();
    const int j = j0 + tid;
    if (j < nref) {
      tile[tid] = load(j * down);
      if (HALF) tnorm[tid] = norm_half(tile[tid]);
    }
    __syncthreads();
    const int cnt = min(KDE_TILE, nref - j0);
    for (int t = s; t < cnt; t += KDE_SPLIT) {
      const float4_t r = tile[t];
      if (HALF) {
        sum += term_half(xi, xn, r, tnorm[t], -1.0f / two_var);
        continue;
      }
      const float d0 = xi[0] - r[0], d1 = xi[1] - r[1], d2 = xi[2] - r[2], d3 = xi[3] - r[3];
      const float d2sum = __builtin_fmaf(d3, d3, __builtin_fmaf(d2, d2, __builtin_fmaf(d1, d1, d0 * d0)));
      sum += exp2f(d2sum * neg_scale_log2);
    }
  }
  part[s][qi] = sum;
  __syncthreads();
  if (s == 0 && i < N) density[i] = ((part[0][qi] + part[1][qi]) + part[2][qi]) + part[3][qi];
}

}  // namespace roma
