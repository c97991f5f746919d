// The two halves of a mid-width ConvRefiner block (matcher.py:77-103) as device functions, defined once for the kernels that run
// them: the depthwise strip body of dwconv5x5_lds_kernel (dwconv.hip) and the MFMA row-group step of pointwise_mfma_kernel
// (refiner_block.hip), both also the two phases of refiner_mid_kernel (refiner_mid.hip).  One definition is what makes the
// one-launch block bit-identical to the two calls: same expressions, same order of the fp32 sums, same roundings.
#pragma once
#include <type_traits>
#include "common.h"

namespace roma {
namespace mid {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef __bf16 b8v __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float4_t mfma16x32(const u32x4& a, const u32x4& b, float4_t c, half_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma16x32(const u32x4& a, const u32x4& b, float4_t c, bf16_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8v, a), __builtin_bit_cast(b8v, b), c, 0, 0, 0);
}

constexpr int kStrip = 8;                                          // output pixels of a strip

// Depthwise 5x5 + BN + ReLU of one strip: output pixels (b, ys, xs .. xs + 7) of the 16-byte channel packet at channel c0, 16-bit
// activations.  s_w: the fp32 taps [25][C] in LDS.  The sums run over input rows 0..4, columns ascending, taps by o = cx - dx, in
// fp32 fmaf; BN is one fmaf, then fmaxf and the pack.  emit(o, packet) receives outputs o = 0 .. min(n_out, 8) - 1.
// The interior / border choice is uniform over the wave's active lanes.
constexpr int kStripCols = kStrip + 4;                             // input columns of a strip

__device__ __forceinline__ bool dw_interior(int ys, int xs, int H, int W) {   // all but a 2-pixel frame: no clamped or masked tap
  return ys >= 2 && ys + 3 <= H && xs >= 2 && xs + kStrip + 2 <= W;
}

// byte offset of (b, row ys - 2, column xs - 2, channel c0) from x in 32 bits (the host checks the tensor is < 4 GB)
__device__ __forceinline__ unsigned dw_row0_offset(int b, int ys, int xs, int c0, int H, int W, int x_pitch) {
  return (unsigned)((((size_t)b * H + ys - 2) * W + xs - 2) * x_pitch + c0) * 2u;
}

template <typename T, typename Emit>
__device__ __forceinline__ void dw_strip(const T* __restrict__ x, const float* s_w, const float* __restrict__ scale,
                                         const float* __restrict__ shift, int b, int ys, int xs, int c0, int C, int H, int W,
                                         int x_pitch, int n_out, Emit&& emit) {
  constexpr int E = 8, XS = kStrip, NC = kStripCols;
  static_assert(sizeof(T) == 2, "16-bit activations");
  float acc[XS][E];
#pragma unroll
  for (int o = 0; o < XS; ++o)
#pragma unroll
    for (int e = 0; e < E; ++e) acc[o][e] = 0.f;
  const bool interior = dw_interior(ys, xs, H, W);
  // 5 taps x 8 channels of fused multiply-adds for every column of one input row (taps of tap-row iy from LDS)
  auto fma_row = [&](const u32x4 (&src)[NC], int iy, auto masked_c) {
    const int yi = ys + iy - 2;
    const float my = (yi >= 0 && yi < H) ? 1.f : 0.f;
    const float* wr = s_w + (size_t)iy * 5 * C + c0;
    float wv[5][E];
#pragma unroll
    for (int dx = 0; dx < 5; ++dx)
#pragma unroll
      for (int e = 0; e < E; e += 4) *reinterpret_cast<float4_t*>(&wv[dx][e]) = *reinterpret_cast<const float4_t*>(wr + dx * C + e);
#pragma unroll
    for (int cx = 0; cx < NC; ++cx) {
      float f[E];
      unpack16<T>(src[cx], f);
      if constexpr (decltype(masked_c)::value) {
        const int xi = xs - 2 + cx;
        const float m = (xi >= 0 && xi < W) ? my : 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] *= m;
      }
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int o = cx - dx;
        if (o >= 0 && o < XS) {
#pragma unroll
          for (int e = 0; e < E; ++e) acc[o][e] = __builtin_fmaf(wv[dx][e], f[e], acc[o][e]);
        }
      }
    }
  };
  if (__all(interior)) {                                         // wave-uniform: a wave with one border strip takes the border path whole
    // all but a 2-pixel frame.  Byte offset of (b, row, column xs - 2, packet k) from x in 32 bits (the host checks the tensor is
    // < 4 GB); the 12 columns of a row are the uniform distances cx * x_pitch * 2 from it: a load is scalar base + one vector
    // offset.  Software pipeline: row iy + 1 is requested before row iy is multiplied.  (hipcc converts the whole row to fp32
    // first — 96 registers — and then issues the 12 loads back to back; pinning a finer interleave needs more registers, not fewer.)
    unsigned voff = dw_row0_offset(b, ys, xs, c0, H, W, x_pitch);
    const unsigned vstep = (unsigned)W * x_pitch * 2u;
    auto load_row = [&](u32x4 (&dst)[NC]) {
#pragma unroll
      for (int cx = 0; cx < NC; ++cx)
        dst[cx] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(x) + (size_t)cx * x_pitch * 2 + voff);
      voff += vstep;
    };
    u32x4 cur[NC], nxt[NC];
    load_row(nxt);
#pragma unroll 1
    for (int iy = 0; iy < 4; ++iy) {
#pragma unroll
      for (int cx = 0; cx < NC; ++cx) cur[cx] = nxt[cx];
      load_row(nxt);
      fma_row(cur, iy, std::false_type{});
    }
    fma_row(nxt, 4, std::false_type{});
  } else {
    // border strips: clamped addresses, taps zeroed through a mask, one row at a time
#pragma unroll 1
    for (int iy = 0; iy < 5; ++iy) {
      const T* row = x + ((size_t)b * H + min(max(ys + iy - 2, 0), H - 1)) * W * x_pitch + c0;
      u32x4 cur[NC];
#pragma unroll
      for (int cx = 0; cx < NC; ++cx) cur[cx] = *reinterpret_cast<const u32x4*>(row + (size_t)min(max(xs - 2 + cx, 0), W - 1) * x_pitch);
      fma_row(cur, iy, std::true_type{});
    }
  }
  float sc[E], sh[E];
#pragma unroll
  for (int e = 0; e < E; e += 4) {
    *reinterpret_cast<float4_t*>(&sc[e]) = *reinterpret_cast<const float4_t*>(scale + c0 + e);
    *reinterpret_cast<float4_t*>(&sh[e]) = *reinterpret_cast<const float4_t*>(shift + c0 + e);
  }
#pragma unroll
  for (int o = 0; o < XS; ++o) {
    if (o >= n_out) break;
    float v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = fmaxf(__builtin_fmaf(acc[o][e], sc[e], sh[e]), 0.f);
    emit(o, pack16<T>(v));
  }
}

// The 1x1 of G groups of 16 pixel rows on the matrix cores: out[row][n] = bias[n] + sum_k a[row][k] * wt[n][k], K summed in KP
// 32-wide MFMA steps in ascending order, the bias added in fp32, one rounding.  Lane (m = lane & 15, kq = lane >> 4) holds in
// a[g][ks] the packet 4 ks + kq of row m of group g (zero past the last real packet); s_pw: the weights [32 KP][4 KP + 1] packets
// in LDS (odd row stride), s_b the fp32 bias.  The results of group g are staged at so[g] as [16 rows][32 KP + 8] elements; a
// weight fragment is read once for all G groups.
template <typename T, int KP, int G>
__device__ __forceinline__ void pw_row_groups(const u32x4 (&a)[G][KP], const u32x4* s_pw, const float* s_b, T* const (&so)[G],
                                              int m, int kq) {
  constexpr int KPAD = 32 * KP, NT = KPAD / 16, RS = KPAD / 8 + 1, OS = KPAD + 8;
  float4_t acc[G][NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g][nt] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KP; ++ks) {
      const u32x4 bfrag = s_pw[(nt * 16 + m) * RS + 4 * ks + kq];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g][nt] = mfma16x32(a[g][ks], bfrag, acc[g][nt], T{});
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float bv = s_b[nt * 16 + m];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) so[g][(4 * kq + r4) * OS + nt * 16 + m] = from_f32<T>(acc[g][nt][r4] + bv);
  }
}

}  // namespace mid
}  // namespace roma
