// 1x1 convolution for NARROW channels-last activations (C <= 32) — the back half of a ConvRefiner block
// (romatch/models/matcher.py:102, Conv2d(D, D, 1)) at the two finest scales, where D = 24 and M = h*w*B is 0.6-1.5 M rows.
// hipBLASLt runs this skinny GEMM (N = K = 24) at 0.65 TB/s (212 us at 864x864); it is a pure streaming op:
//   y[m][n] = b[n] + sum_k x[m][k] * wt[k][n]
// One thread per pixel row: the row's packets are loaded once (16-byte loads), the K x N fp32 weights are wave-uniform
// (scalar loads through the constant cache), fp32 accumulate, 16-byte stores.
#include "common.h"

namespace roma {
namespace {

template <typename T, int NP>   // NP = number of 16-byte packets per row (C = NP * elements-per-packet)
__global__ __launch_bounds__(256) void pointwise_small_kernel(const T* __restrict__ x, const float* __restrict__ wt,
                                                             const float* __restrict__ bias, T* __restrict__ y, size_t M,
                                                             int x_pitch, int y_pitch) {
  constexpr int E = ElemTraits<T>::kPer16B;
  constexpr int C = NP * E;
  for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (size_t)gridDim.x * blockDim.x) {
    float xin[C];
#pragma unroll
    for (int pk = 0; pk < NP; ++pk) unpack16<T>(*reinterpret_cast<const u32x4*>(x + m * x_pitch + pk * E), xin + pk * E);
    float acc[C];
#pragma unroll
    for (int n = 0; n < C; ++n) acc[n] = bias[n];
#pragma unroll
    for (int k = 0; k < C; ++k)
#pragma unroll
      for (int n = 0; n < C; ++n) acc[n] = __builtin_fmaf(xin[k], wt[k * C + n], acc[n]);
#pragma unroll
    for (int pk = 0; pk < NP; ++pk) *reinterpret_cast<u32x4*>(y + m * y_pitch + pk * E) = pack16<T>(acc + pk * E);
  }
}

// ---- The decoder's 1x1 projections at the two finest scales (matcher.py:366-371: Conv2d(K, N, 1) + BatchNorm, folded), K = 64 -> N = 9
// and K = 128 -> N = 64, over M = 10^5 .. 10^6 channels-last pixels: out[m][0:N] = bias + x[m][0:K] @ wt.  The GEMM library runs these
// skinny shapes at about 1 TB/s of in + out; they are streaming ops, built here like pointwise_mfma_kernel (refiner_block.hip): the
// weights sit in LDS once per persistent workgroup, every wavefront takes 16 rows at a time, its A fragments are the rows' 16-byte
// packets straight from global memory (the next tile's are requested before this tile's products), N is padded to whole 16-column
// MFMA tiles, and the results go through a wave-private LDS patch so that a row leaves as 16-byte stores plus N % 8 single elements.
// No workgroup barrier after the weight load. ----
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef __bf16 b8v __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float4_t mfma_16x16x32(const u32x4& a, const u32x4& b, float4_t c, half_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), c, 0, 0, 0);
}
__device__ __forceinline__ float4_t mfma_16x16x32(const u32x4& a, const u32x4& b, float4_t c, bf16_t) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8v, a), __builtin_bit_cast(b8v, b), c, 0, 0, 0);
}

struct PSParams {
  const void* x;      // (M, x_pitch) T
  const void* wt;     // (16 NT, 32 KS) T: wt[n][k], rows n >= N zero
  const float* bias;  // (16 NT)
  void* y;            // (M, y_pitch) T; columns [0, N) of every row are written
  long M;
  int N, x_pitch, y_pitch;
};

template <typename T, int KS, int NT>
__global__ __launch_bounds__(256) void project_skinny_kernel(PSParams p) {
  constexpr int K = 32 * KS, NP = 16 * NT, RS = K / 8 + 1, OS = NP + 8;
  __shared__ u32x4 s_w[NP * RS];                                   // [n][k packet], odd row stride
  __shared__ float s_b[NP];
  __shared__ __attribute__((aligned(16))) T s_out[4 * 16 * OS];    // [wave][row][n]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  for (int i = tid; i < NP * (K / 8); i += 256) {
    const int n = i / (K / 8), k = i % (K / 8);
    s_w[n * RS + k] = reinterpret_cast<const u32x4*>(p.wt)[i];
  }
  for (int i = tid; i < NP; i += 256) s_b[i] = p.bias[i];
  __syncthreads();
  const T* x = static_cast<const T*>(p.x);
  T* y = static_cast<T*>(p.y);
  T* so = s_out + wv * 16 * OS;
  const int PKT = p.N / 8, REM = p.N % 8;
  const long ntile = (p.M + 15) / 16, step = (long)gridDim.x * 4;
  auto fetch = [&](long tile, u32x4* a) {                          // rows past M repeat the last row; their results are not stored
    const long r = tile * 16 + m < p.M ? tile * 16 + m : p.M - 1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = *reinterpret_cast<const u32x4*>(x + r * p.x_pitch + (4 * ks + kq) * 8);
  };
  long tile = (long)blockIdx.x * 4 + wv;
  u32x4 a[KS], a_next[KS];
  if (tile < ntile) fetch(tile, a_next);
  for (; tile < ntile; tile += step) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = a_next[ks];
    if (tile + step < ntile) fetch(tile + step, a_next);
    const long row0 = tile * 16;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float4_t acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = mfma_16x16x32(a[ks], s_w[(nt * 16 + m) * RS + 4 * ks + kq], acc, T{});
      const float bv = s_b[nt * 16 + m];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) so[(4 * kq + r4) * OS + nt * 16 + m] = from_f32<T>(acc[r4] + bv);
    }
    for (int i = lane; i < 16 * PKT; i += 64) {
      const int row = i / PKT, k = i - row * PKT;
      if (row0 + row < p.M) *reinterpret_cast<u32x4*>(y + (row0 + row) * p.y_pitch + k * 8) = *reinterpret_cast<const u32x4*>(so + row * OS + k * 8);
    }
    for (int i = lane; i < 16 * REM; i += 64) {
      const int row = i / REM, e = PKT * 8 + (i - row * REM);
      if (row0 + row < p.M) y[(row0 + row) * p.y_pitch + e] = so[row * OS + e];
    }
  }
}

template <typename T, int KS, int NT>
int launch_ps(const PSParams& p, hipStream_t s) {
  const long need = (p.M + 63) / 64;
  const long cap = 4L * num_cus();                                 // persistent: four workgroups per CU (27 KB of LDS each at most)
  hipLaunchKernelGGL((project_skinny_kernel<T, KS, NT>), dim3((int)(need < cap ? need : cap)), dim3(256), 0, s, p);
  ROMA_CHECK_LAUNCH();
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_project_skinny(const void* x, const void* wt, const float* bias, void* y, long M, int K, int N, int dtype, int x_pitch,
                                   int y_pitch, void* stream) {
  ROMA_REQUIRE(x && wt && bias && y, ROMA_E_ARG, "roma_project_skinny: null pointer");
  ROMA_REQUIRE(M > 0 && K > 0 && N > 0 && x_pitch >= K && y_pitch >= N, ROMA_E_SHAPE, "roma_project_skinny: bad shape");
  ROMA_REQUIRE(dtype == ROMA_F16 || dtype == ROMA_BF16, ROMA_E_DTYPE, "roma_project_skinny: fp16 / bf16 only");
  ROMA_REQUIRE((K == 64 && N == 9) || (K == 128 && N == 64), ROMA_E_UNSUPPORTED, "roma_project_skinny: (K, N) = (%d, %d), not (64, 9) or (128, 64)", K, N);
  ROMA_REQUIRE(x_pitch % 8 == 0 && y_pitch % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(wt), ROMA_E_ALIGN,
               "roma_project_skinny: pitches must be multiples of 8 and bases 16-byte aligned");
  PSParams p{x, wt, bias, y, M, N, x_pitch, y_pitch};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == ROMA_F16) return K == 64 ? launch_ps<half_t, 2, 1>(p, s) : launch_ps<half_t, 4, 4>(p, s);
  return K == 64 ? launch_ps<bf16_t, 2, 1>(p, s) : launch_ps<bf16_t, 4, 4>(p, s);
}

extern "C" int roma_pointwise_small(const void* x, const float* wt, const float* bias, void* y, long M, int C, int dtype, int x_pitch,
                                    int y_pitch, void* stream) {
  ROMA_REQUIRE(x && wt && bias && y, ROMA_E_ARG, "roma_pointwise_small: null pointer");
  ROMA_REQUIRE(M > 0 && C > 0 && x_pitch >= C && y_pitch >= C, ROMA_E_SHAPE, "roma_pointwise_small: bad shape");
  ROMA_REQUIRE(dtype >= ROMA_F32 && dtype <= ROMA_BF16, ROMA_E_DTYPE, "roma_pointwise_small: unknown dtype %d", dtype);
  const int e = dtype == ROMA_F32 ? 4 : 8;
  ROMA_REQUIRE(C % e == 0 && C <= 32 && x_pitch % e == 0 && y_pitch % e == 0 && aligned16(x) && aligned16(y), ROMA_E_ALIGN,
               "roma_pointwise_small: C must be a multiple of %d and <= 32, pitches multiples of %d, bases 16-byte aligned", e, e);
  hipStream_t s = static_cast<hipStream_t>(stream);
  size_t g = ((size_t)M + 255) / 256;
  if (g > 16384) g = 16384;
  const int np = C / e;
#define ROMA_PW(T, NP)                                                                                                        \
  hipLaunchKernelGGL((pointwise_small_kernel<T, NP>), dim3((int)g), dim3(256), 0, s, (const T*)x, wt, bias, (T*)y, (size_t)M, \
                     x_pitch, y_pitch)
#define ROMA_PW_T(T)                                                              \
  switch (np) {                                                                   \
    case 1: ROMA_PW(T, 1); break;                                                 \
    case 2: ROMA_PW(T, 2); break;                                                 \
    case 3: ROMA_PW(T, 3); break;                                                 \
    case 4: ROMA_PW(T, 4); break;                                                 \
    case 5: if constexpr (sizeof(T) == 4) { ROMA_PW(T, 5); } break;               \
    case 6: if constexpr (sizeof(T) == 4) { ROMA_PW(T, 6); } break;               \
    case 7: if constexpr (sizeof(T) == 4) { ROMA_PW(T, 7); } break;               \
    case 8: if constexpr (sizeof(T) == 4) { ROMA_PW(T, 8); } break;               \
  }
  if (dtype == ROMA_F32) { ROMA_PW_T(float) } else if (dtype == ROMA_F16) { ROMA_PW_T(half_t) } else { ROMA_PW_T(bf16_t) }
#undef ROMA_PW_T
#undef ROMA_PW
  ROMA_CHECK_LAUNCH();
}
