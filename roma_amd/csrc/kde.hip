// Gaussian kernel density for sample() — reference: romatch/utils/kde.py:4-12 (called at matcher.py:489):
//   density[i] = sum_j exp(-|x_i - x_j|^2 / (2 std^2)),  x: (N,4) match coordinates, ref points every `down`-th row.
// The reference materialises the N x N distance matrix (3.2 GB in half for N = 40 000); here nothing is
// materialised: 320 KB in, 160 KB out, exp-bound.  A workgroup owns 64 query points x 4 interleaved quarters of each
// staged 256-point reference tile; the four partial sums are combined through LDS in a fixed order, so the result is
// bitwise reproducible (no atomics).
#include "common.h"
#include "sample_device.h"

namespace roma {
namespace {

constexpr int QP = KDE_QP;

// the term, the norm and the summation order live in sample_device.h (kde_body), shared with the batched kernel of sample_batch.hip
struct PackedPoints {
  const float4_t* x;
  __device__ __forceinline__ float4_t operator()(int j) const { return x[j]; }
};

template <bool HALF>
__global__ __launch_bounds__(256) void kde_kernel(const float4_t* __restrict__ x, float* __restrict__ density, int N, int down,
                                                  float neg_scale_log2, float two_var) {
  kde_body<HALF>(PackedPoints{x}, density, blockIdx.x, N, down, neg_scale_log2, two_var);
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_kde_density(const float* x, float* density, int N, int down, float std, int half_mode, void* stream) {
  ROMA_REQUIRE(x && density, ROMA_E_ARG, "roma_kde_density: null pointer");
  ROMA_REQUIRE(N > 0 && down >= 1 && std > 0.f, ROMA_E_SHAPE, "roma_kde_density: bad arguments N=%d down=%d std=%g", N, down, std);
  ROMA_REQUIRE(aligned16(x), ROMA_E_ALIGN, "roma_kde_density: x must be 16-byte aligned");
  const float neg_scale_log2 = -1.4426950408889634f / (2.f * std * std);
  const float two_var = (float)(2.0 * (double)std * (double)std);
  if (half_mode)
    hipLaunchKernelGGL(kde_kernel<true>, dim3((N + QP - 1) / QP), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4_t*>(x), density, N, down, neg_scale_log2, two_var);
  else
    hipLaunchKernelGGL(kde_kernel<false>, dim3((N + QP - 1) / QP), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4_t*>(x), density, N, down, neg_scale_log2, two_var);
  ROMA_CHECK_LAUNCH();
}
