// Ground-truth warp from two depth maps and a relative pose, and the dense match metrics built on it: warp_kpts / get_gt_warp of the
// reference (romatch/utils/utils.py:326-455) and MegadepthDenseBenchmark.geometric_dist (megadepth_dense_benchmark.py:17-42) fused.
// DESIGN.md §3.4.
//
// The per-point chain is one __device__ function, chain(), used by both kernels.  It follows the reference line for line, in fp64 from
// fp32 key-points and fp32 depths (the reference casts exactly these to double at its call sites):
//   d     = depth_A sampled at the normalised key-point (x, y)            grid_sample: align_corners=False, zero padding
//   px    = (W_A (x + 1) / 2, H_A (y + 1) / 2)
//   X_A   = K_A^-1 (px d, py d, d);  X_B = R X_A + t;  z = X_B.z
//   (u,v) = (K_B X_B).xy / ((K_B X_B).z + 1e-4)
//   covisible = 0 < u < W_B - 1 && 0 < v < H_B - 1                         all strict
//   (x2,y2) = (2 u / W_B - 1, 2 v / H_B - 1);  d_B = depth_B sampled there
//   rel   = |(d_B - z) / d_B|;   valid = d != 0 && covisible && rel < threshold
// Nothing is special-cased: a comparison with NaN is false, a division by a zero depth gives inf, and such a point is not valid.
// mode 2 ("combined", utils.py:393-396) runs the chain with the bilinear and with the nearest sampler and takes the nearest result
// where the bilinear one is not valid and the nearest one is; valid is the OR.
//
// Gather addressing.  A key-point may be NaN, inf or 1e30 and a projection astronomically large, so sample_depth() range-checks the
// un-normalised coordinate IN FLOATING POINT (a negated conjunction, so NaN fails it) and returns 0 before anything is converted to an
// integer; inside the range the four bilinear taps lie in [-1, W] x [-1, H] and each is checked against the map again.  No address
// is formed from an unchecked value.
//
// The pair's constants — K_A^-1 by the adjugate, [R | t], K_B, fp64 — are computed by thread 0 and left in LDS: the pair is a grid
// dimension, so they are uniform over the workgroup.  One thread per point, ITEMS points per thread one after the other.
//
// roma_dense_match_metrics reduces per pair without floating-point atomics and without a "last block" ticket: per-thread sums, a
// wave butterfly, the four waves through LDS in order, one Partial per workgroup into the caller's workspace; a second launch of one
// wave per pair adds the partials in a fixed order.  Bitwise reproducible, and a pair never sees another pair's partials.
#include "common.h"

namespace roma {
namespace {

constexpr int THREADS = 256, ITEMS = 4, POINTS_PER_BLOCK = THREADS * ITEMS;
constexpr int MODE_BILINEAR = 0, MODE_NEAREST = 1, MODE_COMBINED = 2;
constexpr int MAX_SIDE = 32768;                                  // H * W of a map then fits an int

// fp64 per-pair constants, in this order in LDS
struct PairConst {
  double ia[9];                                                  // K_A^-1, row major
  double rt[12];                                                 // [R | t], row major (3,4)
  double kb[9];
};
constexpr int NCONST = sizeof(PairConst) / sizeof(double);

struct Dims {
  int Ha, Wa, Hb, Wb;
};

// what one workgroup of the metrics kernel leaves in the workspace
struct Partial {
  double epe;
  long long n[4];                                                // valid, gd < 1, gd < 3, gd < 5
};

struct Chain {
  double x2, y2, rel;
  bool valid;
};

// thread 0.  A singular K_A gives det = 0: every entry of the inverse is then inf or NaN, every X_A not finite, u and v NaN (inf / inf)
// and no point of the pair covisible.
__device__ void pair_constants(const double* Ka, const double* T, const double* Kb, PairConst& c) {
  const double a = Ka[0], b = Ka[1], cc = Ka[2], d = Ka[3], e = Ka[4], f = Ka[5], g = Ka[6], h = Ka[7], i = Ka[8];
  const double A = e * i - f * h, B = f * g - d * i, C = d * h - e * g;
  const double det = a * A + b * B + cc * C;
  c.ia[0] = A / det; c.ia[1] = (cc * h - b * i) / det; c.ia[2] = (b * f - cc * e) / det;
  c.ia[3] = B / det; c.ia[4] = (a * i - cc * g) / det; c.ia[5] = (cc * d - a * f) / det;
  c.ia[6] = C / det; c.ia[7] = (b * g - a * h) / det;  c.ia[8] = (a * e - b * d) / det;
#pragma unroll
  for (int k = 0; k < 12; ++k) c.rt[k] = T[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) c.kb[k] = Kb[k];
}

// F.grid_sample(depth[None, None], (x, y), align_corners=False, padding_mode="zeros") of one (H,W) map, in fp64.  See "gather
// addressing" above: the range test comes first and NaN fails it.
template <bool NEAREST>
__device__ __forceinline__ double sample_depth(const float* __restrict__ d, int H, int W, double x, double y) {
  const double ix = ((x + 1.0) * (double)W - 1.0) / 2.0, iy = ((y + 1.0) * (double)H - 1.0) / 2.0;
  if (NEAREST) {
    const double rx = rint(ix), ry = rint(iy);                   // ties to even, as nearbyint in ATen
    if (!(rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1))) return 0.0;
    return (double)d[(int)ry * W + (int)rx];
  }
  if (!(ix > -1.0 && ix < (double)W && iy > -1.0 && iy < (double)H)) return 0.0;     // all four taps outside, or NaN
  const double fx = floor(ix), fy = floor(iy);
  const int x0 = (int)fx, y0 = (int)fy;                          // in [-1, W-1], [-1, H-1]
  const double wx1 = ix - fx, wx0 = (fx + 1.0) - ix, wy1 = iy - fy, wy0 = (fy + 1.0) - iy;
  const bool l = x0 >= 0, r = x0 + 1 < W, t = y0 >= 0, b = y0 + 1 < H;
  const int at = y0 * W + x0;
  const double nw = (t && l) ? (double)d[at] : 0.0, ne = (t && r) ? (double)d[at + 1] : 0.0;
  const double sw = (b && l) ? (double)d[at + W] : 0.0, se = (b && r) ? (double)d[at + W + 1] : 0.0;
  return nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
}

template <bool NEAREST>
__device__ __forceinline__ Chain chain(const PairConst& c, const float* __restrict__ da, const float* __restrict__ db, const Dims& dm,
                                       double thr, double x, double y) {
  const double d = sample_depth<NEAREST>(da, dm.Ha, dm.Wa, x, y);
  const double px = (double)dm.Wa * (x + 1.0) / 2.0, py = (double)dm.Ha * (y + 1.0) / 2.0;
  const double h0 = px * d, h1 = py * d;
  const double a0 = c.ia[0] * h0 + c.ia[1] * h1 + c.ia[2] * d, a1 = c.ia[3] * h0 + c.ia[4] * h1 + c.ia[5] * d,
               a2 = c.ia[6] * h0 + c.ia[7] * h1 + c.ia[8] * d;
  const double b0 = c.rt[0] * a0 + c.rt[1] * a1 + c.rt[2] * a2 + c.rt[3], b1 = c.rt[4] * a0 + c.rt[5] * a1 + c.rt[6] * a2 + c.rt[7],
               z = c.rt[8] * a0 + c.rt[9] * a1 + c.rt[10] * a2 + c.rt[11];
  const double p0 = c.kb[0] * b0 + c.kb[1] * b1 + c.kb[2] * z, p1 = c.kb[3] * b0 + c.kb[4] * b1 + c.kb[5] * z,
               p2 = c.kb[6] * b0 + c.kb[7] * b1 + c.kb[8] * z;
  const double den = p2 + 1e-4;
  const double u = p0 / den, v = p1 / den;
  const bool covisible = u > 0.0 && u < (double)(dm.Wb - 1) && v > 0.0 && v < (double)(dm.Hb - 1);
  Chain o;
  o.x2 = 2.0 * u / (double)dm.Wb - 1.0;
  o.y2 = 2.0 * v / (double)dm.Hb - 1.0;
  const double d2 = sample_depth<NEAREST>(db, dm.Hb, dm.Wb, o.x2, o.y2);
  o.rel = fabs((d2 - z) / d2);
  o.valid = d != 0.0 && covisible && o.rel < thr;
  return o;
}

template <int MODE>
__device__ __forceinline__ Chain warp_point(const PairConst& c, const float* __restrict__ da, const float* __restrict__ db, const Dims& dm,
                                            double thr, double x, double y) {
  if (MODE == MODE_BILINEAR) return chain<false>(c, da, db, dm, thr, x, y);
  if (MODE == MODE_NEAREST) return chain<true>(c, da, db, dm, thr, x, y);
  Chain o = chain<false>(c, da, db, dm, thr, x, y);
  const Chain n = chain<true>(c, da, db, dm, thr, x, y);
  if (!o.valid && n.valid) o = n;
  return o;
}

__device__ __forceinline__ void load_constants(const PairConst& s_c, PairConst& c) {
  const double* src = reinterpret_cast<const double*>(&s_c);
  double* dst = reinterpret_cast<double*>(&c);
#pragma unroll
  for (int i = 0; i < NCONST; ++i) dst[i] = src[i];
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void warp_kpts_kernel(const float* __restrict__ x, int stride, const float* __restrict__ depth_a,
                                                            const float* __restrict__ depth_b, const double* __restrict__ T,
                                                            const double* __restrict__ Ka, const double* __restrict__ Kb, int N, Dims dm,
                                                            double thr, double2* __restrict__ x2, unsigned char* __restrict__ valid,
                                                            double* __restrict__ rel) {
  __shared__ PairConst s_c;
  const int p = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) pair_constants(Ka + (size_t)p * 9, T + (size_t)p * 12, Kb + (size_t)p * 9, s_c);
  __syncthreads();
  PairConst c;
  load_constants(s_c, c);
  const float* da = depth_a + (size_t)p * ((size_t)dm.Ha * dm.Wa);
  const float* db = depth_b + (size_t)p * ((size_t)dm.Hb * dm.Wb);
  const size_t row0 = (size_t)p * (size_t)N;                     // 64-bit: P * N may pass 2^31
  const int n0 = blockIdx.x * POINTS_PER_BLOCK + tid;
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {
    const int n = n0 + it * THREADS;
    if (n >= N) break;
    const size_t i = row0 + (size_t)n;
    const float2 q = *reinterpret_cast<const float2*>(x + i * (size_t)stride);
    const Chain o = warp_point<MODE>(c, da, db, dm, thr, (double)q.x, (double)q.y);
    if (x2) x2[i] = make_double2(o.x2, o.y2);
    if (valid) valid[i] = o.valid ? 1 : 0;
    if (rel) rel[i] = o.rel;
  }
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void dense_metrics_kernel(const float4* __restrict__ warp, long pitch4, const float* __restrict__ depth_a,
                                                                const float* __restrict__ depth_b, const double* __restrict__ T,
                                                                const double* __restrict__ Ka, const double* __restrict__ Kb, int H, int W,
                                                                Dims dm, double thr, Partial* __restrict__ part, double* __restrict__ gd_out,
                                                                unsigned char* __restrict__ valid_out) {
  __shared__ PairConst s_c;
  __shared__ double s_sum[THREADS / 64];
  __shared__ int s_cnt[THREADS / 64][4];
  const int p = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) pair_constants(Ka + (size_t)p * 9, T + (size_t)p * 12, Kb + (size_t)p * 9, s_c);
  __syncthreads();
  PairConst c;
  load_constants(s_c, c);
  const float* da = depth_a + (size_t)p * ((size_t)dm.Ha * dm.Wa);
  const float* db = depth_b + (size_t)p * ((size_t)dm.Hb * dm.Wb);
  const float4* wp = warp + (size_t)p * ((size_t)H * (size_t)pitch4);
  const int npix = H * W;
  const size_t row0 = (size_t)p * (size_t)npix;
  const int n0 = blockIdx.x * POINTS_PER_BLOCK + tid;
  const float Wf = (float)W, Hf = (float)H;
  double sum = 0.0;
  int cnt[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {
    const int n = n0 + it * THREADS;
    if (n >= npix) break;
    const int r = n / W, col = n - r * W;
    const float4 q = wp[(size_t)r * (size_t)pitch4 + col];
    const Chain o = warp_point<MODE>(c, da, db, dm, thr, (double)q.x, (double)q.y);
    // the ground truth in fp64, the prediction in fp32 in the reference's order (dense_matches is fp32 there), then widened
    const double gx = (double)W * (o.x2 + 1.0) / 2.0, gy = (double)H * (o.y2 + 1.0) / 2.0;
    const float hx = (Wf * (q.z + 1.f)) / 2.f, hy = (Hf * (q.w + 1.f)) / 2.f;
    const double ex = (double)hx - gx, ey = (double)hy - gy;
    const double gd = sqrt(ex * ex + ey * ey);
    if (o.valid) {
      sum += gd;
      cnt[0] += 1;
      cnt[1] += gd < 1.0;
      cnt[2] += gd < 3.0;
      cnt[3] += gd < 5.0;
    }
    if (gd_out) gd_out[row0 + n] = gd;
    if (valid_out) valid_out[row0 + n] = o.valid ? 1 : 0;
  }
  // every thread arrives here: wave butterfly, waves through LDS in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], o, 64);
  }
  if ((tid & 63) == 0) {
    s_sum[tid >> 6] = sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cnt[tid >> 6][k] = cnt[k];
  }
  __syncthreads();
  if (tid == 0) {
    Partial out = {0.0, {0, 0, 0, 0}};
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
      out.epe += s_sum[w];
#pragma unroll
      for (int k = 0; k < 4; ++k) out.n[k] += s_cnt[w][k];
    }
    part[(size_t)p * gridDim.x + blockIdx.x] = out;
  }
}

// one wave per pair: lane l adds partials l, l + 64, ... in that order, then the butterfly
__global__ __launch_bounds__(64) void dense_metrics_finish_kernel(const Partial* __restrict__ part, int nblocks, double* __restrict__ epe_sum,
                                                                  long long* __restrict__ counts) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const Partial* mine = part + (size_t)p * nblocks;
  double sum = 0.0;
  long long cnt[4] = {0, 0, 0, 0};
  for (int j = lane; j < nblocks; j += 64) {
    sum += mine[j].epe;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += mine[j].n[k];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], o, 64);
  }
  if (lane == 0) {
    epe_sum[p] = sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) counts[(size_t)p * 4 + k] = cnt[k];
  }
}

inline bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_warp_kpts(const float* x, int x_stride, const float* depth_a, const float* depth_b, const double* T, const double* Ka,
                              const double* Kb, int P, int N, int Ha, int Wa, int Hb, int Wb, int mode, double threshold, double* x2,
                              unsigned char* valid, double* rel_err, void* stream) {
  ROMA_REQUIRE(x && depth_a && depth_b && T && Ka && Kb, ROMA_E_ARG, "roma_warp_kpts: null pointer");
  ROMA_REQUIRE(x2 || valid || rel_err, ROMA_E_ARG, "roma_warp_kpts: every output is null");
  ROMA_REQUIRE(P >= 1 && P <= 65535, ROMA_E_SHAPE, "roma_warp_kpts: bad shape P=%d (1 to 65535 pairs)", P);
  ROMA_REQUIRE(N >= 1 && N <= (1 << 28), ROMA_E_SHAPE, "roma_warp_kpts: bad shape N=%d (1 to 2^28 points per pair)", N);
  ROMA_REQUIRE(side_ok(Ha) && side_ok(Wa) && side_ok(Hb) && side_ok(Wb), ROMA_E_SHAPE,
               "roma_warp_kpts: bad shape depth_a %dx%d, depth_b %dx%d (sides 1 to %d)", Ha, Wa, Hb, Wb, MAX_SIDE);
  ROMA_REQUIRE(x_stride == 2 || x_stride == 4, ROMA_E_ARG, "roma_warp_kpts: bad stride %d (2 or 4 floats per row)", x_stride);
  ROMA_REQUIRE(mode >= MODE_BILINEAR && mode <= MODE_COMBINED, ROMA_E_ARG,
               "roma_warp_kpts: unknown mode %d (0 = bilinear, 1 = nearest, 2 = combined)", mode);
  ROMA_REQUIRE(!(threshold != threshold), ROMA_E_ARG, "roma_warp_kpts: threshold must not be NaN");
  ROMA_REQUIRE(aligned8(x) && (!x2 || aligned16(x2)), ROMA_E_ALIGN, "roma_warp_kpts: x must be 8-byte and x2 16-byte aligned");
  const dim3 grid((unsigned)((N + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK), (unsigned)P);
  const Dims dm = {Ha, Wa, Hb, Wb};
  auto kernel = mode == MODE_BILINEAR ? warp_kpts_kernel<MODE_BILINEAR>
                                      : (mode == MODE_NEAREST ? warp_kpts_kernel<MODE_NEAREST> : warp_kpts_kernel<MODE_COMBINED>);
  hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, x_stride, depth_a, depth_b, T, Ka, Kb, N, dm,
                     threshold, reinterpret_cast<double2*>(x2), valid, rel_err);
  ROMA_CHECK_LAUNCH();
}

extern "C" int roma_dense_match_metrics(const float* warp, long pitch, const float* depth_a, const float* depth_b, const double* T,
                                        const double* Ka, const double* Kb, int P, int H, int W, int Ha, int Wa, int Hb, int Wb, int mode,
                                        double threshold, void* workspace, long workspace_bytes, double* epe_sum, long long* counts,
                                        double* gd, unsigned char* valid, void* stream) {
  ROMA_REQUIRE(warp && depth_a && depth_b && T && Ka && Kb && workspace, ROMA_E_ARG, "roma_dense_match_metrics: null pointer");
  ROMA_REQUIRE(epe_sum && counts, ROMA_E_ARG, "roma_dense_match_metrics: null pointer (epe_sum and counts are not optional)");
  ROMA_REQUIRE(P >= 1 && P <= 65535, ROMA_E_SHAPE, "roma_dense_match_metrics: bad shape P=%d (1 to 65535 pairs)", P);
  ROMA_REQUIRE(side_ok(H) && side_ok(W) && (long)H * W <= (1L << 28), ROMA_E_SHAPE,
               "roma_dense_match_metrics: bad shape warp %dx%d (sides 1 to %d, at most 2^28 pixels)", H, W, MAX_SIDE);
  ROMA_REQUIRE(side_ok(Ha) && side_ok(Wa) && side_ok(Hb) && side_ok(Wb), ROMA_E_SHAPE,
               "roma_dense_match_metrics: bad shape depth_a %dx%d, depth_b %dx%d (sides 1 to %d)", Ha, Wa, Hb, Wb, MAX_SIDE);
  ROMA_REQUIRE(pitch >= 4L * W && pitch % 4 == 0, ROMA_E_ARG,
               "roma_dense_match_metrics: bad stride: a row pitch of %ld floats (a multiple of 4, at least 4 W = %ld)", pitch, 4L * W);
  ROMA_REQUIRE(mode >= MODE_BILINEAR && mode <= MODE_COMBINED, ROMA_E_ARG,
               "roma_dense_match_metrics: unknown mode %d (0 = bilinear, 1 = nearest, 2 = combined)", mode);
  ROMA_REQUIRE(!(threshold != threshold), ROMA_E_ARG, "roma_dense_match_metrics: threshold must not be NaN");
  const int nblocks = (H * W + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK;
  const long need = (long)P * nblocks * (long)sizeof(Partial);
  ROMA_REQUIRE(workspace_bytes >= need, ROMA_E_ARG, "roma_dense_match_metrics: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  ROMA_REQUIRE(aligned16(warp) && aligned8(workspace), ROMA_E_ALIGN,
               "roma_dense_match_metrics: warp must be 16-byte and the workspace 8-byte aligned");
  const Dims dm = {Ha, Wa, Hb, Wb};
  hipStream_t s = static_cast<hipStream_t>(stream);
  Partial* part = static_cast<Partial*>(workspace);
  auto kernel = mode == MODE_BILINEAR ? dense_metrics_kernel<MODE_BILINEAR>
                                      : (mode == MODE_NEAREST ? dense_metrics_kernel<MODE_NEAREST> : dense_metrics_kernel<MODE_COMBINED>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks, (unsigned)P), dim3(THREADS), 0, s, reinterpret_cast<const float4*>(warp), pitch / 4,
                     depth_a, depth_b, T, Ka, Kb, H, W, dm, threshold, part, gd, valid);
  hipLaunchKernelGGL(dense_metrics_finish_kernel, dim3((unsigned)P), dim3(64), 0, s, part, nblocks, epe_sum, counts);
  ROMA_CHECK_LAUNCH();
}
