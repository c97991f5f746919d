// Non-linear refinement of a homography: Levenberg-Marquardt on the truncated forward-transfer cost of the pixel matches — the polish
// that cv2.findHomography(..., cv2.RANSAC, ...) runs on the inliers after consensus (the call of the reference's HPatches benchmark,
// romatch/benchmarks/hpatches_sequences_homog_benchmark.py:80-86, which then scores the mean distance of the four warped corners),
// and that geometry.hip's select_kernel<KIND_H>, which stops at an algebraic DLT refit, does not.  Pipeline: find_homography ->
// refine_homography.  Ground rules of DESIGN.md §3.4, as pose_refine.hip and fundamental_refine.hip: fp64, nothing allocated, no
// atomics, no host synchronisation, sums in a fixed order, so the output is bitwise reproducible and a pair's result does not depend
// on the rest of the batch.  tests/homography_refine_ref.py restates it in numpy.
//
// One workgroup of 256 threads per pair runs the whole schedule in one launch.  Every thread holds the model, the damping and the
// reduced sums (block-uniform: every thread computes the same values from the same reduced sums); the only communication is the
// reduction (a wave butterfly, then the four waves summed in order through LDS) and the staging of the input model through LDS.
//
//   residual    r = (x', y') - x_B, (x', y') = (H x_A)_{1,2} / (H x_A)_3, e = r_x^2 + r_y^2 in the pixels of image B: what
//               find_homography scores with (in fp32 there).  A match whose e is not finite (w = 0) is an outlier
//   cost        sum of min(e, thr^2) over the usable matches (finite, allowed by mask_in); weight 1 where e < thr^2, else 0
//   coordinates Hartley: x^ = (x - c) s per image, centroid and mean distance sqrt 2 over the usable matches, computed here
//   model       H^ = T_B H T_A^-1 scaled to unit Frobenius norm.  8 parameters: the entries of H^ but the one of largest magnitude
//               (lowest index on ties), which is held; it is at least 1/3, so this gauge does not degenerate as h22 = 1 does for a
//               normalised H with a small corner entry.  The held entry is chosen again at every Jacobian pass.  The model in
//               pixels is T_B^-1 H^ T_A with H[2,2] = 1 (unit Frobenius norm where |H[2,2]| < 1e-12 |H|: find_homography's
//               convention): the cost that accepts a step is the cost of exactly the nine numbers that are returned
//   Jacobian    analytic, in normalised coordinates (threshold scaled by s_B), with a = (x^, y^, 1) / w:
//               dx'/dh^ = (a, 0, -x' a), dy'/dh^ = (0, a, -y' a).  By this zero pattern the 9 x 9 normal matrix is
//               [S_1, 0, -S_x'; 0, S_1, -S_y'; ., ., S_q] with S_f = sum of f a a^T, q = x'^2 + y'^2: 4 x 6 sums, and 9 of J^T r,
//               33 in all, whichever entry is held; the held row and column are dropped after the reduction
//   passes      a COST pass (2 sums: cost, count) for the input and for every candidate, in pixels; a JACOBIAN pass (33 sums) at
//               the start and after a kept step only.  A pass reads the pair's matches again (32 N bytes, they stay in the L2)
//   one step    (A + lambda diag A) delta = -g by an 8 x 8 Cholesky in registers, H^ <- unit(H^ + delta).  Kept when cost' < cost
//               (1 - 1e-12), then lambda <- max(lambda / 10, 1e-10); else lambda <- 10 lambda.  lambda_0 = 1e-3; at most `iters`
//               steps; a step that moves no bit of H^ ends the schedule
//   unchanged   no kept step, fewer than 4 weighted matches under the input, a Cholesky pivot that is not positive, an input that
//               is not finite or is all zero: the input is returned bit for bit, with its own mask, cost and count, and steps = 0
//
// Shared, in twoview_math.h: Match, load_pixels, the normalisation, block_sum, solve_step and the checks of the entry point with the
// other two refinements; Norm and times_t_a with geometry.hip's select_kernel.
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int RH_THREADS = 256, RH_WAVES = RH_THREADS / 64;
constexpr int RH_NPAR = 8, RH_NTRI = 36;
constexpr int RH_S1 = 0, RH_SX = 6, RH_SY = 12, RH_SQ = 18, RH_G = 24, RH_NSUM = 33;   // 4 x 6 of sum f a a^T, 9 of J^T r
constexpr int RH_MIN_MATCHES = 4;
constexpr double RH_LAMBDA0 = 1e-3, RH_LAMBDA_MIN = 1e-10, RH_ACCEPT_REL = 1e-12;

// forward transfer of (x, y) by m against (u, v): e = r_x^2 + r_y^2, r = p - (u, v), p = (m x)_{0,1} iw, iw = 1 / (m x)_2.  Every
// operation is written out, so the passes that use it agree bit for bit.  NaN or inf where w = 0 or the match is not finite
__device__ __forceinline__ double transfer_error(const double* m, double x, double y, double u, double v, double& iw, double& px,
                                                 double& py, double& rx, double& ry) {
  const double hx = __builtin_fma(m[0], x, __builtin_fma(m[1], y, m[2]));
  const double hy = __builtin_fma(m[3], x, __builtin_fma(m[4], y, m[5]));
  const double hw = __builtin_fma(m[6], x, __builtin_fma(m[7], y, m[8]));
  iw = 1.0 / hw;
  px = hx * iw;
  py = hy * iw;
  rx = __builtin_fma(hx, iw, -u);
  ry = __builtin_fma(hy, iw, -v);
  return __builtin_fma(rx, rx, ry * ry);
}

// o = T_B f T_A^-1: normalised coordinates from pixels
__device__ __forceinline__ void to_normalised(const double* f, const Norm& n, double* o) {
  double g[9];
  const double iA = 1.0 / n.sA;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = f[3 * r] * iA;
    g[3 * r + 1] = f[3 * r + 1] * iA;
    g[3 * r + 2] = f[3 * r + 2] + (n.cxA * f[3 * r] + n.cyA * f[3 * r + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o[j] = n.sB * (g[j] - n.cxB * g[6 + j]);
    o[3 + j] = n.sB * (g[3 + j] - n.cyB * g[6 + j]);
    o[6 + j] = g[6 + j];
  }
}

// o = finish(T_B^-1 c T_A): the H in pixels as it is returned, with H[2,2] = 1, or unit Frobenius norm where |H[2,2]| < 1e-12 |H|.
// Step 3 of geometry.hip's select_kernel<KIND_H>, expression by expression (that kernel keeps its own statements, so that its
// instructions and with them the bits of find_homography stay what they were).  T_B^-1 g: rows 0,1 = row / sB + cB * row 2
__device__ __forceinline__ void homography_to_pixels(const double* c, const Norm& n, double* o) {
  double g[9];
  times_t_a(c, n, g);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o[j] = g[j] / n.sB + n.cxB * g[6 + j];
    o[3 + j] = g[3 + j] / n.sB + n.cyB * g[6 + j];
    o[6 + j] = g[6 + j];
  }
  double fro = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) fro += o[i] * o[i];
  fro = sqrt(fro);
  if (fabs(o[8]) < 1e-12 * fro) {
    unit_frobenius(o);
  } else {
    const double inv = 1.0 / o[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] *= inv;
    o[8] = 1.0;
  }
}

// cost and inlier count of the pixel model f over the pair's matches, reduced
__device__ __forceinline__ void cost_pass(const double* f, const double2* __restrict__ xa, const double2* __restrict__ xb,
                                          const unsigned char* mask_in, size_t base, int N, double t2, double (*red)[RH_NSUM],
                                          double& cost, double& count) {
  double c[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < N; i += RH_THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    double iw, px, py, rx, ry;
    const double e = transfer_error(f, m.x, m.y, m.u, m.v, iw, px, py, rx, ry);
    const bool in = m.ok && e < t2;
    c[0] += m.ok ? (in ? e : t2) : 0.0;
    c[1] += in ? 1.0 : 0.0;
  }
  block_sum<2, RH_WAVES>(c, red);
  cost = c[0];
  count = c[1];
}

// the 33 sums of the normalised model h over the pair's matches, reduced; t2 is the threshold^2 in the normalised image B
__device__ __forceinline__ void jacobian_pass(const double* h, const Norm& n, const double2* __restrict__ xa,
                                              const double2* __restrict__ xb, const unsigned char* mask_in, size_t base, int N, double t2,
                                              double (*red)[RH_NSUM], double (&s)[RH_NSUM]) {
#pragma unroll
  for (int k = 0; k < RH_NSUM; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < N; i += RH_THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    const double x = (m.x - n.cxA) * n.sA, y = (m.y - n.cyA) * n.sA, u = (m.u - n.cxB) * n.sB, v = (m.v - n.cyB) * n.sB;
    double iw, px, py, rx, ry;
    const double e = transfer_error(h, x, y, u, v, iw, px, py, rx, ry);
    const bool in = m.ok && e < t2;
    // a match without weight adds exact zeros (its terms may be NaN or inf)
    const double a[3] = {in ? x * iw : 0.0, in ? y * iw : 0.0, in ? iw : 0.0};
    px = in ? px : 0.0; py = in ? py : 0.0; rx = in ? rx : 0.0; ry = in ? ry : 0.0;
    const double q = __builtin_fma(px, px, py * py), d = -__builtin_fma(px, rx, py * ry);
    int o = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int l = j; l < 3; ++l, ++o) {
        const double aa = a[j] * a[l];
        s[RH_S1 + o] += aa;
        s[RH_SX + o] = __builtin_fma(px, aa, s[RH_SX + o]);
        s[RH_SY + o] = __builtin_fma(py, aa, s[RH_SY + o]);
        s[RH_SQ + o] = __builtin_fma(q, aa, s[RH_SQ + o]);
      }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s[RH_G + j] = __builtin_fma(a[j], rx, s[RH_G + j]);
      s[RH_G + 3 + j] = __builtin_fma(a[j], ry, s[RH_G + 3 + j]);
      s[RH_G + 6 + j] = __builtin_fma(a[j], d, s[RH_G + 6 + j]);
    }
  }
  block_sum<RH_NSUM, RH_WAVES>(s, red);
}

// entry (i, j), i <= j, of the 9 x 9 normal matrix from the sums; i and j are compile-time constants where it is called
__device__ __forceinline__ double normal_entry(const double* s, int i, int j) {
  const int bi = i / 3, bj = j / 3, a = i % 3, b = j % 3;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int t = 3 * lo - lo * (lo - 1) / 2 + (hi - lo);        // (lo, hi) in the order 00 01 02 11 12 22
  if (bi == bj) return bi == 2 ? s[RH_SQ + t] : s[RH_S1 + t];
  if (bj == 2) return bi == 0 ? -s[RH_SX + t] : -s[RH_SY + t];
  return 0.0;
}

// the upper triangle and the gradient of the 8 parameters: row and column `held` of the 9 x 9 system dropped.  Selects between
// compile-time entries read into values first, so that everything stays in registers (a conditional between two array elements
// selects the address, and the sums go to scratch)
__device__ __forceinline__ void drop_held(const double* s, int held, double* tri, double* g) {
  int o = 0;
#pragma unroll
  for (int a = 0; a < RH_NPAR; ++a) {
#pragma unroll
    for (int b = a; b < RH_NPAR; ++b, ++o) {
      const double both = normal_entry(s, a, b), row = normal_entry(s, a, b + 1), none = normal_entry(s, a + 1, b + 1);
      tri[o] = held > b ? both : (held > a ? row : none);
    }
    const double lo = s[RH_G + a], hi = s[RH_G + a + 1];
    g[a] = held > a ? lo : hi;
  }
}

__global__ __launch_bounds__(RH_THREADS) void refine_homography_kernel(const double2* __restrict__ xa, const double2* __restrict__ xb,
                                                                       const double* __restrict__ H_in, const unsigned char* mask_in,
                                                                       int N, double t2, int iters, double* __restrict__ H_out,
                                                                       unsigned char* __restrict__ mask_out,
                                                                       double* __restrict__ cost_out, int* __restrict__ count_out,
                                                                       int* __restrict__ steps_out) {
  __shared__ double red[RH_WAVES][RH_NSUM], fin[9];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  // the input model goes through LDS, so that every thread holds it in vector registers
  if (tid < 9) fin[tid] = H_in[p * 9 + tid];
  __syncthreads();
  double f0[9];
  bool good = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { f0[i] = fin[i]; good = good && isfinite(f0[i]); }

  const Norm nrm = normalisation<RH_THREADS>(xa, xb, mask_in, base, N, red);
  const double t2n = t2 * (nrm.sB * nrm.sB);

  // the start: H^ = T_B H T_A^-1 of unit Frobenius norm (all zero for a zero H, or one whose norm overflows)
  double h[9];
  to_normalised(f0, nrm, h);
  unit_frobenius(h);
  {
    bool finite = true, nonzero = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) { finite = finite && isfinite(h[i]); nonzero = nonzero || h[i] != 0.0; }
    good = good && finite && nonzero;
  }

  // pass 0 costs the input as given, pass it > 0 the candidate of step it; one call site per kind of pass
  double fk[9], fc[9], sums[RH_NSUM];
  double lambda = RH_LAMBDA0, cost0 = 0.0, count0 = 0.0, cost = 0.0, count = 0.0;
  int steps = 0, held = 0;
  bool failed = false, need_jacobian = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) fc[i] = f0[i];
  for (int it = 0; it <= iters; ++it) {
    double hc[9];
    if (it > 0) {
      if (need_jacobian) {
        double best = fabs(h[0]);
        held = 0;
#pragma unroll
        for (int i = 1; i < 9; ++i) {
          const double mag = fabs(h[i]);
          if (mag > best) { best = mag; held = i; }
        }
        jacobian_pass(h, nrm, xa, xb, mask_in, base, N, t2n, red, sums);
        need_jacobian = false;
      }
      double tri[RH_NTRI], g[RH_NPAR], delta[RH_NPAR];
      drop_held(sums, held, tri, g);
      if (!solve_step<RH_NPAR>(tri, g, lambda, delta)) { failed = true; break; }
      // "moves no bit", literally, in integer arithmetic
      long long moved = 0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double below = delta[i < RH_NPAR ? i : RH_NPAR - 1], above = delta[i > 0 ? i - 1 : 0];
        hc[i] = h[i] + (i < held ? below : (i > held ? above : 0.0));
        moved |= __double_as_longlong(hc[i]) ^ __double_as_longlong(h[i]);
      }
      if (moved == 0) break;
      unit_frobenius(hc);
      homography_to_pixels(hc, nrm, fc);
    }
    double c2, n2;
    cost_pass(fc, xa, xb, mask_in, base, N, t2, red, c2, n2);
    if (it == 0) {
      cost0 = cost = c2;
      count0 = count = n2;
      if (!(good && count0 >= (double)RH_MIN_MATCHES)) break;
    } else if (c2 < cost * (1.0 - RH_ACCEPT_REL)) {
#pragma unroll
      for (int i = 0; i < 9; ++i) { h[i] = hc[i]; fk[i] = fc[i]; }
      cost = c2;
      count = n2;
      lambda = fmax(lambda / 10.0, RH_LAMBDA_MIN);
      ++steps;
      need_jacobian = true;
    } else {
      lambda *= 10.0;
    }
  }
  if (failed || steps == 0) {                                   // the input, as it came
    steps = 0;
    cost = cost0;
    count = count0;
#pragma unroll
    for (int i = 0; i < 9; ++i) fk[i] = f0[i];
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H_out[p * 9 + i] = fk[i];
    cost_out[p] = cost;
    count_out[p] = (int)count;
    steps_out[p] = steps;
  }
  // the mask of the returned model: the e of the pass that counted its inliers, bit for bit
  for (int i = tid; i < N; i += RH_THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    double iw, px, py, rx, ry;
    mask_out[base + i] = (m.ok && transfer_error(fk, m.x, m.y, m.u, m.v, iw, px, py, rx, ry) < t2) ? 1 : 0;
  }
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_refine_homography(const double* xa, const double* xb, const double* H_in, const unsigned char* mask_in, int P, int N,
                                      double threshold, int iters, double* H, unsigned char* mask, double* cost, int* count,
                                      int* steps, void* stream) {
  ROMA_REQUIRE(xa && xb && H_in && H && mask && cost && count && steps, ROMA_E_ARG, "roma_refine_homography: null pointer");
  const int rc = check_refine(__func__, xa, xb, P, N, RH_MIN_MATCHES, threshold, iters);
  if (rc) return rc;
  hipLaunchKernelGGL(refine_homography_kernel, dim3(P), dim3(RH_THREADS), 0, static_cast<hipStream_t>(stream), (const double2*)xa,
                     (const double2*)xb, H_in, mask_in, N, threshold * threshold, iters, H, mask, cost, count, steps);
  ROMA_CHECK_LAUNCH();
}
