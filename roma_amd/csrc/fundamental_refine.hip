// Non-linear refinement of a fundamental matrix: Levenberg-Marquardt on the truncated Sampson cost of the pixel matches — the polish
// that the OpenCV estimators behind the reference's uncalibrated calls (cv2.findFundamentalMat with USAC_ACCURATE / RANSAC,
// demo/demo_fundamental.py, romatch/utils/utils.py:54-76) run after consensus, and that geometry.hip's select_kernel, which stops at
// an algebraic 8-point refit projected to rank 2, does not.  Pipeline: find_fundamental -> refine_fundamental.  Ground rules of
// DESIGN.md §3.4, as pose_refine.hip: fp64, nothing allocated, no atomics, no host synchronisation, sums in a fixed order, so the
// output is bitwise reproducible and a pair's result does not depend on the rest of the batch.  tests/fundamental_refine_ref.py
// restates it in numpy.
//
// One workgroup of 256 threads per pair runs the whole schedule in one launch.  Every thread holds the model, the damping and the
// reduced sums (block-uniform: every thread computes the same values from the same reduced sums); the only communication is the
// reduction (a wave butterfly, then the four waves summed in order through LDS), the staging of per-pair constants through LDS,
// and the 3 x 3 Jacobi of the initial factorisation.
//
//   residual    r = x_B^T F x_A / sqrt((F x_A)_1^2 + (F x_A)_2^2 + (F^T x_B)_1^2 + (F^T x_B)_2^2) in the pixels of the input: what
//               find_fundamental scores with (in fp32 there)
//   cost        sum of min(r^2, thr^2) over the usable matches (finite, allowed by mask_in); weight 1 where r^2 < thr^2, else 0
//   coordinates Hartley: x^ = (x - c) s per image, centroid and mean distance sqrt 2 over the usable matches, computed here
//   model       F^ = U diag(1, s, 0) V^T, U, V in SO(3): exactly rank 2 by construction.  7 parameters (w_u, w_v, ds):
//               U <- U exp([w_u]x), V <- V exp([w_v]x) (each |w| limited to 1 rad), s <- s + ds.  The model in pixels is
//               T_B^T F^ T_A, scaled to unit Frobenius norm with its largest-magnitude entry positive (find_fundamental's
//               convention): the cost that accepts a step is the cost of exactly the nine numbers that are returned
//   start       the eigenvectors v_i of F^^T F^ (jacobi_lds), F^ = T_B^-T F T_A^-1, ordered by eigenvalue; u_i = F^ v_i / |F^ v_i|,
//               u_3 = u_1 x u_2, v_3 flipped where det V < 0, s = |F^ v_2| / |F^ v_1|
//   Jacobian    analytic, of T_B^T F^ T_A: dF^/dw_u = (s u3 v2^T, -u3 v1^T, u2 v1^T - s u1 v2^T), dF^/dw_v = (s u2 v3^T, -u1 v3^T,
//               u1 v2^T - s u2 v1^T), dF^/ds = u2 v2^T; for r = n / sqrt d: dr = dn / sqrt d - n dd / (2 d^(3/2))
//   passes      a COST pass (2 sums: cost, count) for the input and for every candidate, with the model in registers; a JACOBIAN
//               pass (37 sums: 28 of J^T J, 7 of J^T r, cost, count) at the start and after a kept step only, with the model and its
//               7 derivatives staged in LDS.  A pass reads the pair's matches again (32 N bytes, they stay in the L2)
//   one step    (A + lambda diag A) delta = -g by a 7 x 7 Cholesky in registers.  Kept when cost' < cost (1 - 1e-12), then lambda <-
//               max(lambda / 10, 1e-10); else lambda <- 10 lambda.  lambda_0 = 1e-3; at most `iters` steps; a step that moves no bit
//               of (U, s, V) ends the schedule
//   baseline    `cost` starts as the cost of the input F as given, before the projection to rank 2, so a kept step is below the input
//   unchanged   no kept step, fewer than 8 weighted matches under the input, a Cholesky pivot that is not positive, an input that is
//               not finite or has no second singular value (sigma_2^2 <= 1e-14 sigma_1^2: the eigenvalues of F^^T F^ carry an
//               absolute error of a few eps sigma_1^2, below that v_2 is not determined): the input is returned bit for bit, with
//               its own mask, cost and count, and steps = 0
//
// Shared with pose_refine.hip, in twoview_math.h: the residual, Match, block_sum, solve_step and the checks of the entry point; with
// homography_refine.hip: load_pixels and the normalisation; with geometry.hip's select_kernel: Norm, to_pixels, jacobi_lds.  The schedules stay apart: here a candidate gets a cost pass, and
// only a kept step a Jacobian pass.  The row of the normal equations and the mask loop are written out here as in pose_refine.hip:
// this kernel sits at 256 VGPRs, and behind a shared function the compiler allocates its registers differently.
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int RF_THREADS = 256, RF_WAVES = RF_THREADS / 64;
constexpr int RF_NPAR = 7, RF_NTRI = 28, RF_NSUM = 37;          // 28 + 7 + cost + count
constexpr int RF_COST = 35, RF_COUNT = 36;
constexpr int RF_MIN_MATCHES = 8;
constexpr double RF_LAMBDA0 = 1e-3, RF_LAMBDA_MIN = 1e-10, RF_ACCEPT_REL = 1e-12, RF_RANK_TOL = 1e-14;

// o = T_B^-T f T_A^-1: normalised coordinates from pixels
__device__ __forceinline__ void to_normalised(const double* f, const Norm& n, double* o) {
  double g[9];
  const double iA = 1.0 / n.sA, iB = 1.0 / n.sB;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = f[3 * r] * iA;
    g[3 * r + 1] = f[3 * r + 1] * iA;
    g[3 * r + 2] = f[3 * r + 2] + (n.cxA * f[3 * r] + n.cyA * f[3 * r + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o[j] = g[j] * iB;
    o[3 + j] = g[3 + j] * iB;
    o[6 + j] = g[6 + j] + (n.cxB * g[j] + n.cyB * g[3 + j]);
  }
}

// unit Frobenius norm, largest-magnitude entry positive (lowest index on ties): the convention of find_fundamental
__device__ __forceinline__ void finish_model(double* o) {
  unit_frobenius(o);
  int jm = 0;
#pragma unroll
  for (int i = 1; i < 9; ++i)
    if (fabs(o[i]) > fabs(o[jm])) jm = i;
  double sgn = 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i)
    if (i == jm && o[i] < 0.0) sgn = -1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) o[i] *= sgn;
}

// a u_i v_j^T + b u_k v_l^T, columns of U and V (row major)
__device__ __forceinline__ void outer2(const double* U, const double* V, double a, int i, int j, double b, int k, int l, double* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * r + c] = a * (U[3 * r + i] * V[3 * c + j]) + b * (U[3 * r + k] * V[3 * c + l]);
}

// the model in pixels as it is returned: finish(T_B^T U diag(1, s, 0) V^T T_A)
__device__ __forceinline__ void pixel_model(const double* U, double s, const double* V, const Norm& n, double* f) {
  double h[9];
  outer2(U, V, 1.0, 0, 0, s, 1, 1, h);
  to_pixels(h, n, f);
  finish_model(f);
}

// M[0] = T_B^T F^ T_A and M[1..7] its derivatives by (w_u, w_v, ds) at zero, into LDS (thread 0 writes; the caller's pass follows
// a barrier)
__device__ __forceinline__ void stage_matrices(const double* U, double s, const double* V, const Norm& n, double* M) {
  double h[9], o[9];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    switch (k) {
      case 0: outer2(U, V, 1.0, 0, 0, s, 1, 1, h); break;
      case 1: outer2(U, V, s, 2, 1, 0.0, 0, 0, h); break;
      case 2: outer2(U, V, -1.0, 2, 0, 0.0, 0, 0, h); break;
      case 3: outer2(U, V, 1.0, 1, 0, -s, 0, 1, h); break;
      case 4: outer2(U, V, s, 1, 2, 0.0, 0, 0, h); break;
      case 5: outer2(U, V, -1.0, 0, 2, 0.0, 0, 0, h); break;
      case 6: outer2(U, V, 1.0, 0, 1, -s, 1, 0, h); break;
      default: outer2(U, V, 1.0, 1, 1, 0.0, 0, 0, h); break;
    }
    to_pixels(h, n, o);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) M[9 * k + i] = o[i];
    }
  }
  __syncthreads();
}

// cost and inlier count of the pixel model f over the pair's matches, reduced
__device__ __forceinline__ void cost_pass(const double* f, const double2* __restrict__ xa, const double2* __restrict__ xb,
                                          const unsigned char* mask_in, size_t base, int N, double t2, double (*red)[RF_NSUM],
                                          double& cost, double& count) {
  double c[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < N; i += RF_THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    double ex[3], et[2], n, d, isd, r;
    apply_model(f, m.x, m.y, m.u, m.v, ex, et);
    sampson_terms(ex, et, m.u, m.v, n, d);
    const double r2 = squared_residual(n, d, isd, r);
    const bool in = m.ok && r2 < t2;
    c[0] += m.ok ? (in ? r2 : t2) : 0.0;
    c[1] += in ? 1.0 : 0.0;
  }
  block_sum<2, RF_WAVES>(c, red);
  cost = c[0];
  count = c[1];
}

// the 37 sums of the model staged in M (LDS) over the pair's matches, reduced
__device__ __forceinline__ void jacobian_pass(const double* M, const double2* __restrict__ xa, const double2* __restrict__ xb,
                                              const unsigned char* mask_in, size_t base, int N, double t2, double (*red)[RF_NSUM],
                                              double (&s)[RF_NSUM]) {
#pragma unroll
  for (int k = 0; k < RF_NSUM; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < N; i += RF_THREADS) {
    // M is read from LDS for every match (broadcast reads): hoisted out of the loop its 72 values would take 144 registers
    asm volatile("" ::: "memory");
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    double ex[3], et[2], n, d, isd, r;
    apply_model(M, m.x, m.y, m.u, m.v, ex, et);
    sampson_terms(ex, et, m.u, m.v, n, d);
    const double r2 = squared_residual(n, d, isd, r);
    const bool in = m.ok && r2 < t2;
    const double half = n * (0.5 * isd / d);
    double J[RF_NPAR];
#pragma unroll
    for (int k = 0; k < RF_NPAR; ++k) {
      double mx[3], mt[2];
      apply_model(M + 9 * (1 + k), m.x, m.y, m.u, m.v, mx, mt);
      const double dn = m.u * mx[0] + m.v * mx[1] + mx[2];
      const double dd = 2.0 * (ex[0] * mx[0] + ex[1] * mx[1] + et[0] * mt[0] + et[1] * mt[1]);
      J[k] = in ? dn * isd - half * dd : 0.0;
    }
    const double rw = in ? r : 0.0;
    int o = 0;
#pragma unroll
    for (int a = 0; a < RF_NPAR; ++a)
#pragma unroll
      for (int b = a; b < RF_NPAR; ++b, ++o) s[o] = __builtin_fma(J[a], J[b], s[o]);
#pragma unroll
    for (int a = 0; a < RF_NPAR; ++a) s[RF_NTRI + a] = __builtin_fma(J[a], rw, s[RF_NTRI + a]);
    s[RF_COST] += m.ok ? (in ? r2 : t2) : 0.0;
    s[RF_COUNT] += in ? 1.0 : 0.0;
  }
  block_sum<RF_NSUM, RF_WAVES>(s, red);
}

// Xc = X exp([w]x), |w| limited to 1 rad: every row a of X becomes a + A (a x w) + B ((a x w) x w)
__device__ __forceinline__ void rotate_right(const double* X, const double* w_in, const double* series, double* Xc) {
  double w[3] = {w_in[0], w_in[1], w_in[2]};
  double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 > 1.0) {
    const double sc = 1.0 / sqrt(th2);
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] *= sc;
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  }
  double A, B;
  so3_exp_series(th2, A, B, So3Table{series});
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double k1[3], k2[3];
    cross3(X + 3 * r, w, k1);
    cross3(k1, w, k2);
#pragma unroll
    for (int i = 0; i < 3; ++i) Xc[3 * r + i] = X[3 * r + i] + A * k1[i] + B * k2[i];
  }
}

__global__ __launch_bounds__(RF_THREADS) void refine_fundamental_kernel(const double2* __restrict__ xa, const double2* __restrict__ xb,
                                                                        const double* __restrict__ F_in, const unsigned char* mask_in,
                                                                        int N, double t2, int iters, double* __restrict__ F_out,
                                                                        unsigned char* __restrict__ mask_out,
                                                                        double* __restrict__ cost_out, int* __restrict__ count_out,
                                                                        int* __restrict__ steps_out) {
  __shared__ double red[RF_WAVES][RF_NSUM], fin[9], JA[27], JV[27], M[72], series[2 * SO3_EXP_TERMS];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  // the pair's constants go through LDS, so that every thread holds them in vector registers
  // (so do the 20 coefficients of the exponential's series: as immediates they would hold 38 scalar registers across the schedule)
  if (tid < 9) fin[tid] = F_in[p * 9 + tid];
  if (tid == 0) so3_fill_table(series);
  __syncthreads();
  double f0[9];
  bool good = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { f0[i] = fin[i]; good = good && isfinite(f0[i]); }

  const Norm nrm = normalisation<RF_THREADS>(xa, xb, mask_in, base, N, red);

  // the start: F^ = U diag(sigma_1, sigma_2, ~0) V^T from the eigenvectors of F^^T F^
  double U[9], V[9], s = 0.0;
  {
    double h[9];
    to_normalised(f0, nrm, h);
    if (tid == 0) {                                             // static indices: h stays in registers
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          JA[r * 9 + c] = h[r] * h[c] + h[3 + r] * h[3 + c] + h[6 + r] * h[6 + c];
          JV[r * 9 + c] = r == c ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    jacobi_lds(JA, JV, 3);
    const double e0 = JA[0], e1 = JA[10], e2 = JA[20];
    int i1 = e1 > e0 ? 1 : 0;
    i1 = e2 > (i1 ? e1 : e0) ? 2 : i1;
    int i3 = e1 < e0 ? 1 : 0;
    i3 = e2 < (i3 ? e1 : e0) ? 2 : i3;
    if (i1 == i3) { i1 = 0; i3 = 2; }                          // all equal (or NaN): any order, the pair is returned unchanged below
    const int i2 = 3 - i1 - i3;
#pragma unroll
    for (int r = 0; r < 3; ++r) { V[3 * r] = JV[r * 9 + i1]; V[3 * r + 1] = JV[r * 9 + i2]; V[3 * r + 2] = JV[r * 9 + i3]; }
    if (det3(V) < 0.0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) V[3 * r + 2] = -V[3 * r + 2];
    }
    double u1[3], u2[3], u3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u1[r] = h[3 * r] * V[0] + h[3 * r + 1] * V[3] + h[3 * r + 2] * V[6];
      u2[r] = h[3 * r] * V[1] + h[3 * r + 1] * V[4] + h[3 * r + 2] * V[7];
    }
    const double s1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    const double s2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    good = good && isfinite(s1) && isfinite(s2) && s1 > 0.0 && s2 * s2 > RF_RANK_TOL * (s1 * s1);
    const double i1s = 1.0 / s1, i2s = 1.0 / s2;
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] *= i1s; u2[r] *= i2s; }
    cross3(u1, u2, u3);
#pragma unroll
    for (int r = 0; r < 3; ++r) { U[3 * r] = u1[r]; U[3 * r + 1] = u2[r]; U[3 * r + 2] = u3[r]; }
    s = s2 * i1s;
  }

  // pass 0 costs the input as given, pass it > 0 the candidate of step it; one call site per kind of pass keeps the registers in bounds
  double fk[9], fc[9], sums[RF_NSUM];
  double lambda = RF_LAMBDA0, cost0 = 0.0, count0 = 0.0, cost = 0.0, count = 0.0;
  int steps = 0;
  bool failed = false, need_jacobian = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) fc[i] = f0[i];
  for (int it = 0; it <= iters; ++it) {
    double Uc[9], Vc[9], sc = s;
    if (it > 0) {
      if (need_jacobian) {
        stage_matrices(U, s, V, nrm, M);
        jacobian_pass(M, xa, xb, mask_in, base, N, t2, red, sums);
        need_jacobian = false;
      }
      double delta[RF_NPAR];
      if (!solve_step<RF_NPAR>(sums, sums + RF_NTRI, lambda, delta)) { failed = true; break; }
      rotate_right(U, delta, series, Uc);
      rotate_right(V, delta + 3, series, Vc);
      sc = s + delta[6];
      // "moves no bit", literally: integer arithmetic, where 19 floating-point comparisons would hold 19 lane masks in scalar registers
      long long moved = __double_as_longlong(sc) ^ __double_as_longlong(s);
#pragma unroll
      for (int i = 0; i < 9; ++i)
        moved |= (__double_as_longlong(Uc[i]) ^ __double_as_longlong(U[i])) | (__double_as_longlong(Vc[i]) ^ __double_as_longlong(V[i]));
      if (moved == 0) break;
      pixel_model(Uc, sc, Vc, nrm, fc);
    }
    double c2, n2;
    cost_pass(fc, xa, xb, mask_in, base, N, t2, red, c2, n2);
    if (it == 0) {
      cost0 = cost = c2;
      count0 = count = n2;
      if (!(good && count0 >= (double)RF_MIN_MATCHES)) break;
    } else if (c2 < cost * (1.0 - RF_ACCEPT_REL)) {
#pragma unroll
      for (int i = 0; i < 9; ++i) { U[i] = Uc[i]; V[i] = Vc[i]; fk[i] = fc[i]; }
      s = sc;
      cost = c2;
      count = n2;
      lambda = fmax(lambda / 10.0, RF_LAMBDA_MIN);
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
    for (int i = 0; i < 9; ++i) F_out[p * 9 + i] = fk[i];
    cost_out[p] = cost;
    count_out[p] = (int)count;
    steps_out[p] = steps;
  }
  // the mask of the returned model: the r^2 of the pass that counted its inliers, bit for bit
  for (int i = tid; i < N; i += RF_THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    double ex[3], et[2], n, d, isd, r;
    apply_model(fk, m.x, m.y, m.u, m.v, ex, et);
    sampson_terms(ex, et, m.u, m.v, n, d);
    mask_out[base + i] = (m.ok && squared_residual(n, d, isd, r) < t2) ? 1 : 0;
  }
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_refine_fundamental(const double* xa, const double* xb, const double* F_in, const unsigned char* mask_in, int P, int N,
                                       double threshold, int iters, double* F, unsigned char* mask, double* cost, int* count,
                                       int* steps, void* stream) {
  ROMA_REQUIRE(xa && xb && F_in && F && mask && cost && count && steps, ROMA_E_ARG, "roma_refine_fundamental: null pointer");
  const int rc = check_refine(__func__, xa, xb, P, N, RF_MIN_MATCHES, threshold, iters);
  if (rc) return rc;
  hipLaunchKernelGGL(refine_fundamental_kernel, dim3(P), dim3(RF_THREADS), 0, static_cast<hipStream_t>(stream), (const double2*)xa,
                     (const double2*)xb, F_in, mask_in, N, threshold * threshold, iters, F, mask, cost, count, steps);
  ROMA_CHECK_LAUNCH();
}
