// Non-linear refinement of a relative pose: Levenberg-Marquardt on the truncated Sampson cost of the calibrated matches — what
// poselib.estimate_relative_pose runs behind its RANSAC (romatch/benchmarks/megadepth_pose_estimation_benchmark_poselib.py:82-95).
// It follows essential.hip's recover_pose_kernel in the pipeline find_essential -> recover_pose -> refine_pose.  Ground rules of
// fp64, nothing allocated, no atomics, no host synchronisation, sums in a fixed order, so the output is bitwise
// reproducible and a pair's result does not depend on the rest of the batch.  tests/pose_refine_ref.py restates it in numpy.
//
// One workgroup of 256 threads per pair runs the whole schedule in one launch.  Every thread holds the pose, the damping and the
// reduced sums (they are block-uniform: every thread computes the same values from the same reduced sums), so the only
// communication is the reduction: a wave butterfly, then the four waves summed in order through LDS, two barriers per pass.
//
//   pose        (R, t), |t| = 1, E = [t]x R
//   parameters  (w, a, b): R <- exp([w]x) R (|w| limited to 1 rad), t <- (t + a b1 + b b2) / |.|; e = the coordinate axis of the smallest |t_i| (lowest
//               index on ties), b1 = (t x e) / |t x e|, b2 = t x b1.  The candidate's R is re-orthonormalised (Gram-Schmidt on its
//               rows) before it is evaluated, so the cost that accepts a step is the cost of the pose that is returned.
//   residual    r = x_B^T E x_A / sqrt((E x_A)_1^2 + (E x_A)_2^2 + (E^T x_B)_1^2 + (E^T x_B)_2^2) on x_hat = K^-1 x (as calibrate_kernel)
//   cost        sum of min(r^2, thr^2) over the usable matches (finite, allowed by mask_in); weight 1 where r^2 < thr^2, else 0 —
//               the truncated loss, the MSAC score of the estimator in front of it
//   Jacobian    analytic: dE/dw_k = [t]x [e_k]x R (the left factor of exp([w]x) R acts on R alone), dE/da = [b1]x R, dE/db = [b2]x R;
//               for r = n / sqrt d: dr = dn / sqrt d - n dd / (2 d^(3/2))
//   one pass    22 sums: the 15 upper entries of J^T J, the 5 of J^T r, the cost, the inlier count.  A pass reads the pair's pixel
//               matches again and calibrates them (6 multiply-adds against a few hundred of the residual and its Jacobian; the
//               32 N bytes stay in the L2), so no thread keeps points and there is no limit on N
//   one step    (A + lambda diag A) delta = -g by a 5 x 5 Cholesky in registers; the candidate's pass gives its cost AND its normal
//               equations, so an accepted step costs no second pass.  Kept when cost' < cost (1 - 1e-12) — strictly lower, by more
//               than the rounding of the sums, so a recomputation elsewhere agrees that no step raised the cost —, then lambda <-
//               max(lambda / 10, 1e-10); else lambda <- 10 lambda.  lambda_0 = 1e-3; `iters` steps, fixed; a step that moves no
//               bit of the pose ends the schedule (no later one would)
//   failure     fewer than 5 weighted matches under the input pose, a Cholesky pivot that is not positive, an input pose that is
//               not finite or has t = 0: the input pose is returned as it came, with its own mask, cost and count
//
// Shared with fundamental_refine.hip, in twoview_math.h: the residual, Match, block_sum, solve_step and the checks of the entry
// point.  The schedules stay apart: here one pass gives the cost and the normal equations of a candidate.  The row of the normal
// equations and the mask loop are written out here as in fundamental_refine.hip: this kernel sits at 256 VGPRs, and behind a shared
// function the compiler allocates its registers differently.
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int RP_THREADS = 256, RP_WAVES = RP_THREADS / 64;
constexpr int RP_NPAR = 5, RP_NTRI = 15, RP_NSUM = 22;        // 15 + 5 + cost + count
constexpr int RP_COST = 20, RP_COUNT = 21;
constexpr int RP_MIN_MATCHES = 5;
constexpr double RP_LAMBDA0 = 1e-3, RP_LAMBDA_MIN = 1e-10, RP_ACCEPT_REL = 1e-12;

__device__ __forceinline__ void tangent_basis(const double* t, double* b1, double* b2) {
  const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
  int j = a1 < a0 ? 1 : 0;
  j = a2 < (j ? a1 : a0) ? 2 : j;
  const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
  cross3(t, e, b1);
  const double inv = 1.0 / sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) b1[i] *= inv;
  cross3(t, b1, b2);
}

// M[0] = E = [t]x R, M[1..3] = [t]x [e_k]x R, M[4] = [b1]x R, M[5] = [b2]x R
__device__ __forceinline__ void model_matrices(const double* R, const double* t, double (&M)[6][9]) {
  double b1[3], b2[3], tmp[9];
  tangent_basis(t, b1, b2);
  skew_times(t, R, M[0]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    skew_times(e, R, tmp);
    skew_times(t, tmp, M[1 + k]);
  }
  skew_times(b1, R, M[4]);
  skew_times(b2, R, M[5]);
}

// the calibrated match i of pair p, as calibrate_kernel computes it; ok: finite and allowed by mask_in
__device__ __forceinline__ Match load_match(const double2* __restrict__ xa, const double2* __restrict__ xb, const unsigned char* mask_in,
                                            size_t q, const double* ia, const double* ib, bool kok) {
  const double2 a = xa[q], b = xb[q];
  Match m;
  m.x = ia[0] * a.x + ia[1] * a.y + ia[2];
  m.y = ia[3] * a.y + ia[4];
  m.u = ib[0] * b.x + ib[1] * b.y + ib[2];
  m.v = ib[3] * b.y + ib[4];
  m.ok = kok && isfinite(a.x) && isfinite(a.y) && isfinite(b.x) && isfinite(b.y) && isfinite(m.x) && isfinite(m.y) && isfinite(m.u) &&
         isfinite(m.v) && (!mask_in || mask_in[q] != 0);
  return m;
}

// The 22 sums of one pose over the pair's matches, reduced: on return every thread holds the same s[].
__device__ __forceinline__ void evaluate(const double* R, const double* t, const double2* __restrict__ xa, const double2* __restrict__ xb,
                                         const unsigned char* mask_in, size_t base, int N, const double* ia, const double* ib, bool kok,
                                         double t2, double (*red)[RP_NSUM], double (&s)[RP_NSUM]) {
  double M[6][9];
  model_matrices(R, t, M);
#pragma unroll
  for (int k = 0; k < RP_NSUM; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < N; i += RP_THREADS) {
    const Match m = load_match(xa, xb, mask_in, base + i, ia, ib, kok);
    double ex[3], et[2], n, d, isd, r;
    apply_model(M[0], m.x, m.y, m.u, m.v, ex, et);
    sampson_terms(ex, et, m.u, m.v, n, d);
    const double r2 = squared_residual(n, d, isd, r);
    const bool in = m.ok && r2 < t2;
    const double half = n * (0.5 * isd / d);
    double J[RP_NPAR];
#pragma unroll
    for (int k = 0; k < RP_NPAR; ++k) {
      double mx[3], mt[2];
      apply_model(M[1 + k], m.x, m.y, m.u, m.v, mx, mt);
      const double dn = m.u * mx[0] + m.v * mx[1] + mx[2];
      const double dd = 2.0 * (ex[0] * mx[0] + ex[1] * mx[1] + et[0] * mt[0] + et[1] * mt[1]);
      J[k] = in ? dn * isd - half * dd : 0.0;
    }
    const double rw = in ? r : 0.0;
    int o = 0;
#pragma unroll
    for (int a = 0; a < RP_NPAR; ++a)
#pragma unroll
      for (int b = a; b < RP_NPAR; ++b, ++o) s[o] = __builtin_fma(J[a], J[b], s[o]);
#pragma unroll
    for (int a = 0; a < RP_NPAR; ++a) s[RP_NTRI + a] = __builtin_fma(J[a], rw, s[RP_NTRI + a]);
    s[RP_COST] += m.ok ? (in ? r2 : t2) : 0.0;
    s[RP_COUNT] += in ? 1.0 : 0.0;
  }
  block_sum<RP_NSUM, RP_WAVES>(s, red);
}

// Rc = orthonormalised exp([w]x) R, tc = (t + a b1 + b b2) / |.|
__device__ __forceinline__ void apply_step(const double* R, const double* t, const double (&delta)[RP_NPAR], double* Rc, double* tc) {
  // the rotation of one step is limited to 1 rad, where so3_exp_series is exact to rounding
  double w[3] = {delta[0], delta[1], delta[2]};
  double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 > 1.0) {
    const double sc = 1.0 / sqrt(th2);
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] *= sc;
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  }
  double A, B;
  so3_exp_series(th2, A, B, So3Literals());
  // exp([w]x) R = R + A [w]x R + B [w]x [w]x R
  double KR[9], KKR[9], X[9];
  skew_times(w, R, KR);
  skew_times(w, KR, KKR);
#pragma unroll
  for (int i = 0; i < 9; ++i) X[i] = R[i] + A * KR[i] + B * KKR[i];
  orthonormalise_rows(X, Rc);
  double b1[3], b2[3];
  tangent_basis(t, b1, b2);
#pragma unroll
  for (int i = 0; i < 3; ++i) tc[i] = t[i] + delta[3] * b1[i] + delta[4] * b2[i];
  const double it = 1.0 / sqrt(tc[0] * tc[0] + tc[1] * tc[1] + tc[2] * tc[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) tc[i] *= it;
}

__global__ __launch_bounds__(RP_THREADS) void refine_pose_kernel(const double2* __restrict__ xa, const double2* __restrict__ xb,
                                                                 const double* __restrict__ Ka, const double* __restrict__ Kb,
                                                                 const double* __restrict__ R_in, const double* __restrict__ t_in,
                                                                 const unsigned char* mask_in, int N, double t2, int iters,
                                                                 double* __restrict__ R_out, double* __restrict__ t_out,
                                                                 unsigned char* __restrict__ mask_out, double* __restrict__ cost_out,
                                                                 int* __restrict__ count_out, int* __restrict__ steps_out) {
  __shared__ double red[RP_WAVES][RP_NSUM], in[30];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  // the pair's constants go through LDS, so that every thread holds them in vector registers (read straight from global memory
  // they are scalar loads, and 42 fp64 values kept in scalar registers across the schedule overflow that file)
  if (tid < 9) { in[tid] = Ka[p * 9 + tid]; in[9 + tid] = Kb[p * 9 + tid]; in[18 + tid] = R_in[p * 9 + tid]; }
  if (tid < 3) in[27 + tid] = t_in[p * 3 + tid];
  __syncthreads();
  double ia[5], ib[5];
  const bool ka_ok = invert_k(in, ia), kb_ok = invert_k(in + 9, ib), kok = ka_ok && kb_ok;
  double R[9], t[3];
  bool good = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = in[18 + i]; good = good && isfinite(R[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { t[i] = in[27 + i]; good = good && isfinite(t[i]); }
  good = good && (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) > 0.0;

  // pass 0 evaluates the input pose, pass it > 0 the candidate of step it; (Rk, tk, s) is the last accepted pose with its sums
  double Rk[9], tk[3], s[RP_NSUM];
  double lambda = RP_LAMBDA0, cost0 = 0.0, count0 = 0.0;
  int steps = 0;
  bool failed = false;
  for (int it = 0; it <= iters; ++it) {
    double Rc[9], tc[3], sc[RP_NSUM];
    if (it == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rc[i] = R[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) tc[i] = t[i];
    } else {
      double delta[RP_NPAR];
      if (!solve_step<RP_NPAR>(s, s + RP_NTRI, lambda, delta)) { failed = true; break; }
      apply_step(Rk, tk, delta, Rc, tc);
      bool moved = false;
#pragma unroll
      for (int i = 0; i < 9; ++i) moved = moved || Rc[i] != Rk[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) moved = moved || tc[i] != tk[i];
      if (!moved) break;
    }
    evaluate(Rc, tc, xa, xb, mask_in, base, N, ia, ib, kok, t2, red, sc);
    const bool first = it == 0;
    if (first) { cost0 = sc[RP_COST]; count0 = sc[RP_COUNT]; }
    if (first || sc[RP_COST] < s[RP_COST] * (1.0 - RP_ACCEPT_REL)) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rk[i] = Rc[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) tk[i] = tc[i];
#pragma unroll
      for (int k = 0; k < RP_NSUM; ++k) s[k] = sc[k];
      if (!first) {
        lambda = fmax(lambda / 10.0, RP_LAMBDA_MIN);
        ++steps;
      }
    } else {
      lambda *= 10.0;
    }
    if (first && !(good && count0 >= (double)RP_MIN_MATCHES)) break;
  }
  if (failed) {                                             // the input pose, as it came
    steps = 0;
    s[RP_COST] = cost0;
    s[RP_COUNT] = count0;
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rk[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tk[i];
  }
  if (tid < 9) R_out[p * 9 + tid] = R[tid];
  if (tid < 3) t_out[p * 3 + tid] = t[tid];
  if (tid == 0) {
    cost_out[p] = s[RP_COST];
    count_out[p] = (int)s[RP_COUNT];
    steps_out[p] = steps;
  }
  double M[6][9];
  model_matrices(R, t, M);
  for (int i = tid; i < N; i += RP_THREADS) {
    const Match m = load_match(xa, xb, mask_in, base + i, ia, ib, kok);
    double ex[3], et[2], n, d, isd, r;
    apply_model(M[0], m.x, m.y, m.u, m.v, ex, et);
    sampson_terms(ex, et, m.u, m.v, n, d);
    mask_out[base + i] = (m.ok && squared_residual(n, d, isd, r) < t2) ? 1 : 0;
  }
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_refine_pose(const double* xa, const double* xb, const double* Ka, const double* Kb, const double* R_in,
                                const double* t_in, const unsigned char* mask_in, int P, int N, double threshold, int iters, double* R,
                                double* t, unsigned char* mask, double* cost, int* count, int* steps, void* stream) {
  ROMA_REQUIRE(xa && xb && Ka && Kb && R_in && t_in && R && t && mask && cost && count && steps, ROMA_E_ARG,
               "roma_refine_pose: null pointer");
  const int rc = check_refine(__func__, xa, xb, P, N, RP_MIN_MATCHES, threshold, iters);
  if (rc) return rc;
  hipLaunchKernelGGL(refine_pose_kernel, dim3(P), dim3(RP_THREADS), 0, static_cast<hipStream_t>(stream), (const double2*)xa,
                     (const double2*)xb, Ka, Kb, R_in, t_in, mask_in, N, threshold * threshold, iters, R, t, mask, cost, count, steps);
  ROMA_CHECK_LAUNCH();
}
