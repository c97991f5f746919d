// Calibrated two-view geometry: RANSAC for essential matrices (5-point minimal solver) and relative pose recovery.  Replaces
// estimate_pose of the reference (romatch/utils/utils.py:31-52: cv2.findEssentialMat on calibrated points, then cv2.recoverPose),
// which both pose benchmarks call.  Same ground rules as geometry.hip: fp64 minimal solver, fp32 scoring of every slot (MSAC, or
// MAGSAC++ through the *_ex entry points), fixed number of samples, no atomics, no host synchronisation, bitwise reproducible.
// DESIGN.md §3.4.
//
// Pipeline, one call of roma_essential_hypotheses + one of roma_essential_select (P pairs of N matches, H = iters samples each):
//   calibrate_kernel         one block/pair   x_hat = K^-1 x in fp64 (both images) + the fp32 copy the scoring reads (NaN where a match
//                                             is not finite, or everywhere when K is not invertible); normalisation record (0, 0, 1)
//   five_point_kernel        32 lanes/sample  draws the sample (stage 4) and solves the 5-point problem in fp64 -> R = 10 slots
//   score_kernel<KIND_F>     an E in calibrated coordinates is an F: the scoring of geometry.hip on iters * 10 slots, ka = kb = 1
//   reduce_kernel            (ransac_common.h)
//   essential_select_kernel  one block/pair   lowest cost, lo_iters rounds of least squares on the inliers projected onto the
//                                             essential manifold (weighted by W for MAGSAC++), kept only if the cost drops; E with
//                                             singular values (s, s, 0)
// and, on its own, recover_pose_kernel (one block/pair): the four (R, t) of E, cheirality vote over the masked matches.
//
// The 5-point solver (Nistér 2004, hidden-variable finish: the degree-10 polynomial in z).  One sample is solved by a group of 32
// lanes, because its 10 x 20 fp64 system does not fit one lane's registers:
//   1. every lane: 5 x 9 epipolar system (rows [u x, u y, u, v x, v y, v, x, y, 1]), elimination with partial pivoting (pivot test
//      1e-10 x largest entry, as F), null space X, Y, Z, W by back-substitution, orthonormalised by two rounds of Gram-Schmidt;
//      E = xX + yY + zZ + W.  The basis goes to LDS.
//   2. lane j < 20 owns column j of the 10 x 20 constraint matrix (det E = 0; 2 E E^T E - tr(E E^T) E = 0), monomial order
//        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
//      The coefficient of the monomial v_a v_b v_c is the trilinear form of the constraints summed over the orders of (a, b, c)
//      (polarisation) — the lane reads its three basis matrices from LDS, nothing is indexed dynamically in registers.
//   3. rows scaled by their largest entry (cross-lane max); Gauss-Jordan with partial pivoting: the owning lane picks the pivot
//      row, the pivot column is broadcast by cross-lane moves, every lane updates its own column.  A pivot <= 1e-10 (the rows have
//      largest entry 1) rejects the sample.
//   4. rows x^2z - z x^2, y^2z - z y^2, xyz - z xy of the reduced system are linear in (x, y, 1) with polynomial coefficients in z
//      of degree (3, 3, 4); their 3 x 3 determinant is the degree-10 polynomial, scaled to largest coefficient 1.
//   5. real roots: lanes 0-15 of the group take z in [-1, 1], lanes 16-31 take w = 1 / z in (-1, 1) on the reversed polynomial, so
//      every interval is bounded.  Roots are isolated by the derivative ladder: the real roots of the (10 - d)-th derivative, d = 1
//      .. 10, lie one in each interval between the roots of the derivative before it where the sign changes; one lane per
//      interval, 32 bisection steps (50 on the polynomial itself, then 2 Newton steps kept inside the bracket).
//   6. per root: (x, y, 1) is the cross product of the two rows of the 3 x 3 matrix at z that gives the longest one; the solution
//      is polished by 3 Gauss-Newton steps on the ten constraints over the unit 4-vector of basis coefficients (the degree-10
//      coefficients lose up to 1e-3 on hard samples; the polished models satisfy the constraints to ~1e-13).
//   7. slots are ordered by increasing z (w < 0 first, from 0 down; then z in [-1, 1]; then w > 0 downwards), unit Frobenius norm;
//      unused slots are zero and invalid.
// Pose recovery: eigen-decomposition of E^T E (Jacobi) -> v1, v2, v3 = v1 x v2; u1 = E v1 / |E v1|, u2 = E v2 made orthogonal to u1,
// u3 = u1 x u2; R = U W V^T or U W^T V^T, t = +-u3, candidates in the order (W,+) (W,-) (W^T,+) (W^T,-).  Depths of a match under
// a candidate from the normal equations of lambda_B x_B = lambda_A R x_A + t; a match votes when both are finite and positive.
//
// Shared code: the scoring, the workspace layout and the checks are ransac_common.h's (with geometry.hip); elimination, jacobi_lds
// and invert_k are twoview_math.h's.  Steps 1 and 2 of essential_select_kernel repeat geometry.hip's select_kernel, statement for
// statement.
#include "ransac_common.h"

namespace roma {
namespace {

constexpr int E_S = 5, E_R = 10;
constexpr int GROUP = 32, GROUPS = 8;                 // lanes per sample, samples per 256-thread block
constexpr int BISECT_INNER = 32, BISECT_FINAL = 50, NEWTON_FINAL = 2, POLISH_ITERS = 3;

// xh: (P,N,4) fp64 calibrated (xa, ya, xb, yb); pts: the fp32 copy; norm: (0, 0, 1, 0) twice
__global__ __launch_bounds__(256) void calibrate_kernel(const double* __restrict__ xa, const double* __restrict__ xb,
                                                        const double* __restrict__ Ka, const double* __restrict__ Kb, int N,
                                                        double* __restrict__ norm, float* __restrict__ pts, double* __restrict__ xh) {
  const int p = blockIdx.x, tid = threadIdx.x;
  double ia[5], ib[5];
  const bool ka_ok = invert_k(Ka + p * 9, ia), kb_ok = invert_k(Kb + p * 9, ib), kok = ka_ok && kb_ok;
  if (tid < 8) norm[p * 8 + tid] = (tid & 3) == 2 ? 1.0 : 0.0;
  const double nan = __builtin_nan("");
  for (int i = tid; i < N; i += 256) {
    const size_t q = ((size_t)p * N + i) * 2;
    const double ax = xa[q], ay = xa[q + 1], bx = xb[q], by = xb[q + 1];
    const bool ok = kok && isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by);
    double o[4];
    o[0] = ia[0] * ax + ia[1] * ay + ia[2];
    o[1] = ia[3] * ay + ia[4];
    o[2] = ib[0] * bx + ib[1] * by + ib[2];
    o[3] = ib[3] * by + ib[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool fin = ok && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(o[3]);
      xh[q * 2 + k] = fin ? o[k] : nan;
      pts[q * 2 + k] = fin ? (float)o[k] : __builtin_nanf("");
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- 5-point solver
// monomials as multisets over (x, y, z, 1) = (0, 1, 2, 3): a | b << 2 | c << 4 | (number of equal orders: 1, 2 or 6) << 6
#define ROMA_MONO(a, b, c, f) ((a) | ((b) << 2) | ((c) << 4) | ((f) << 6))
__device__ const int MONOMIAL[32] = {
    ROMA_MONO(0, 0, 0, 6), ROMA_MONO(1, 1, 1, 6), ROMA_MONO(0, 0, 1, 2), ROMA_MONO(0, 1, 1, 2), ROMA_MONO(0, 0, 2, 2),
    ROMA_MONO(0, 0, 3, 2), ROMA_MONO(1, 1, 2, 2), ROMA_MONO(1, 1, 3, 2), ROMA_MONO(0, 1, 2, 1), ROMA_MONO(0, 1, 3, 1),
    ROMA_MONO(0, 2, 2, 2), ROMA_MONO(0, 2, 3, 1), ROMA_MONO(0, 3, 3, 2), ROMA_MONO(1, 2, 2, 2), ROMA_MONO(1, 2, 3, 1),
    ROMA_MONO(1, 3, 3, 2), ROMA_MONO(2, 2, 2, 6), ROMA_MONO(2, 2, 3, 2), ROMA_MONO(2, 3, 3, 2), ROMA_MONO(3, 3, 3, 6),
    ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6),
    ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6),
    ROMA_MONO(3, 3, 3, 6), ROMA_MONO(3, 3, 3, 6)};
#undef ROMA_MONO

// acc += T(P, Q, R), the trilinear form with T(E, E, E) = (det E, 2 E E^T E - tr(E E^T) E)
__device__ __forceinline__ void trilinear_acc(const double* P, const double* Q, const double* R, double* acc) {
  acc[0] += P[0] * (Q[4] * R[8] - Q[5] * R[7]) - P[1] * (Q[3] * R[8] - Q[5] * R[6]) + P[2] * (Q[3] * R[7] - Q[4] * R[6]);
  double pq[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) pq[3 * r + c] = P[3 * r] * Q[3 * c] + P[3 * r + 1] * Q[3 * c + 1] + P[3 * r + 2] * Q[3 * c + 2];
  const double tr = pq[0] + pq[4] + pq[8];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      acc[1 + 3 * r + c] += 2.0 * (pq[3 * r] * R[c] + pq[3 * r + 1] * R[3 + c] + pq[3 * r + 2] * R[6 + c]) - tr * R[3 * r + c];
}

// out[i + j] += s * a[i] * b[j]
template <int NA, int NB> __device__ __forceinline__ void poly_mul_acc(const double* a, const double* b, double s, double* out) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] = __builtin_fma(s * a[i], b[j], out[i + j]);
}

// rows e (monomial m z) and f (monomial m) of the reduced system B (6 x 10 in LDS, rows x^2z x^2 y^2z y^2 xyz xy) -> e - z f as
// polynomials in z (ascending): the factors of x (4 coefficients), y (4) and 1 (5)
__device__ __forceinline__ void row_polys(const double* B, int e, int f, double* px, double* py, double* p1) {
  const double* be = B + e * 10;
  const double* bf = B + f * 10;
  px[0] = be[2]; px[1] = be[1] - bf[2]; px[2] = be[0] - bf[1]; px[3] = -bf[0];
  py[0] = be[5]; py[1] = be[4] - bf[5]; py[2] = be[3] - bf[4]; py[3] = -bf[3];
  p1[0] = be[9]; p1[1] = be[8] - bf[9]; p1[2] = be[7] - bf[8]; p1[3] = be[6] - bf[7]; p1[4] = -bf[6];
}

// value of the polynomial c (N coefficients, ascending) at z = v (side 0), or z^-(N-1) times its value at z = 1 / v (side 1)
template <int N> __device__ __forceinline__ double eval_side(const double* c, double v, bool rev) {
  double s = 0.0;
#pragma unroll
  for (int i = N - 1; i >= 0; --i) s = __builtin_fma(s, v, rev ? c[N - 1 - i] : c[i]);
  return s;
}

// FALLING.v[i][k] = i (i - 1) .. (i - k + 1): the factor of t^(i-k) in the k-th derivative of t^i
struct FallingTable {
  double v[11][11];
  constexpr FallingTable() : v{} {
    for (int i = 0; i < 11; ++i) {
      v[i][0] = 1.0;
      for (int k = 1; k < 11; ++k) v[i][k] = v[i][k - 1] * (double)(i - k + 1);
    }
  }
};
constexpr FallingTable FALLING{};

// One level of the derivative ladder: the real roots in [-1, 1] of the (10 - D)-th derivative of a, one lane per interval between
// the nodes (-1, the roots of the level before, +1) of this side in LDS; the roots found become the next nodes.  Block-uniform.
template <int D>
__device__ __forceinline__ void ladder_level(const double (&a)[11], double* nodes, int j, int bit0, int& nint, double& root, bool& has) {
  double b[D + 1];
#pragma unroll
  for (int i = 0; i <= D; ++i) b[i] = a[i + 10 - D] * FALLING.v[i + 10 - D][10 - D];
  const bool active = j < nint;
  double lo = active ? nodes[j] : 0.0, hi = active ? nodes[j + 1] : 0.0;
  auto f = [&](double x) {
    double s = b[D];
#pragma unroll
    for (int i = D - 1; i >= 0; --i) s = __builtin_fma(s, x, b[i]);
    return s;
  };
  const bool neg = f(lo) < 0.0;
  has = active && (neg != (f(hi) < 0.0));
  constexpr int steps = D == 10 ? BISECT_FINAL : BISECT_INNER;
  for (int it = 0; it < steps; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool same = (f(mid) < 0.0) == neg;
    lo = same ? mid : lo;
    hi = same ? hi : mid;
  }
  root = 0.5 * (lo + hi);
  if constexpr (D == 10) {
#pragma unroll
    for (int it = 0; it < NEWTON_FINAL; ++it) {
      double s = b[D], d = 0.0;
#pragma unroll
      for (int i = D - 1; i >= 0; --i) { d = __builtin_fma(d, root, s); s = __builtin_fma(s, root, b[i]); }
      const double nr = root - s / d;
      root = (nr >= lo && nr <= hi) ? nr : root;
    }
  }
  __syncthreads();                                               // every lane has read its nodes
  const uint32_t m = (uint32_t)(__ballot(has) >> bit0) & 0xFFFFu;
  const int cnt = __popc(m);
  if (has) nodes[1 + __popc(m & ((1u << j) - 1u))] = root;
  if (j == 0) nodes[cnt + 1] = 1.0;
  __syncthreads();
  nint = cnt + 1;
}

// samples: (P, iters, 5) int32; models: (P, iters, 10, 9) fp64 (unit Frobenius norm); valid: (P, iters, 10)
__global__ __launch_bounds__(256) void five_point_kernel(const double* __restrict__ xh, const float* __restrict__ pts, int P, int N,
                                                         int iters, uint32_t stream, int p0, int* __restrict__ samples,
                                                         double* __restrict__ models, int* __restrict__ valid) {
  __shared__ double s_basis[GROUPS][36];
  __shared__ double s_rows[GROUPS][60];
  __shared__ double s_nodes[GROUPS][2][12];
  const int tid = threadIdx.x, g = tid >> 5, ln = tid & 31;
  const long t = (long)blockIdx.x * GROUPS + g;
  const bool live = t < (long)P * iters;                         // a dead group runs along (the barriers are block-wide), writes nothing
  const long tc = live ? t : 0;
  const int p = (int)(tc / iters), h = (int)(tc % iters);
  const size_t base = (size_t)p * N;

  // ---- the draw, on every lane
  int idx[E_S];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < E_S; ++k) {
    const uint32_t ctr = (((uint32_t)(p0 + p) * (uint32_t)iters + (uint32_t)h) * 8u + (uint32_t)k);
    int got = -1;
    for (uint32_t att = 0; att < 16; ++att) {
      const uint32_t hs = fmix32(stream + ctr * 0x9E3779B1u + att * 0x7FEB352Du);
      const int i = (int)(((uint64_t)hs * (uint64_t)(uint32_t)N) >> 32);
      const float v = pts[(base + i) * 4];
      bool good = v == v;
#pragma unroll
      for (int j = 0; j < k; ++j) good = good && idx[j] != i;
      if (good) { got = i; break; }
    }
    idx[k] = got;
    ok = ok && got >= 0;
  }
#pragma unroll
  for (int k = 0; k < E_S; ++k)
    if (live && ln == k) samples[(size_t)t * E_S + k] = ok ? idx[k] : -1;

  // ---- 1. null space of the 5 x 9 epipolar system, on every lane
  bool good = ok;
  {
    double A[5][9];
#pragma unroll
    for (int k = 0; k < E_S; ++k) {
      const double* q = xh + (base + (ok ? idx[k] : 0)) * 4;
      const double x = q[0], y = q[1], u = q[2], v = q[3];
      A[k][0] = u * x; A[k][1] = u * y; A[k][2] = u;
      A[k][3] = v * x; A[k][4] = v * y; A[k][5] = v;
      A[k][6] = x; A[k][7] = y; A[k][8] = 1.0;
    }
    good = eliminate<5>(A) && good;
    double nb[4][9];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int i = 5; i < 9; ++i) nb[f][i] = i == 5 + f ? 1.0 : 0.0;
      back_substitute<5>(A, nb[f]);
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int o = 0; o < f; ++o) {
          double d = 0.0;
#pragma unroll
          for (int i = 0; i < 9; ++i) d = __builtin_fma(nb[f][i], nb[o][i], d);
#pragma unroll
          for (int i = 0; i < 9; ++i) nb[f][i] = __builtin_fma(-d, nb[o][i], nb[f][i]);
        }
      unit_frobenius(nb[f]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (ln == f) {
#pragma unroll
        for (int i = 0; i < 9; ++i) s_basis[g][f * 9 + i] = nb[f][i];
      }
  }
  __syncthreads();
  const double* basis = s_basis[g];

  // ---- 2. this lane's column of the 10 x 20 constraint matrix
  double col[10];
  {
    const int mono = MONOMIAL[ln];
    const int ma = mono & 3, mb = (mono >> 2) & 3, mc = (mono >> 4) & 3, mf = mono >> 6;
    double Ea[9], Eb[9], Ec[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { Ea[i] = basis[ma * 9 + i]; Eb[i] = basis[mb * 9 + i]; Ec[i] = basis[mc * 9 + i]; }
#pragma unroll
    for (int r = 0; r < 10; ++r) col[r] = 0.0;
    trilinear_acc(Ea, Eb, Ec, col); trilinear_acc(Ea, Ec, Eb, col);
    trilinear_acc(Eb, Ea, Ec, col); trilinear_acc(Eb, Ec, Ea, col);
    trilinear_acc(Ec, Ea, Eb, col); trilinear_acc(Ec, Eb, Ea, col);
    const double w = ln >= 20 ? 0.0 : (mf == 1 ? 1.0 : (mf == 2 ? 0.5 : 1.0 / 6.0));
#pragma unroll
    for (int r = 0; r < 10; ++r) col[r] *= w;
  }

  // ---- 3. row scaling, Gauss-Jordan with partial pivoting across the group
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    double m = fabs(col[r]);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, GROUP));
    good = good && m > 0.0 && isfinite(m);
    col[r] = m > 0.0 ? col[r] / m : 0.0;
  }
#pragma unroll
  for (int c = 0; c < 10; ++c) {
    int pr = c;
    double best = fabs(col[c]);
#pragma unroll
    for (int r = c + 1; r < 10; ++r) {
      const bool gt = fabs(col[r]) > best;
      best = gt ? fabs(col[r]) : best;
      pr = gt ? r : pr;
    }
    pr = __shfl(pr, c, GROUP);
#pragma unroll
    for (int r = c + 1; r < 10; ++r) {
      const bool sw = r == pr;
      const double tmp = col[c];
      col[c] = sw ? col[r] : tmp;
      col[r] = sw ? tmp : col[r];
    }
    double pc[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) pc[r] = __shfl(col[r], c, GROUP);
    const double piv = pc[c];
    good = good && fabs(piv) > PIVOT_TOL;
    const double v = col[c] * (piv != 0.0 ? 1.0 / piv : 0.0);
#pragma unroll
    for (int r = 0; r < 10; ++r)
      if (r != c) col[r] = __builtin_fma(-pc[r], v, col[r]);
    col[c] = v;
  }
  if (ln >= 10 && ln < 20) {
#pragma unroll
    for (int r = 4; r < 10; ++r) s_rows[g][(r - 4) * 10 + (ln - 10)] = col[r];
  }
  if (ln < 2) s_nodes[g][ln][0] = -1.0;
  if (ln >= 2 && ln < 4) s_nodes[g][ln - 2][1] = 1.0;
  __syncthreads();

  // ---- 4. the degree-10 polynomial, on every lane
  const bool rev = ln >= 16;                                      // side 1: w = 1 / z on the reversed polynomial
  double a[11];
  {
    double kx[4], ky[4], k1[5], lx[4], ly[4], l1[5], mx[4], my[4], m1[5];
    row_polys(s_rows[g], 0, 1, kx, ky, k1);
    row_polys(s_rows[g], 2, 3, lx, ly, l1);
    row_polys(s_rows[g], 4, 5, mx, my, m1);
    double q1[8], q2[8], q3[7], c[11];
#pragma unroll
    for (int i = 0; i < 8; ++i) { q1[i] = 0.0; q2[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < 7; ++i) q3[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) c[i] = 0.0;
    poly_mul_acc<4, 5>(ly, m1, 1.0, q1); poly_mul_acc<5, 4>(l1, my, -1.0, q1);
    poly_mul_acc<4, 5>(lx, m1, 1.0, q2); poly_mul_acc<5, 4>(l1, mx, -1.0, q2);
    poly_mul_acc<4, 4>(lx, my, 1.0, q3); poly_mul_acc<4, 4>(ly, mx, -1.0, q3);
    poly_mul_acc<4, 8>(kx, q1, 1.0, c); poly_mul_acc<4, 8>(ky, q2, -1.0, c); poly_mul_acc<5, 7>(k1, q3, 1.0, c);
    double cm = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) cm = fmax(cm, fabs(c[i]));
    good = good && cm > 0.0 && isfinite(cm);
    const double inv = cm > 0.0 ? 1.0 / cm : 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) a[i] = (rev ? c[10 - i] : c[i]) * inv;
  }

  // ---- 5. real roots by the derivative ladder, one lane per interval and side
  const int j = ln & 15, bit0 = (tid & 32) + (rev ? 16 : 0);
  double* nodes = s_nodes[g][rev ? 1 : 0];
  int nint = 1;
  double root = 0.0;
  bool has = false;
  ladder_level<1>(a, nodes, j, bit0, nint, root, has);
  ladder_level<2>(a, nodes, j, bit0, nint, root, has);
  ladder_level<3>(a, nodes, j, bit0, nint, root, has);
  ladder_level<4>(a, nodes, j, bit0, nint, root, has);
  ladder_level<5>(a, nodes, j, bit0, nint, root, has);
  ladder_level<6>(a, nodes, j, bit0, nint, root, has);
  ladder_level<7>(a, nodes, j, bit0, nint, root, has);
  ladder_level<8>(a, nodes, j, bit0, nint, root, has);
  ladder_level<9>(a, nodes, j, bit0, nint, root, has);
  ladder_level<10>(a, nodes, j, bit0, nint, root, has);
  if (rev) has = has && fabs(root) < 1.0;                         // |z| = 1 belongs to side 0

  // ---- 6. (x, y, 1) at the root, Gauss-Newton polish over the unit coefficient vector
  double e[9];
  {
    double q[4];
    {
      double kx[4], ky[4], k1[5], lx[4], ly[4], l1[5], mx[4], my[4], m1[5];
      row_polys(s_rows[g], 0, 1, kx, ky, k1);
      row_polys(s_rows[g], 2, 3, lx, ly, l1);
      row_polys(s_rows[g], 4, 5, mx, my, m1);
      const double sc = rev ? root : 1.0;                         // side 1: rows scaled by z^-4
      const double r0[3] = {eval_side<4>(kx, root, rev) * sc, eval_side<4>(ky, root, rev) * sc, eval_side<5>(k1, root, rev)};
      const double r1[3] = {eval_side<4>(lx, root, rev) * sc, eval_side<4>(ly, root, rev) * sc, eval_side<5>(l1, root, rev)};
      const double r2[3] = {eval_side<4>(mx, root, rev) * sc, eval_side<4>(my, root, rev) * sc, eval_side<5>(m1, root, rev)};
      double v[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
      const double w1[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
      const double w2[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
      double nv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      const double n1 = w1[0] * w1[0] + w1[1] * w1[1] + w1[2] * w1[2], n2 = w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2];
      const bool t1 = n1 > nv;
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] = t1 ? w1[i] : v[i];
      nv = t1 ? n1 : nv;
      const bool t2 = n2 > nv;
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] = t2 ? w2[i] : v[i];
      // E ~ x X + y Y + z Z + W with (x, y, 1) ~ v; side 1: times w = 1 / z
      q[0] = rev ? root * v[0] : v[0];
      q[1] = rev ? root * v[1] : v[1];
      q[2] = rev ? v[2] : root * v[2];
      q[3] = rev ? root * v[2] : v[2];
      const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      const double inv = n > 0.0 ? 1.0 / n : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] *= inv;
    }
#pragma unroll 1
    for (int it = 0; it < POLISH_ITERS; ++it) {
#pragma unroll
      for (int i = 0; i < 9; ++i) e[i] = q[0] * basis[i] + q[1] * basis[9 + i] + q[2] * basis[18 + i] + q[3] * basis[27 + i];
      double g1[9], g2[9];                                        // E^T E, E E^T
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          g1[3 * r + c] = e[r] * e[c] + e[3 + r] * e[3 + c] + e[6 + r] * e[6 + c];
          g2[3 * r + c] = e[3 * r] * e[3 * c] + e[3 * r + 1] * e[3 * c + 1] + e[3 * r + 2] * e[3 * c + 2];
        }
      const double tr = g2[0] + g2[4] + g2[8];
      double res[11];
      res[0] = det3(e);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          res[1 + 3 * r + c] = 2.0 * (e[3 * r] * g1[c] + e[3 * r + 1] * g1[3 + c] + e[3 * r + 2] * g1[6 + c]) - tr * e[3 * r + c];
      res[10] = 0.5 * (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0);
      const double cof[9] = {e[4] * e[8] - e[5] * e[7], e[5] * e[6] - e[3] * e[8], e[3] * e[7] - e[4] * e[6],
                             e[7] * e[2] - e[8] * e[1], e[8] * e[0] - e[6] * e[2], e[6] * e[1] - e[7] * e[0],
                             e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]};
      double J[4][11];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double b[9], ebt[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) b[i] = basis[k * 9 + i];
        double d = 0.0, teb = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { d = __builtin_fma(cof[i], b[i], d); teb = __builtin_fma(e[i], b[i], teb); }
        J[k][0] = d;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) ebt[3 * r + c] = e[3 * r] * b[3 * c] + e[3 * r + 1] * b[3 * c + 1] + e[3 * r + 2] * b[3 * c + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double bg = b[3 * r] * g1[c] + b[3 * r + 1] * g1[3 + c] + b[3 * r + 2] * g1[6 + c];
            const double ebe = ebt[3 * r] * e[c] + ebt[3 * r + 1] * e[3 + c] + ebt[3 * r + 2] * e[6 + c];
            const double gb = g2[3 * r] * b[c] + g2[3 * r + 1] * b[3 + c] + g2[3 * r + 2] * b[6 + c];
            J[k][1 + 3 * r + c] = 2.0 * (bg + ebe + gb) - 2.0 * teb * e[3 * r + c] - tr * b[3 * r + c];
          }
        J[k][10] = q[k];
      }
      // normal equations (J^T J) dq = J^T res, elimination without pivoting (symmetric positive definite at a simple root)
      double Nm[4][5];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < 11; ++i) s = __builtin_fma(J[r][i], J[c][i], s);
          Nm[r][c] = s;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) s = __builtin_fma(J[r][i], res[i], s);
        Nm[r][4] = s;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double inv = 1.0 / Nm[c][c];
#pragma unroll
        for (int r = c + 1; r < 4; ++r) {
          const double f = Nm[r][c] * inv;
#pragma unroll
          for (int k = c + 1; k < 5; ++k) Nm[r][k] = __builtin_fma(-f, Nm[c][k], Nm[r][k]);
        }
      }
      double dq[4];
#pragma unroll
      for (int r = 3; r >= 0; --r) {
        double s = Nm[r][4];
#pragma unroll
        for (int k = r + 1; k < 4; ++k) s = __builtin_fma(-Nm[r][k], dq[k], s);
        dq[r] = s / Nm[r][r];
      }
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 4; ++i) fin = fin && isfinite(dq[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = fin ? q[i] - dq[i] : q[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = q[0] * basis[i] + q[1] * basis[9 + i] + q[2] * basis[18 + i] + q[3] * basis[27 + i];
    unit_frobenius(e);
  }
  bool fin = true;
  double fro = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) { fin = fin && isfinite(e[i]); fro += e[i] * e[i]; }
  const bool vr = live && good && has && fin && fro > 0.5;

  // ---- 7. slots in increasing z
  const uint32_t m32 = (uint32_t)(__ballot(vr) >> (tid & 32));
  const uint32_t mneg = (uint32_t)(__ballot(vr && rev && root < 0.0) >> (tid & 32)) >> 16;
  const uint32_t mp = m32 & 0xFFFFu, mpos = (m32 >> 16) & ~mneg;
  const uint32_t above = ~((2u << j) - 1u), below = (1u << j) - 1u;
  int rank;
  if (!rev) rank = __popc(mneg) + __popc(mp & below);
  else if (root < 0.0) rank = __popc(mneg & above);
  else rank = __popc(mneg) + __popc(mp) + __popc(mpos & above);
  const int total = min(__popc(m32), E_R);
  if (vr && rank < E_R) {
    valid[(size_t)t * E_R + rank] = 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) models[((size_t)t * E_R + rank) * 9 + i] = e[i];
  }
  if (live && ln < E_R && ln >= total) {
    valid[(size_t)t * E_R + ln] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) models[((size_t)t * E_R + ln) * 9 + i] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------ selection + local optimisation
// cand (LDS, 9) <- its projection onto the essential manifold (singular values (1, 1, 0) / sqrt 2), NaN when it has rank < 2.
// A, V: LDS scratch of jacobi_lds.  Every thread of the block calls it.
__device__ void project_essential(double* cand, double* A, double* V) {
  const int tid = threadIdx.x;
  if (tid < 9) {
    const int r = tid / 3, c = tid % 3;
    A[r * 9 + c] = cand[r] * cand[c] + cand[3 + r] * cand[3 + c] + cand[6 + r] * cand[6 + c];
    V[r * 9 + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  jacobi_lds(A, V, 3);
  if (tid == 0) {
    const int j3 = argmin_diag(A, 3), j1 = (j3 + 1) % 3, j2 = (j3 + 2) % 3;
    double v1[3], v2[3], u1[3], u2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { v1[i] = V[i * 9 + j1]; v2[i] = V[i * 9 + j2]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u1[r] = cand[3 * r] * v1[0] + cand[3 * r + 1] * v1[1] + cand[3 * r + 2] * v1[2];
      u2[r] = cand[3 * r] * v2[0] + cand[3 * r + 1] * v2[1] + cand[3 * r + 2] * v2[2];
    }
    const double i1 = 1.0 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] *= i1;
    const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
    const double i2 = 1.0 / sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] *= i2;
    double f[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) f[3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c];
    unit_frobenius(f);
#pragma unroll
    for (int i = 0; i < 9; ++i) cand[i] = f[i];
  }
  __syncthreads();
}

__device__ __forceinline__ bool finite9(const double* m) {
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) fin = fin && isfinite(m[i]);
  return fin;
}

template <int SCORE>
__global__ __launch_bounds__(256) void essential_select_kernel(const double* __restrict__ xh, const float4* __restrict__ pts,
                                                               const double* __restrict__ models, const double* __restrict__ cost,
                                                               int N, int M, float t2, int lo_iters, double* __restrict__ out_model,
                                                               unsigned char* __restrict__ mask) {
  __shared__ double dred[256];
  __shared__ int ired[256];
  __shared__ double A[81], V[81], cur[9], cand[9], wsum[4][45];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float4* pq = pts + (size_t)p * N;

  // 1. lowest cost, lowest slot index on ties
  double bc = INFINITY;
  int bm = -1;
  for (int m = tid; m < M; m += 256) {
    const double c = cost[(size_t)p * M + m];
    if (c < bc) { bc = c; bm = m; }
  }
  dred[tid] = bc;
  ired[tid] = bm;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const double c2 = dred[tid + o];
      const int m2 = ired[tid + o];
      if (m2 >= 0 && (ired[tid] < 0 || c2 < dred[tid] || (c2 == dred[tid] && m2 < ired[tid]))) { dred[tid] = c2; ired[tid] = m2; }
    }
    __syncthreads();
  }
  bm = ired[0];
  __syncthreads();
  if (bm < 0) {                                                   // no model: zeros and an empty mask (block-uniform)
    if (tid < 9) out_model[p * 9 + tid] = 0.0;
    for (int i = tid; i < N; i += 256) mask[(size_t)p * N + i] = 0;
    return;
  }
  if (tid < 9) cur[tid] = models[((size_t)p * M + bm) * 9 + tid];
  __syncthreads();
  double cc;
  int cn;
  block_score<KIND_F, SCORE>(cur, pq, N, 1.f, 1.f, t2, dred, ired, cc, cn);

  // 2. local optimisation: least squares on the inliers, projected onto the essential manifold, kept only if its cost is lower
  for (int round = 0; round < lo_iters; ++round) {
    if (cn < 8) break;
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (float)cur[i];
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.0;
    for (int i = tid; i < N; i += 256) {
      const float e = point_error<KIND_F>(m, pq[i], 1.f, 1.f);
      if (!(e < t2)) continue;
      const double* q = xh + ((size_t)p * N + i) * 4;
      const double x = q[0], y = q[1], u = q[2], v = q[3];
      double sw = 1.0;                                              // SCORE_MAGSAC: rows scaled by sqrt W under the current model
      if constexpr (SCORE == SCORE_MAGSAC) sw = sqrt((double)magsac_lookup(magsac_weight_cells, e, (float)MAGSAC_CELLS / t2));
      const double a[9] = {sw * (u * x), sw * (u * y), sw * u, sw * (v * x), sw * (v * y), sw * v, sw * x, sw * y, sw};
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c) { acc[k] = __builtin_fma(a[r], a[c], acc[k]); ++k; }
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) {
      double v = acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      acc[k] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 45; ++k) wsum[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < 81) {
      const int r = tid / 9, c = tid % 9, lo = min(r, c), hi = max(r, c);
      const int k = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
      A[tid] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
      V[tid] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi_lds(A, V, 9);
    const int j = argmin_diag(A, 9);
    __syncthreads();
    if (tid < 9) cand[tid] = V[tid * 9 + j];
    __syncthreads();
    project_essential(cand, A, V);
    if (!finite9(cand)) break;                                    // block-uniform (LDS)
    double c2;
    int n2;
    block_score<KIND_F, SCORE>(cand, pq, N, 1.f, 1.f, t2, dred, ired, c2, n2);
    if (!(c2 < cc)) break;
    if (tid < 9) cur[tid] = cand[tid];
    __syncthreads();
    cc = c2;
    cn = n2;
  }

  // 3. the returned model is on the manifold whatever the rounds did (a minimal model is there to ~1e-13 only); sign; mask
  if (tid < 9) cand[tid] = cur[tid];
  __syncthreads();
  project_essential(cand, A, V);
  const bool pf = finite9(cand);
  __syncthreads();
  if (tid == 0) {
    double o[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = pf ? cand[i] : cur[i];
    unit_frobenius(o);
    int jm = 0;
#pragma unroll
    for (int i = 1; i < 9; ++i)
      if (fabs(o[i]) > fabs(o[jm])) jm = i;
    const double sgn = o[jm] < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { o[i] *= sgn; cur[i] = o[i]; out_model[p * 9 + i] = o[i]; }
  }
  __syncthreads();
  float m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = (float)cur[i];
  for (int i = tid; i < N; i += 256) mask[(size_t)p * N + i] = point_error<KIND_F>(m, pq[i], 1.f, 1.f) < t2 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ pose recovery
__global__ __launch_bounds__(256) void recover_pose_kernel(const double* __restrict__ xa, const double* __restrict__ xb,
                                                           const double* __restrict__ Ka, const double* __restrict__ Kb,
                                                           const double* __restrict__ E, const unsigned char* mask_in, int N,
                                                           double* __restrict__ R_out, double* __restrict__ t_out,
                                                           int* __restrict__ count, unsigned char* mask_out) {
  __shared__ double A[81], V[81], e[9], Rc[2][9], tv[3];
  __shared__ int red[4][256];
  __shared__ int s_ok, s_best;
  const int p = blockIdx.x, tid = threadIdx.x;
  double ia[5], ib[5];
  const bool ka_ok = invert_k(Ka + p * 9, ia), kb_ok = invert_k(Kb + p * 9, ib), kok = ka_ok && kb_ok;
  if (tid < 9) e[tid] = E[p * 9 + tid];
  __syncthreads();
  if (tid < 9) {
    const int r = tid / 3, c = tid % 3;
    A[r * 9 + c] = e[r] * e[c] + e[3 + r] * e[3 + c] + e[6 + r] * e[6 + c];
    V[r * 9 + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  jacobi_lds(A, V, 3);
  if (tid == 0) {
    const int j3 = argmin_diag(A, 3), j1 = (j3 + 1) % 3, j2 = (j3 + 2) % 3;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) { v1[i] = V[i * 9 + j1]; v2[i] = V[i * 9 + j2]; }
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1]; v3[1] = v1[2] * v2[0] - v1[0] * v2[2]; v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    for (int r = 0; r < 3; ++r) {
      u1[r] = e[3 * r] * v1[0] + e[3 * r + 1] * v1[1] + e[3 * r + 2] * v1[2];
      u2[r] = e[3 * r] * v2[0] + e[3 * r + 1] * v2[1] + e[3 * r + 2] * v2[2];
    }
    const double i1 = 1.0 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    for (int i = 0; i < 3; ++i) u1[i] *= i1;
    const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
    const double i2 = 1.0 / sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int i = 0; i < 3; ++i) u2[i] *= i2;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    bool fin = kok;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        const double tw = u2[r] * v1[c] - u1[r] * v2[c], rest = u3[r] * v3[c];      // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T
        Rc[0][3 * r + c] = tw + rest;
        Rc[1][3 * r + c] = rest - tw;
        fin = fin && isfinite(tw) && isfinite(rest);
      }
      tv[r] = u3[r];
    }
    s_ok = fin ? 1 : 0;
  }
  __syncthreads();
  const bool ok = s_ok != 0;                                      // block-uniform
  if (!ok) {                                                      // zero / non-finite E or K: identity, no votes
    if (tid < 9) R_out[p * 9 + tid] = (tid % 4 == 0) ? 1.0 : 0.0;
    if (tid < 3) t_out[p * 3 + tid] = 0.0;
    if (tid == 0) count[p] = 0;
    for (int i = tid; i < N; i += 256) mask_out[(size_t)p * N + i] = 0;
    return;
  }
  double R0[9], R1[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) { R0[i] = Rc[0][i]; R1[i] = Rc[1][i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = tv[i];
  // bit c of the result: the match has positive, finite depth in both cameras under candidate c
  auto votes = [&](int i) -> int {
    const size_t q = ((size_t)p * N + i) * 2;
    if (mask_in && !mask_in[(size_t)p * N + i]) return 0;
    const double ax = xa[q], ay = xa[q + 1], bx = xb[q], by = xb[q + 1];
    const double x = ia[0] * ax + ia[1] * ay + ia[2], y = ia[3] * ay + ia[4];
    const double b0 = ib[0] * bx + ib[1] * by + ib[2], b1 = ib[3] * by + ib[4];
    const double bb = b0 * b0 + b1 * b1 + 1.0;
    const double bt = b0 * t[0] + b1 * t[1] + t[2];
    int out = 0;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const double* R = w == 0 ? R0 : R1;
      const double a0 = R[0] * x + R[1] * y + R[2], a1 = R[3] * x + R[4] * y + R[5], a2 = R[6] * x + R[7] * y + R[8];
      const double aa = a0 * a0 + a1 * a1 + a2 * a2, ab = a0 * b0 + a1 * b1 + a2;
      const double at = a0 * t[0] + a1 * t[1] + a2 * t[2];
      const double det = aa * bb - ab * ab;
      // t -> -t flips the sign of both depths
      const double la = (ab * bt - bb * at) / det, lb = (aa * bt - ab * at) / det;
      const bool fin = isfinite(la) && isfinite(lb);
      out |= (fin && la > 0.0 && lb > 0.0) ? (1 << (2 * w)) : 0;
      out |= (fin && la < 0.0 && lb < 0.0) ? (2 << (2 * w)) : 0;
    }
    return out;
  };
  int n[4] = {0, 0, 0, 0};
  for (int i = tid; i < N; i += 256) {
    const int v = votes(i);
#pragma unroll
    for (int c = 0; c < 4; ++c) n[c] += (v >> c) & 1;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) red[c][tid] = n[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int c = 0; c < 4; ++c) red[c][tid] += red[c][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int best = 0;
    for (int c = 1; c < 4; ++c)
      if (red[c][0] > red[best][0]) best = c;
    s_best = best;
    count[p] = red[best][0];
  }
  __syncthreads();
  const int best = s_best;
  if (tid < 9) R_out[p * 9 + tid] = Rc[best >> 1][tid];
  if (tid < 3) t_out[p * 3 + tid] = (best & 1) ? -tv[tid] : tv[tid];
  for (int i = tid; i < N; i += 256) mask_out[(size_t)p * N + i] = (votes(i) >> best) & 1;
}

// --------------------------------------------------------------------------------------------------------------- workspace
// ransac_common.h's regions, then the calibrated points xh
constexpr int WE_XH = WS_N, WE_N = WS_N + 1;

long layout_e(int P, int N, int iters, long* off) {
  const long xh_bytes = (long)P * N * 32;
  return ws_layout(E_S, E_R, P, N, iters, &xh_bytes, 1, off);
}

int check_args_e(const char* fn, const void* xa, const void* xb, const void* Ka, const void* Kb, const void* ws, int P, int N,
                 int iters, float threshold, long ws_bytes) {
  ROMA_REQUIRE(xa && xb && Ka && Kb && ws, ROMA_E_ARG, "%s: null pointer", fn);
  const int rc = check_problem(fn, P, N, iters, E_S, GROUPS, threshold);
  return rc ? rc : check_workspace(fn, ws_bytes, layout_e(P, N, iters, nullptr));
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_essential_workspace(int P, int N, int iters, long* offsets) {
  if (P < 1 || N < 1 || iters < 1) {
    set_error("roma_essential_workspace: bad arguments P=%d N=%d iters=%d", P, N, iters);
    return ROMA_E_ARG;
  }
  return layout_e(P, N, iters, offsets);
}

namespace {

int essential_hypotheses(const char* fn, const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                         float threshold, int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  int rc = check_args_e(fn, xa, xb, Ka, Kb, ws, P, N, iters, threshold, ws_bytes);
  if (rc) return rc;
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_pair_offset(fn, p0);
  if (rc) return rc;
  long off[WE_N];
  layout_e(P, N, iters, off);
  const Regions r = regions(ws, off);
  double* xh = region<double>(ws, off, WE_XH);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int M = iters * E_R, C = (N + CHUNK - 1) / CHUNK;
  const uint32_t sstream = sample_stream(seed, STAGE_E);
  const float t2 = threshold * threshold;
  const Grids g = ransac_grids(P, N, iters, E_R, GROUPS);
  hipLaunchKernelGGL(calibrate_kernel, dim3(P), dim3(256), 0, st, xa, xb, Ka, Kb, N, r.norm, (float*)r.pts, xh);
  hipLaunchKernelGGL(five_point_kernel, g.solve, dim3(256), 0, st, xh, (const float*)r.pts, P, N, iters, sstream, p0, r.samples, r.models,
                     r.valid);
  const auto score = by_scoring(scoring, score_kernel<KIND_F, SCORE_MSAC>, score_kernel<KIND_F, SCORE_MAGSAC>);
  hipLaunchKernelGGL(score, g.score, dim3(256), 0, st, r.pts, r.norm, r.models, r.valid, N, M, t2, r.slab_cost, r.slab_cnt);
  hipLaunchKernelGGL(reduce_kernel, g.reduce, dim3(256), 0, st, r.slab_cost, r.slab_cnt, r.valid, P, M, C, r.cost, r.count);
  return check_launch(fn);
}

int essential_select(const char* fn, const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                     float threshold, int scoring, int lo_iters, const void* ws, long ws_bytes, double* E, unsigned char* mask,
                     void* stream) {
  int rc = check_args_e(fn, xa, xb, Ka, Kb, ws, P, N, iters, threshold, ws_bytes);
  if (rc) return rc;
  ROMA_REQUIRE(E && mask, ROMA_E_ARG, "%s: null pointer", fn);
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_lo_iters(fn, lo_iters);
  if (rc) return rc;
  long off[WE_N];
  layout_e(P, N, iters, off);
  const Regions r = regions(ws, off);
  const auto sel = by_scoring(scoring, essential_select_kernel<SCORE_MSAC>, essential_select_kernel<SCORE_MAGSAC>);
  hipLaunchKernelGGL(sel, dim3(P), dim3(256), 0, static_cast<hipStream_t>(stream), region<double>(ws, off, WE_XH), r.pts, r.models, r.cost, N,
                     iters * E_R, threshold * threshold, lo_iters, E, mask);
  return check_launch(fn);
}

}  // namespace

extern "C" int roma_essential_hypotheses(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N,
                                         int iters, float threshold, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  return essential_hypotheses(__func__, xa, xb, Ka, Kb, P, N, iters, threshold, SCORE_MSAC, seed, p0, ws, ws_bytes, stream);
}

extern "C" int roma_essential_hypotheses_ex(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N,
                                            int iters, float threshold, int scoring, unsigned seed, int p0, void* ws, long ws_bytes,
                                            void* stream) {
  return essential_hypotheses(__func__, xa, xb, Ka, Kb, P, N, iters, threshold, scoring, seed, p0, ws, ws_bytes, stream);
}

extern "C" int roma_essential_select(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                                     float threshold, int lo_iters, const void* ws, long ws_bytes, double* E, unsigned char* mask,
                                     void* stream) {
  return essential_select(__func__, xa, xb, Ka, Kb, P, N, iters, threshold, SCORE_MSAC, lo_iters, ws, ws_bytes, E, mask, stream);
}

extern "C" int roma_essential_select_ex(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                                        float threshold, int scoring, int lo_iters, const void* ws, long ws_bytes, double* E,
                                        unsigned char* mask, void* stream) {
  return essential_select(__func__, xa, xb, Ka, Kb, P, N, iters, threshold, scoring, lo_iters, ws, ws_bytes, E, mask, stream);
}

extern "C" int roma_recover_pose(const double* xa, const double* xb, const double* Ka, const double* Kb, const double* E,
                                 const unsigned char* mask_in, int P, int N, double* R, double* t, int* count, unsigned char* mask_out,
                                 void* stream) {
  ROMA_REQUIRE(xa && xb && Ka && Kb && E && R && t && count && mask_out, ROMA_E_ARG, "roma_recover_pose: null pointer");
  ROMA_REQUIRE(P >= 1 && P <= (1 << 24), ROMA_E_SHAPE, "roma_recover_pose: bad shape P=%d", P);
  ROMA_REQUIRE(N >= E_S && N <= (1 << 26), ROMA_E_SHAPE, "roma_recover_pose: N=%d matches, need at least %d", N, E_S);
  hipLaunchKernelGGL(recover_pose_kernel, dim3(P), dim3(256), 0, static_cast<hipStream_t>(stream), xa, xb, Ka, Kb, E, mask_in, N, R, t,
                     count, mask_out);
  ROMA_CHECK_LAUNCH();
}
