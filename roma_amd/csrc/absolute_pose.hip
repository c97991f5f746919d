// Absolute pose: RANSAC on 2D-3D matches (P3P minimal solver) and non-linear refinement — what a caller runs to place a further image
// against the point cloud of triangulate.hip or a depth map, where the host path calls cv2.solvePnPRansac or
// poselib.estimate_absolute_pose.  Convention x ~ K (R X + t): X in any world frame, x in pixels of the image being placed, K upper
// triangular with last row 0 0 1.  Ground rules of geometry.hip: fp64 minimal solver, fp32 scoring of every slot (MSAC or MAGSAC++),
// fixed number of samples, no atomics, no allocation, no host synchronisation, sums in a fixed order: bitwise reproducible, and a
// pair's result does not depend on the rest of the batch.  DESIGN.md §3.4; tests/absolute_pose_ref.py restates it in numpy.
//
// Pipeline, one call of roma_absolute_pose_hypotheses + one of roma_absolute_pose_select (P pairs of N matches, iters samples each):
//   ap_prepare_kernel  one block/pair   centroid c and scale s of the world points over the finite rows (fp64, fixed-order LDS tree, mean
//                                       distance sqrt 3); X' = s (X - c).  Scoring record (X', u) fp32 + v fp32, and the fp64 copy
//                                       (X', K^-1 x) the solver reads; NaN rows where X or x is not finite, everywhere for a singular K
//   p3p_kernel         one lane/sample  draws the sample (geometry.hip's scheme, stage 5) and solves P3P in fp64 -> 4 slots (R, t')
//   ap_score_kernel    the score_kernel pattern of ransac_common.h: 1024-point chunks in LDS, one slot per thread, broadcast reads,
//                      partial cost and count into the slab; M = K [R | t'] composed once per slot in fp32, a point costs three dot
//                      products, one reciprocal and the squared pixel distance; M_2 . X' <= 0 (behind the camera) is an outlier
//   reduce_kernel      (ransac_common.h)
//   ap_select_kernel   one block/pair   lowest cost (lowest slot on ties), lo_iters rounds of the refinement's LM step at lambda_0 on
//                                       the inliers (weight W for MAGSAC++, 1 for MSAC), each kept only if the fp32 re-score drops
// and, on its own, refine_absolute_pose_kernel (one workgroup of 256 per pair, the schedule of pose_refine.hip).
// Internally the pose is (R, t' = s (R c + t)) on X'; (R, t = t' / s - R c) is what the entry points return.  The normalisation is
// what lets fp32 score a world that sits 1e4 units from its origin, and it turns the rotation of an LM step about the cloud's centre.
//
// P3P.  The solver intersects two conics in the depths (the formulation of Persson & Nordberg's Lambda Twist, with the degenerate
// conic split by its adjugate as in Richter-Gebert): one cubic root and 3 x 3 algebra, so a sample fits one lane.
//   f_i = (K^-1 x_i, 1) / |.|, c_ij = f_i . f_j, a_ij = |X'_i - X'_j|^2; the depths d satisfy d^T M_ij d = a_ij
//   rejected: |(X_2 - X_1) x (X_3 - X_1)| <= 1e-6 |X_2 - X_1| |X_3 - X_1| (collinear, or two points coincide)
//   D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23: d^T D1 d = d^T D2 d = 0.  det(alpha D1 + beta D2) = k0 alpha^3 + k1 alpha^2 beta +
//   k2 alpha beta^2 + k3 beta^3; the side with the larger of |k0|, |k3| is made monic (rejected when that is <= 1e-12 max |k|), one real
//   root in closed form (of three, the one with the largest |derivative|), two Newton steps
//   D0 = the degenerate member; B = -adj D0 = p p^T with p = l x m: p from the column of the largest diagonal entry of B (rejected
//   when that is <= 0: no real lines), D0 + [p]x = 2 m l^T: l = the row, m = the column of its largest entry
//   on each line the other conic is a quadratic in one depth ratio; a real root with three positive depths is scaled by
//   d^T (M12 + M13 + M23) d = a12 + a13 + a23
//   (R, t') from the camera points d_i f_i and the X'_i (the frames (e1, e2, e1 x e2) of both triangles), R made orthonormal, then 2
//   undamped Gauss-Newton steps on the sample's six reprojection equations in calibrated coordinates (the refinement's Jacobian);
//   kept when finite with the three points in front
//   slots: line l before line m, on a line the root -sqrt before +sqrt, kept solutions first; unused slots zero and invalid
//
// Refinement (and the round of the select kernel): 6 parameters, R <- exp([w]x) R (|w| limited to 1 rad, re-orthonormalised before
// it is evaluated), t' <- t' + delta.  Residual (u, v) - x in pixels; cost = sum of min(e, thr^2) over the usable matches (finite,
// allowed by mask_in, in front of the camera).  Analytic Jacobian; one pass forms 21 + 6 sums plus cost and count by block_sum, the
// step is solve_step<6>.  lambda_0 = 1e-3, kept when cost' < cost (1 - 1e-12), lambda / 10 (not below 1e-10) or x 10, `iters`
// steps, ended early by a step that moves no bit.  Fewer than 4 weighted matches, a pivot that is not positive or an input that is not
// finite: the input pose comes back bit for bit with steps = 0 and its own mask, cost and count.  The pass (ap_evaluate) and the step
// (ap_apply_step) are one device function each, shared by the refinement and the select kernel.
#include "ransac_common.h"

namespace roma {
namespace {

constexpr int AP_S = 3, AP_R = 4;
constexpr int AP_POLISH = 2;
constexpr int P3P_THREADS = 128;
constexpr int AP_THREADS = 256, AP_WAVES = AP_THREADS / 64;
constexpr int AP_NPAR = 6, AP_NTRI = 21, AP_NSUM = 29;       // 21 + 6 + cost + count
constexpr int AP_COST = 27, AP_COUNT = 28;
constexpr int AP_MIN_MATCHES = 4;
constexpr double AP_LAMBDA0 = 1e-3, AP_LAMBDA_MIN = 1e-10, AP_ACCEPT_REL = 1e-12;
constexpr double AP_LEAD_TOL = 1e-12;
constexpr double AP_PI = 3.141592653589793;

struct Cam {
  double fx, sk, cx, fy, cy;
};

__device__ __forceinline__ Cam load_cam(const double* K) { return Cam{K[0], K[1], K[2], K[4], K[5]}; }

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// ------------------------------------------------------------------------------------------- residual, Jacobian, step (fp64)
// One match under (R, t): squared error e in pixels, depth z, residual (ru, rv), Jacobian by (w, dt).  Nothing is guarded: a row that
// is not finite, or z = 0, gives NaN / inf, which the callers' comparisons turn down.
struct ApPoint {
  double e, z, ru, rv, Ju[AP_NPAR], Jv[AP_NPAR];
};

__device__ __forceinline__ void ap_point(const double* R, const double* t, const Cam& k, const double* X, double xu, double xv, ApPoint& o) {
  double Q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) Q[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2];
  const double y0 = Q[0] + t[0], y1 = Q[1] + t[1];
  o.z = Q[2] + t[2];
  const double iz = 1.0 / o.z, a = y0 * iz, b = y1 * iz;
  o.ru = k.fx * a + k.sk * b + k.cx - xu;
  o.rv = k.fy * b + k.cy - xv;
  o.e = o.ru * o.ru + o.rv * o.rv;
  // dY / d(w, dt): dY = w x Q + dt
  const double d0[AP_NPAR] = {0.0, Q[2], -Q[1], 1.0, 0.0, 0.0};
  const double d1[AP_NPAR] = {-Q[2], 0.0, Q[0], 0.0, 1.0, 0.0};
  const double d2[AP_NPAR] = {Q[1], -Q[0], 0.0, 0.0, 0.0, 1.0};
#pragma unroll
  for (int j = 0; j < AP_NPAR; ++j) {
    const double da = (d0[j] - a * d2[j]) * iz, db = (d1[j] - b * d2[j]) * iz;
    o.Ju[j] = k.fx * da + k.sk * db;
    o.Jv[j] = k.fy * db;
  }
}

// s[0..20] += wgt J^T J (upper triangle, row by row), s[21..26] += wgt J^T r
__device__ __forceinline__ void ap_accumulate(const ApPoint& q, double wgt, double* s) {
  int o = 0;
#pragma unroll
  for (int a = 0; a < AP_NPAR; ++a) {
    const double wu = wgt * q.Ju[a], wv = wgt * q.Jv[a];
#pragma unroll
    for (int b = a; b < AP_NPAR; ++b, ++o) s[o] = __builtin_fma(wu, q.Ju[b], __builtin_fma(wv, q.Jv[b], s[o]));
    s[AP_NTRI + a] = __builtin_fma(wu, q.ru, __builtin_fma(wv, q.rv, s[AP_NTRI + a]));
  }
}

// Rc = orthonormalised exp([w]x) R, tc = t + dt; the rotation of one step is limited to 1 rad, where so3_exp_series is exact
__device__ __forceinline__ void ap_apply_step(const double* R, const double* t, const double (&delta)[AP_NPAR], double* Rc, double* tc) {
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
  double KR[9], KKR[9], X[9];
  skew_times(w, R, KR);
  skew_times(w, KR, KKR);
#pragma unroll
  for (int i = 0; i < 9; ++i) X[i] = R[i] + A * KR[i] + B * KKR[i];
  orthonormalise_rows(X, Rc);
#pragma unroll
  for (int i = 0; i < 3; ++i) tc[i] = t[i] + delta[3 + i];
}

// The 29 sums of one pose (R, t') over the pair's matches, reduced: on return every thread holds the same s[].  Matches are read in
// world coordinates and normalised on the way (3 subtractions and 3 products against a few hundred operations of the Jacobian).
// WEIGHT = SCORE_MAGSAC: an inlier's row is weighted by W(e / thr^2) of magsac_table.h, else by 1.
template <int WEIGHT>
__device__ __forceinline__ void ap_evaluate(const double* R, const double* t, const Cam& cam, bool kok, const double* __restrict__ Xw,
                                            const double2* __restrict__ xp, const unsigned char* mask_in, size_t base, int N,
                                            const double* c, double sc, double t2, double (*red)[AP_NSUM], double (&s)[AP_NSUM]) {
#pragma unroll
  for (int k = 0; k < AP_NSUM; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < N; i += AP_THREADS) {
    const double* xw = Xw + (base + i) * 3;
    const double2 px = xp[base + i];
    const double X[3] = {(xw[0] - c[0]) * sc, (xw[1] - c[1]) * sc, (xw[2] - c[2]) * sc};
    const bool ok = kok && isfinite(xw[0]) && isfinite(xw[1]) && isfinite(xw[2]) && isfinite(px.x) && isfinite(px.y) &&
                    (!mask_in || mask_in[base + i] != 0);
    ApPoint q;
    ap_point(R, t, cam, X, px.x, px.y, q);
    const bool front = ok && q.z > 0.0, in = front && q.e < t2;
    double wgt = in ? 1.0 : 0.0;
    if constexpr (WEIGHT == SCORE_MAGSAC) {
      if (in) wgt = (double)magsac_lookup(magsac_weight_cells, (float)q.e, (float)MAGSAC_CELLS / (float)t2);
    }
    s[AP_COST] += front ? (in ? q.e : t2) : 0.0;
    s[AP_COUNT] += in ? 1.0 : 0.0;
    if (!in) {
      q.ru = 0.0; q.rv = 0.0;
#pragma unroll
      for (int j = 0; j < AP_NPAR; ++j) { q.Ju[j] = 0.0; q.Jv[j] = 0.0; }
    }
    ap_accumulate(q, wgt, s);
  }
  block_sum<AP_NSUM, AP_WAVES>(s, red);
}

// ------------------------------------------------------------------------------------------------------------------ prepare
// norm[p*8 + {0,1,2,3}] = (cx, cy, cz, s); pts: (P,N) float4 (X', u); pv: (P,N) float v; xn: (P,N,5) fp64 (X', K^-1 x)
__global__ __launch_bounds__(256) void ap_prepare_kernel(const double* __restrict__ Xw, const double* __restrict__ xp,
                                                         const double* __restrict__ K, int N, double* __restrict__ norm,
                                                         float4* __restrict__ pts, float* __restrict__ pv, double* __restrict__ xn) {
  __shared__ double red[3][256];
  __shared__ int ired[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* X = Xw + (size_t)p * N * 3;
  const double* x = xp + (size_t)p * N * 2;
  double ki[5];
  const bool kok = invert_k(K + p * 9, ki);
  auto finite_row = [&](int i) {
    return isfinite(X[3 * i]) && isfinite(X[3 * i + 1]) && isfinite(X[3 * i + 2]) && isfinite(x[2 * i]) && isfinite(x[2 * i + 1]);
  };
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int n = 0;
  for (int i = tid; i < N; i += 256)
    if (finite_row(i)) { s0 += X[3 * i]; s1 += X[3 * i + 1]; s2 += X[3 * i + 2]; ++n; }
  red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2; ired[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o];
      ired[tid] += ired[tid + o];
    }
    __syncthreads();
  }
  const int cnt = ired[0];
  const double c0 = cnt > 0 ? red[0][0] / cnt : 0.0, c1 = cnt > 0 ? red[1][0] / cnt : 0.0, c2 = cnt > 0 ? red[2][0] / cnt : 0.0;
  __syncthreads();
  double sd = 0.0;
  for (int i = tid; i < N; i += 256)
    if (finite_row(i)) {
      const double d0 = X[3 * i] - c0, d1 = X[3 * i + 1] - c1, d2 = X[3 * i + 2] - c2;
      sd += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    }
  red[0][tid] = sd;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[0][tid] += red[0][tid + o];
    __syncthreads();
  }
  const double md = cnt > 0 ? red[0][0] / cnt : 0.0;
  double s = 1.7320508075688772 / md;
  if (!(md > 0.0) || !isfinite(s)) s = 1.0;                       // identical points (or none finite): every sample is degenerate
  if (tid < 8) norm[p * 8 + tid] = tid == 0 ? c0 : tid == 1 ? c1 : tid == 2 ? c2 : tid == 3 ? s : 0.0;
  const double nan = __builtin_nan("");
  const float nanf = __builtin_nanf("");
  for (int i = tid; i < N; i += 256) {
    const size_t q = (size_t)p * N + i;
    const double u = x[2 * i], v = x[2 * i + 1];
    double o[5];
    o[0] = (X[3 * i] - c0) * s;
    o[1] = (X[3 * i + 1] - c1) * s;
    o[2] = (X[3 * i + 2] - c2) * s;
    o[3] = ki[0] * u + ki[1] * v + ki[2];
    o[4] = ki[3] * v + ki[4];
    const bool ok = kok && finite_row(i) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(o[3]) && isfinite(o[4]);
#pragma unroll
    for (int k = 0; k < 5; ++k) xn[q * 5 + k] = ok ? o[k] : nan;
    pts[q] = ok ? make_float4((float)o[0], (float)o[1], (float)o[2], (float)u) : make_float4(nanf, nanf, nanf, nanf);
    pv[q] = ok ? (float)v : nanf;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- P3P
// one real root of x^3 + A x^2 + B x + C
__device__ __forceinline__ double cubic_real_root(double A, double B, double C) {
  const double p = B - A * A / 3.0;
  const double q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + C;
  const double disc = q * q / 4.0 + p * p * p / 27.0;
  double x;
  if (disc > 0.0) {
    const double sq = sqrt(disc);
    const double u = cbrt(-q / 2.0 - (q >= 0.0 ? sq : -sq));
    const double y = u != 0.0 ? u - p / (3.0 * u) : 0.0;
    x = y - A / 3.0;
  } else {
    const double r = 2.0 * sqrt(fmax(-p / 3.0, 0.0));
    const double pr = p * r;
    const double cphi = pr != 0.0 ? fmin(fmax(3.0 * q / pr, -1.0), 1.0) : 0.0;
    const double phi = acos(cphi);
    double best = -1.0;
    x = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double xk = r * cos((phi - 2.0 * AP_PI * k) / 3.0) - A / 3.0;
      const double d = fabs((3.0 * xk + 2.0 * A) * xk + B);
      const bool gt = d > best;
      x = gt ? xk : x;
      best = gt ? d : best;
    }
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double f = ((x + A) * x + B) * x + C;
    const double df = (3.0 * x + 2.0 * A) * x + B;
    if (df != 0.0) x -= f / df;
  }
  return x;
}

__device__ __forceinline__ double sel3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// a^T Q b for a symmetric or general 3 x 3 Q (row major)
__device__ __forceinline__ double qform(const double* a, const double* Q, const double* b) {
  return a[0] * (Q[0] * b[0] + Q[1] * b[1] + Q[2] * b[2]) + a[1] * (Q[3] * b[0] + Q[4] * b[1] + Q[5] * b[2]) +
         a[2] * (Q[6] * b[0] + Q[7] * b[1] + Q[8] * b[2]);
}

// samples: (P, iters, 3) int32; models: (P, iters, 4, 9) fp64 R; tvec: (P, iters, 4, 3) fp64 t'; valid: (P, iters, 4)
__global__ __launch_bounds__(P3P_THREADS) void p3p_kernel(const double* __restrict__ xn, const float4* __restrict__ pts, int P, int N,
                                                          int iters, uint32_t stream, int p0, int* __restrict__ samples,
                                                          double* __restrict__ models, double* __restrict__ tvec,
                                                          int* __restrict__ valid) {
  const long t = (long)blockIdx.x * P3P_THREADS + threadIdx.x;
  if (t >= (long)P * iters) return;
  const int p = (int)(t / iters), h = (int)(t % iters);
  const size_t base = (size_t)p * N;

  int idx[AP_S];
  bool ok;
  draw_sample<AP_S>(stream, (uint32_t)(p0 + p), iters, h, N, [&](int i) { const float v = pts[base + i].x; return v == v; }, idx, ok);
#pragma unroll
  for (int k = 0; k < AP_S; ++k) samples[(size_t)t * AP_S + k] = ok ? idx[k] : -1;
  double* out_R = models + (size_t)t * AP_R * 9;
  double* out_t = tvec + (size_t)t * AP_R * 3;
  int* out_v = valid + (size_t)t * AP_R;
  int nsol = 0;

  double Xs[3][3], bs[3][2], f[3][3];
#pragma unroll
  for (int k = 0; k < AP_S; ++k) {
    const double* q = xn + (base + (ok ? idx[k] : 0)) * 5;
    Xs[k][0] = q[0]; Xs[k][1] = q[1]; Xs[k][2] = q[2];
    bs[k][0] = q[3]; bs[k][1] = q[4];
    const double inv = 1.0 / sqrt(q[3] * q[3] + q[4] * q[4] + 1.0);
    f[k][0] = q[3] * inv; f[k][1] = q[4] * inv; f[k][2] = inv;
  }
  double e1[3], e2[3], e3[3], cr[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { e1[i] = Xs[1][i] - Xs[0][i]; e2[i] = Xs[2][i] - Xs[0][i]; e3[i] = Xs[2][i] - Xs[1][i]; }
  cross3(e1, e2, cr);
  const double a12 = dot3(e1, e1), a13 = dot3(e2, e2), a23 = dot3(e3, e3);
  bool good = ok && sqrt(dot3(cr, cr)) > COLLINEAR_TOL * sqrt(a12) * sqrt(a13);
  const double c12 = dot3(f[0], f[1]), c13 = dot3(f[0], f[2]), c23 = dot3(f[1], f[2]);
  const double D1[9] = {a23, -a23 * c12, 0.0, -a23 * c12, a23 - a12, a12 * c23, 0.0, a12 * c23, -a12};
  const double D2[9] = {a23, 0.0, -a23 * c13, 0.0, -a13, a13 * c23, -a23 * c13, a13 * c23, a23 - a13};
  const double k0 = det3(D1), k3 = det3(D2);
  double k1 = 0.0, k2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double m1[9], m2[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { m1[j] = j / 3 == i ? D2[j] : D1[j]; m2[j] = j / 3 == i ? D1[j] : D2[j]; }
    k1 += det3(m1);
    k2 += det3(m2);
  }
  const double kmax = fmax(fmax(fabs(k0), fabs(k1)), fmax(fabs(k2), fabs(k3)));
  const bool side = fabs(k3) >= fabs(k0);
  const double lead = side ? k3 : k0;
  good = good && fabs(lead) > AP_LEAD_TOL * kmax;
  if (good) {
    const double g = side ? cubic_real_root(k2 / k3, k1 / k3, k0 / k3) : cubic_real_root(k1 / k0, k2 / k0, k3 / k0);
    double D0[9], Q[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { D0[i] = side ? D1[i] + g * D2[i] : g * D1[i] + D2[i]; Q[i] = side ? D2[i] : D1[i]; }
    // B = -adj D0 (symmetric)
    const double B00 = -(D0[4] * D0[8] - D0[5] * D0[7]), B01 = -(D0[5] * D0[6] - D0[3] * D0[8]), B02 = -(D0[3] * D0[7] - D0[4] * D0[6]);
    const double B11 = -(D0[0] * D0[8] - D0[2] * D0[6]), B12 = -(D0[1] * D0[6] - D0[0] * D0[7]), B22 = -(D0[0] * D0[4] - D0[1] * D0[3]);
    int bi = 0;
    double bb = B00;
    if (B11 > bb) { bi = 1; bb = B11; }
    if (B22 > bb) { bi = 2; bb = B22; }
    if (bb > 0.0) {
      const double sb = sqrt(bb);
      const double pv[3] = {sel3(bi, B00, B01, B02) / sb, sel3(bi, B01, B11, B12) / sb, sel3(bi, B02, B12, B22) / sb};
      const double Nm[9] = {D0[0], D0[1] - pv[2], D0[2] + pv[1], D0[3] + pv[2], D0[4], D0[5] - pv[0], D0[6] - pv[1], D0[7] + pv[0], D0[8]};
      int ij = 0;
      double nb = fabs(Nm[0]);
#pragma unroll
      for (int i = 1; i < 9; ++i) {
        const bool gt = fabs(Nm[i]) > nb;
        ij = gt ? i : ij;
        nb = gt ? fabs(Nm[i]) : nb;
      }
      const int row = ij / 3, col = ij % 3;
      const double lines[2][3] = {{sel3(row, Nm[0], Nm[3], Nm[6]), sel3(row, Nm[1], Nm[4], Nm[7]), sel3(row, Nm[2], Nm[5], Nm[8])},
                                  {sel3(col, Nm[0], Nm[1], Nm[2]), sel3(col, Nm[3], Nm[4], Nm[5]), sel3(col, Nm[6], Nm[7], Nm[8])}};
      // the inverse of [e1 e2 cr] (columns), shared by the solutions: its rows are (e2 x cr, cr x e1, e1 x e2) / det
      double Ai[9];
      {
        double r0[3], r1[3];
        cross3(e2, cr, r0);
        cross3(cr, e1, r1);
        const double idet = 1.0 / dot3(e1, r0);
#pragma unroll
        for (int i = 0; i < 3; ++i) { Ai[i] = r0[i] * idet; Ai[3 + i] = r1[i] * idet; Ai[6 + i] = cr[i] * idet; }
      }
      const double asum = a12 + a13 + a23;
      const double Ms[9] = {2.0, -c12, -c13, -c12, 2.0, -c23, -c13, -c23, 2.0};
      const Cam unit{1.0, 0.0, 0.0, 1.0, 0.0};
#pragma unroll 1
      for (int li = 0; li < 2; ++li) {
        const double L[3] = {lines[li][0], lines[li][1], lines[li][2]};
        int k = 0;
        double lk = fabs(L[0]);
        if (fabs(L[1]) > lk) { k = 1; lk = fabs(L[1]); }
        if (fabs(L[2]) > lk) { k = 2; lk = fabs(L[2]); }
        if (!(lk > 0.0)) continue;
        const int i = k == 0 ? 1 : 0, j = k == 2 ? 1 : 2;
        const double Lk = sel3(k, L[0], L[1], L[2]), Li = sel3(i, L[0], L[1], L[2]), Lj = sel3(j, L[0], L[1], L[2]);
        double u[3], w[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          u[c] = c == k ? -Li / Lk : (c == i ? 1.0 : 0.0);
          w[c] = c == k ? -Lj / Lk : (c == j ? 1.0 : 0.0);
        }
        const double qa = qform(u, Q, u), qb = 2.0 * qform(u, Q, w), qc = qform(w, Q, w);
        const double disc = qb * qb - 4.0 * qa * qc;
        if (!(disc >= 0.0)) continue;
        const double sq = sqrt(disc);
#pragma unroll 1
        for (int si = 0; si < 2; ++si) {
          const double al = (-qb + (si == 0 ? -sq : sq)) / (2.0 * qa);
          double d[3] = {al * u[0] + w[0], al * u[1] + w[1], al * u[2] + w[2]};
          const double sc = sqrt(asum / qform(d, Ms, d));
#pragma unroll
          for (int c = 0; c < 3; ++c) d[c] *= sc;
          if (!(isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && d[0] > 0.0 && d[1] > 0.0 && d[2] > 0.0)) continue;
          // (R, t') from the camera points Y_i = d_i f_i
          double Y[3][3], g1[3], g2[3], gc[3], Rm[9], R[9], tt[3];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[a][c] = d[a] * f[a][c];
#pragma unroll
          for (int c = 0; c < 3; ++c) { g1[c] = Y[1][c] - Y[0][c]; g2[c] = Y[2][c] - Y[0][c]; }
          cross3(g1, g2, gc);
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Rm[3 * r + c] = g1[r] * Ai[c] + g2[r] * Ai[3 + c] + gc[r] * Ai[6 + c];
          orthonormalise_rows(Rm, R);
#pragma unroll
          for (int r = 0; r < 3; ++r) tt[r] = Y[0][r] - (R[3 * r] * Xs[0][0] + R[3 * r + 1] * Xs[0][1] + R[3 * r + 2] * Xs[0][2]);
#pragma unroll 1
          for (int it = 0; it < AP_POLISH; ++it) {
            double s[AP_NTRI + AP_NPAR];
#pragma unroll
            for (int a = 0; a < AP_NTRI + AP_NPAR; ++a) s[a] = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              ApPoint q;
              ap_point(R, tt, unit, Xs[a], bs[a][0], bs[a][1], q);
              ap_accumulate(q, 1.0, s);
            }
            double delta[AP_NPAR];
            bool fin = solve_step<AP_NPAR>(s, s + AP_NTRI, 0.0, delta);
#pragma unroll
            for (int a = 0; a < AP_NPAR; ++a) fin = fin && isfinite(delta[a]);
            if (!fin) break;
            double Rc[9], tc[3];
            ap_apply_step(R, tt, delta, Rc, tc);
#pragma unroll
            for (int a = 0; a < 9; ++a) R[a] = Rc[a];
#pragma unroll
            for (int a = 0; a < 3; ++a) tt[a] = tc[a];
          }
          bool keep = nsol < AP_R;
#pragma unroll
          for (int a = 0; a < 9; ++a) keep = keep && isfinite(R[a]);
#pragma unroll
          for (int a = 0; a < 3; ++a)
            keep = keep && isfinite(tt[a]) && (R[6] * Xs[a][0] + R[7] * Xs[a][1] + R[8] * Xs[a][2] + tt[2]) > 0.0;
          if (keep) {
#pragma unroll
            for (int a = 0; a < 9; ++a) out_R[nsol * 9 + a] = R[a];
#pragma unroll
            for (int a = 0; a < 3; ++a) out_t[nsol * 3 + a] = tt[a];
            out_v[nsol] = 1;
            ++nsol;
          }
        }
      }
    }
  }
  for (int sl = nsol; sl < AP_R; ++sl) {
    for (int a = 0; a < 9; ++a) out_R[sl * 9 + a] = 0.0;
    for (int a = 0; a < 3; ++a) out_t[sl * 3 + a] = 0.0;
    out_v[sl] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------ scoring (fp32)
// M = K [R | t'] (row major 3 x 4) in fp32
__device__ __forceinline__ void compose_projection(const double* R, const double* t, const Cam& k, float* M) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
    M[c] = (float)(k.fx * r0 + k.sk * r1 + k.cx * r2);
    M[4 + c] = (float)(k.fy * r1 + k.cy * r2);
    M[8 + c] = (float)r2;
  }
}

// squared reprojection error in pixels of the record q = (X', u), v; +inf behind the camera, and for a NaN record
__device__ __forceinline__ float ap_point_error(const float* M, float4 q, float v) {
  const float hx = __builtin_fmaf(M[0], q.x, __builtin_fmaf(M[1], q.y, __builtin_fmaf(M[2], q.z, M[3])));
  const float hy = __builtin_fmaf(M[4], q.x, __builtin_fmaf(M[5], q.y, __builtin_fmaf(M[6], q.z, M[7])));
  const float hw = __builtin_fmaf(M[8], q.x, __builtin_fmaf(M[9], q.y, __builtin_fmaf(M[10], q.z, M[11])));
  const float iw = 1.0f / hw;
  const float dx = __builtin_fmaf(-hx, iw, q.w), dy = __builtin_fmaf(-hy, iw, v);
  return hw > 0.f ? __builtin_fmaf(dx, dx, dy * dy) : INFINITY;
}

// slab_cost / slab_cnt: (P, S, M) with M = iters * 4 slots and S = ceil(N / CHUNK) chunks, as score_kernel of ransac_common.h
template <int SCORE>
__global__ __launch_bounds__(256) void ap_score_kernel(const float4* __restrict__ pts, const float* __restrict__ pv,
                                                       const double* __restrict__ K, const double* __restrict__ models,
                                                       const double* __restrict__ tvec, const int* __restrict__ valid, int N, int M,
                                                       float t2, float* __restrict__ slab_cost, int* __restrict__ slab_cnt) {
  __shared__ float4 sp[CHUNK];
  __shared__ float sv[CHUNK];
  __shared__ float sl[SCORE == SCORE_MAGSAC ? MAGSAC_CELLS : 1];
  const int p = blockIdx.z, s = blockIdx.y, S = gridDim.y;
  const int i0 = s * CHUNK, n = min(CHUNK, N - i0);
  const size_t src = (size_t)p * N + i0;
  for (int i = threadIdx.x; i < n; i += 256) { sp[i] = pts[src + i]; sv[i] = pv[src + i]; }
  if constexpr (SCORE == SCORE_MAGSAC)
    for (int i = threadIdx.x; i < MAGSAC_CELLS; i += 256) sl[i] = magsac_loss_cells.c[i].v;
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  float cost = 0.f;
  int cnt = 0;
  if (valid[slot]) {
    float md[12];
    {
      double R[9], t[3];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = models[slot * 9 + i];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = tvec[slot * 3 + i];
      compose_projection(R, t, load_cam(K + p * 9), md);
    }
    if constexpr (SCORE == SCORE_MSAC) {
      for (int j = 0; j < n; ++j) {
        const float e = ap_point_error(md, sp[j], sv[j]);
        const bool in = e < t2;
        cnt += in ? 1 : 0;
        cost += in ? e : t2;
      }
    } else {
      const float scale = (float)MAGSAC_CELLS / t2;
      for (int j = 0; j < n; ++j) {
        const float e = ap_point_error(md, sp[j], sv[j]);
        if (e < t2) {
          float frac;
          const int i = magsac_cell(e, scale, frac);
          const float lo = sl[i], hi = sl[min(i + 1, MAGSAC_CELLS - 1)];
          cost += __builtin_fmaf(frac, (i < MAGSAC_CELLS - 1 ? hi : 1.f) - lo, lo);
          ++cnt;
        }
      }
      cost = t2 * ((float)(n - cnt) + cost);
    }
  }
  const size_t o = ((size_t)p * S + s) * M + m;
  slab_cost[o] = cost;
  slab_cnt[o] = cnt;
}

// Cost and inlier count of (R, t') over the pair's N records: block_cost of ransac_common.h
template <int SCORE>
__device__ void ap_block_score(const double* R, const double* t, const Cam& cam, const float4* pq, const float* pvq, int N, float t2,
                               double* dred, int* ired, double& cost, int& cnt) {
  float m[12];
  compose_projection(R, t, cam, m);
  block_cost<SCORE>(N, t2, [&](int i) { return ap_point_error(m, pq[i], pvq[i]); }, dred, ired, cost, cnt);
}

// ------------------------------------------------------------------------------------------ selection + local optimisation
template <int SCORE>
__global__ __launch_bounds__(AP_THREADS) void ap_select_kernel(const double* __restrict__ Xw, const double2* __restrict__ xp,
                                                               const double* __restrict__ K, const double* __restrict__ norm,
                                                               const float4* __restrict__ pts, const float* __restrict__ pv,
                                                               const double* __restrict__ models, const double* __restrict__ tvec,
                                                               const double* __restrict__ cost, int N, int M, float t2, int lo_iters,
                                                               double* __restrict__ R_out, double* __restrict__ t_out,
                                                               unsigned char* __restrict__ mask) {
  __shared__ double dred[256];
  __shared__ int ired[256];
  __shared__ double red[AP_WAVES][AP_NSUM], in[25];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  const float4* pq = pts + base;
  const float* pvq = pv + base;

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
    if (tid < 9) R_out[p * 9 + tid] = 0.0;
    if (tid < 3) t_out[p * 3 + tid] = 0.0;
    for (int i = tid; i < N; i += 256) mask[base + i] = 0;
    return;
  }
  // the pair's constants through LDS, so that every thread holds them in vector registers (pose_refine.hip)
  if (tid < 9) { in[tid] = K[p * 9 + tid]; in[9 + tid] = models[((size_t)p * M + bm) * 9 + tid]; }
  if (tid < 3) in[18 + tid] = tvec[((size_t)p * M + bm) * 3 + tid];
  if (tid < 4) in[21 + tid] = norm[p * 8 + tid];
  __syncthreads();
  const Cam cam = load_cam(in);
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = in[9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = in[18 + i];
  const double c[3] = {in[21], in[22], in[23]}, sc = in[24];
  double cc;
  int cn;
  ap_block_score<SCORE>(R, t, cam, pq, pvq, N, t2, dred, ired, cc, cn);

  // 2. local optimisation: one LM step of the refinement on the inliers, kept only if the re-scored cost is lower
  for (int round = 0; round < lo_iters; ++round) {
    if (cn < AP_MIN_MATCHES) break;
    double s[AP_NSUM], delta[AP_NPAR], Rc[9], tc[3];
    ap_evaluate<SCORE>(R, t, cam, true, Xw, xp, nullptr, base, N, c, sc, (double)t2, red, s);
    if (!solve_step<AP_NPAR>(s, s + AP_NTRI, AP_LAMBDA0, delta)) break;
    ap_apply_step(R, t, delta, Rc, tc);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(Rc[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fin = fin && isfinite(tc[i]);
    if (!fin) break;
    double c2;
    int n2;
    ap_block_score<SCORE>(Rc, tc, cam, pq, pvq, N, t2, dred, ired, c2, n2);
    if (!(c2 < cc)) break;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tc[i];
    cc = c2;
    cn = n2;
  }

  // 3. back to the world frame: t = t' / s - R c; mask under the pose that is returned
  if (tid < 9) R_out[p * 9 + tid] = R[tid];
  if (tid < 3) t_out[p * 3 + tid] = t[tid] / sc - (R[3 * tid] * c[0] + R[3 * tid + 1] * c[1] + R[3 * tid + 2] * c[2]);
  float m[12];
  compose_projection(R, t, cam, m);
  for (int i = tid; i < N; i += 256) mask[base + i] = ap_point_error(m, pq[i], pvq[i]) < t2 ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------------- refinement
__global__ __launch_bounds__(AP_THREADS) void refine_absolute_pose_kernel(const double* __restrict__ Xw, const double2* __restrict__ xp,
                                                                          const double* __restrict__ K, const double* __restrict__ R_in,
                                                                          const double* __restrict__ t_in, const unsigned char* mask_in,
                                                                          int N, double t2, int iters, double* __restrict__ R_out,
                                                                          double* __restrict__ t_out, unsigned char* __restrict__ mask_out,
                                                                          double* __restrict__ cost_out, int* __restrict__ count_out,
                                                                          int* __restrict__ steps_out) {
  __shared__ double red[AP_WAVES][AP_NSUM], in[21];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  if (tid < 9) { in[tid] = K[p * 9 + tid]; in[9 + tid] = R_in[p * 9 + tid]; }
  if (tid < 3) in[18 + tid] = t_in[p * 3 + tid];
  __syncthreads();
  double ki[5];
  const bool kok = invert_k(in, ki);
  const Cam cam = load_cam(in);
  double R[9], t[3];
  bool good = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = in[9 + i]; good = good && isfinite(R[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { t[i] = in[18 + i]; good = good && isfinite(t[i]); }

  // the normalisation of ap_prepare_kernel over the usable matches: centroid, then the mean distance
  auto usable = [&](int i) {
    const double* xw = Xw + (base + i) * 3;
    const double2 px = xp[base + i];
    return kok && isfinite(xw[0]) && isfinite(xw[1]) && isfinite(xw[2]) && isfinite(px.x) && isfinite(px.y) &&
           (!mask_in || mask_in[base + i] != 0);
  };
  double c[3], sc;
  {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += AP_THREADS)
      if (usable(i)) {
        const double* xw = Xw + (base + i) * 3;
        a[0] += xw[0]; a[1] += xw[1]; a[2] += xw[2]; a[3] += 1.0;
      }
    block_sum<4, AP_WAVES>(a, red);
    const double inv = a[3] > 0.0 ? 1.0 / a[3] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = a[i] * inv;
    double d[1] = {0.0};
    for (int i = tid; i < N; i += AP_THREADS)
      if (usable(i)) {
        const double* xw = Xw + (base + i) * 3;
        const double d0 = xw[0] - c[0], d1 = xw[1] - c[1], d2 = xw[2] - c[2];
        d[0] += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      }
    block_sum<1, AP_WAVES>(d, red);
    const double md = d[0] * inv;
    sc = 1.7320508075688772 / md;
    if (!(md > 0.0) || !isfinite(sc)) sc = 1.0;
  }
  double tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) tn[i] = sc * (R[3 * i] * c[0] + R[3 * i + 1] * c[1] + R[3 * i + 2] * c[2] + t[i]);

  // pass 0 evaluates the input pose, pass it > 0 the candidate of step it; (Rk, tk, s) is the last accepted pose with its sums
  double Rk[9], tk[3], s[AP_NSUM];
  double lambda = AP_LAMBDA0, cost0 = 0.0, count0 = 0.0;
  int steps = 0;
  bool failed = false;
  for (int it = 0; it <= iters; ++it) {
    double Rc[9], tc[3], sn[AP_NSUM];
    if (it == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rc[i] = R[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) tc[i] = tn[i];
    } else {
      double delta[AP_NPAR];
      if (!solve_step<AP_NPAR>(s, s + AP_NTRI, lambda, delta)) { failed = true; break; }
      ap_apply_step(Rk, tk, delta, Rc, tc);
      bool moved = false;
#pragma unroll
      for (int i = 0; i < 9; ++i) moved = moved || Rc[i] != Rk[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) moved = moved || tc[i] != tk[i];
      if (!moved) break;
    }
    ap_evaluate<SCORE_MSAC>(Rc, tc, cam, kok, Xw, xp, mask_in, base, N, c, sc, t2, red, sn);
    const bool first = it == 0;
    if (first) { cost0 = sn[AP_COST]; count0 = sn[AP_COUNT]; }
    if (first || sn[AP_COST] < s[AP_COST] * (1.0 - AP_ACCEPT_REL)) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rk[i] = Rc[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) tk[i] = tc[i];
#pragma unroll
      for (int k = 0; k < AP_NSUM; ++k) s[k] = sn[k];
      if (!first) {
        lambda = fmax(lambda / 10.0, AP_LAMBDA_MIN);
        ++steps;
      }
    } else {
      lambda *= 10.0;
    }
    if (first && !(good && count0 >= (double)AP_MIN_MATCHES)) break;
  }
  if (failed) {
    steps = 0;
    s[AP_COST] = cost0;
    s[AP_COUNT] = count0;
  }
  const bool kept = steps > 0;                                  // else the input pose, as it came
  if (!kept) {
#pragma unroll
    for (int i = 0; i < 9; ++i) Rk[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tk[i] = tn[i];
  }
  if (tid < 9) R_out[p * 9 + tid] = Rk[tid];
  if (tid < 3)
    t_out[p * 3 + tid] = kept ? tk[tid] / sc - (Rk[3 * tid] * c[0] + Rk[3 * tid + 1] * c[1] + Rk[3 * tid + 2] * c[2]) : t[tid];
  if (tid == 0) {
    cost_out[p] = s[AP_COST];
    count_out[p] = (int)s[AP_COUNT];
    steps_out[p] = steps;
  }
  for (int i = tid; i < N; i += AP_THREADS) {
    const double* xw = Xw + (base + i) * 3;
    const double2 px = xp[base + i];
    const double X[3] = {(xw[0] - c[0]) * sc, (xw[1] - c[1]) * sc, (xw[2] - c[2]) * sc};
    ApPoint q;
    ap_point(Rk, tk, cam, X, px.x, px.y, q);
    mask_out[base + i] = (usable(i) && q.z > 0.0 && q.e < t2) ? 1 : 0;
  }
}

// --------------------------------------------------------------------------------------------------------------- workspace
// ransac_common.h's regions with S = 3 and R = 4 ([3] holds R), then t', the v of the scoring records and the fp64 copy
constexpr int WA_TVEC = WS_N, WA_PV = WS_N + 1, WA_XN = WS_N + 2, WA_N = WS_N + 3;

long layout_ap(int P, int N, int iters, long* off) {
  const long extra[3] = {(long)P * iters * AP_R * 24, (long)P * N * 4, (long)P * N * 40};
  return ws_layout(AP_S, AP_R, P, N, iters, extra, 3, off);
}

int check_args_ap(const char* fn, const void* X, const void* x, const void* K, const void* ws, int P, int N, int iters, float threshold,
                  long ws_bytes) {
  ROMA_REQUIRE(X && x && K && ws, ROMA_E_ARG, "%s: null pointer", fn);
  const int rc = check_problem(fn, P, N, iters, AP_S, P3P_THREADS, threshold);
  return rc ? rc : check_workspace(fn, ws_bytes, layout_ap(P, N, iters, nullptr));
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_absolute_pose_workspace(int P, int N, int iters, long* offsets) {
  if (P < 1 || N < 1 || iters < 1) {
    set_error("roma_absolute_pose_workspace: bad arguments P=%d N=%d iters=%d", P, N, iters);
    return ROMA_E_ARG;
  }
  return layout_ap(P, N, iters, offsets);
}

extern "C" int roma_absolute_pose_hypotheses(const double* X, const double* x, const double* K, int P, int N, int iters, float threshold,
                                             int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  const char* fn = __func__;
  int rc = check_args_ap(fn, X, x, K, ws, P, N, iters, threshold, ws_bytes);
  if (rc) return rc;
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_pair_offset(fn, p0);
  if (rc) return rc;
  long off[WA_N];
  layout_ap(P, N, iters, off);
  const Regions r = regions(ws, off);
  double* tvec = region<double>(ws, off, WA_TVEC);
  float* pv = region<float>(ws, off, WA_PV);
  double* xn = region<double>(ws, off, WA_XN);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int M = iters * AP_R, C = (N + CHUNK - 1) / CHUNK;
  const uint32_t sstream = sample_stream(seed, STAGE_AP);
  const float t2 = threshold * threshold;
  const Grids g = ransac_grids(P, N, iters, AP_R, P3P_THREADS);
  hipLaunchKernelGGL(ap_prepare_kernel, dim3(P), dim3(256), 0, st, X, x, K, N, r.norm, r.pts, pv, xn);
  hipLaunchKernelGGL(p3p_kernel, g.solve, dim3(P3P_THREADS), 0, st, xn, r.pts, P, N, iters, sstream, p0, r.samples, r.models, tvec, r.valid);
  const auto score = by_scoring(scoring, ap_score_kernel<SCORE_MSAC>, ap_score_kernel<SCORE_MAGSAC>);
  hipLaunchKernelGGL(score, g.score, dim3(256), 0, st, r.pts, pv, K, r.models, tvec, r.valid, N, M, t2, r.slab_cost, r.slab_cnt);
  hipLaunchKernelGGL(reduce_kernel, g.reduce, dim3(256), 0, st, r.slab_cost, r.slab_cnt, r.valid, P, M, C, r.cost, r.count);
  return check_launch(fn);
}

extern "C" int roma_absolute_pose_select(const double* X, const double* x, const double* K, int P, int N, int iters, float threshold,
                                         int scoring, int lo_iters, const void* ws, long ws_bytes, double* R, double* t,
                                         unsigned char* mask, void* stream) {
  const char* fn = __func__;
  int rc = check_args_ap(fn, X, x, K, ws, P, N, iters, threshold, ws_bytes);
  if (rc) return rc;
  ROMA_REQUIRE(R && t && mask, ROMA_E_ARG, "%s: null pointer", fn);
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_lo_iters(fn, lo_iters);
  if (rc) return rc;
  ROMA_REQUIRE(aligned16(x), ROMA_E_ALIGN, "%s: x must be 16-byte aligned", fn);
  long off[WA_N];
  layout_ap(P, N, iters, off);
  const Regions r = regions(ws, off);
  const auto sel = by_scoring(scoring, ap_select_kernel<SCORE_MSAC>, ap_select_kernel<SCORE_MAGSAC>);
  hipLaunchKernelGGL(sel, dim3(P), dim3(AP_THREADS), 0, static_cast<hipStream_t>(stream), X, (const double2*)x, K, r.norm, r.pts,
                     region<float>(ws, off, WA_PV), r.models, region<double>(ws, off, WA_TVEC), r.cost, N, iters * AP_R,
                     threshold * threshold, lo_iters, R, t, mask);
  return check_launch(fn);
}

extern "C" int roma_refine_absolute_pose(const double* X, const double* x, const double* K, const double* R_in, const double* t_in,
                                         const unsigned char* mask_in, int P, int N, double threshold, int iters, double* R, double* t,
                                         unsigned char* mask, double* cost, int* count, int* steps, void* stream) {
  ROMA_REQUIRE(X && x && K && R_in && t_in && R && t && mask && cost && count && steps, ROMA_E_ARG,
               "roma_refine_absolute_pose: null pointer");
  const int rc = check_refine(__func__, x, x, P, N, AP_MIN_MATCHES, threshold, iters);
  if (rc) return rc;
  hipLaunchKernelGGL(refine_absolute_pose_kernel, dim3(P), dim3(AP_THREADS), 0, static_cast<hipStream_t>(stream), X, (const double2*)x,
                     K, R_in, t_in, mask_in, N, threshold * threshold, iters, R, t, mask, cost, count, steps);
  ROMA_CHECK_LAUNCH();
}
