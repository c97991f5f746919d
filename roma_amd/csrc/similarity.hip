// 3-D similarity registration: RANSAC on putative 3D-3D correspondences (3-point minimal sample) and iterated re-weighted refinement —
// what puts two reconstructions, each known up to the scale of its own baseline, into one frame, or a reconstruction onto a
// ground-truth cloud.  Model (s, R, t): Y ~ s R X + t with s > 0, R orthonormal with det +1; with_scale = 0 is the rigid model (s = 1).
// Ground rules of geometry.hip: fp64 minimal solver, fp32 scoring of every slot (MSAC or MAGSAC++), fixed number of samples, no
// atomics, no allocation, no host synchronisation, sums in a fixed order: bitwise reproducible, and a pair's result does not depend on
// the rest of the batch.  DESIGN.md §3.4; tests/similarity_ref.py restates it in numpy.
//
// Pipeline, one call of roma_similarity_hypotheses + one of roma_similarity_select (P pairs of N correspondences, iters samples each):
//   sim_prepare_kernel  one block/pair   centroid and scale (mean distance sqrt 3) of X over the usable rows (all six numbers finite),
//                                        and of Y (fp64, fixed-order LDS tree); X' = sX (X - cX), Y' = sY (Y - cY); with_scale = 0: one
//                                        scale, Y's, for both clouds.  Scoring record (X', Y'_x) fp32 + (Y'_y, Y'_z) fp32, and the fp64
//                                        copy (X', Y') the solver and the select kernel read; NaN rows where a row is not usable
//   sim_solve_kernel    one lane/sample  draws 3 distinct usable rows (geometry.hip's scheme, stage 6), forms the 18 sums with unit
//                                        weights and calls the closed form -> one slot (s', R, t'), zero and invalid when rejected
//   sim_score_kernel    the score_kernel pattern of ransac_common.h: 1024-point chunks in LDS (24 KB), one slot per thread, broadcast
//                       reads, partial cost and count into the slab; M = s' R composed once per slot in fp32, a point costs three dot
//                       products and the squared distance |y' - (M x' + t')|^2
//   reduce_kernel       (ransac_common.h)
//   sim_select_kernel   one block/pair   lowest cost (lowest slot on ties), lo_iters rounds of the closed form on the inliers (weight W
//                                        for MAGSAC++, 1 for MSAC), each kept only if the fp32 re-score drops
// and, on its own, refine_similarity_kernel (one workgroup of 256 per pair): the same closed form iterated on the inliers of the
// truncated cost in fp64.
// Internally the model is (s' = s sY / sX, R, t' = sY (s R cX + t - cY)) on the normalised clouds; the entry points return
// (s = s' sX / sY, R, t = t' / sY + cY - s R cX).  The threshold is a distance in Y units (thr' = sY thr).  The normalisation is what
// lets fp32 score a world that sits 1e4 units from its origin, and scale ratios of 0.05 or 20.
//
// The closed form (sim_closed_form) maps 18 weighted sums — W = sum w, sum w x (3), sum w y (3), sum w y x^T (9), sum w |x|^2,
// sum w |y|^2 — to the least-squares (s, R, t) of Umeyama:
//   means mx, my; C = sum w (y - my)(x - mx)^T = sum w y x^T - (sum w y) mx^T; vx = sum w |x - mx|^2, vy likewise
//   R by Horn's quaternion: the symmetric 4 x 4 matrix N of C, SIM_SWEEPS sweeps of cyclic Jacobi in registers (the rotation of
//   twoview_math.h's jacobi_lds), the eigenvector of the largest diagonal entry (lowest index on ties), normalised -> a proper rotation,
//   no reflection case
//   rejected when lambda_1 - lambda_2 <= gap_tol sqrt(vx vy): the rotation about the clouds' common axis is not fixed.  lambda_1 -
//   lambda_2 over sqrt(vx vy) is about the squared ratio of the clouds' second extent to their first; the weighted calls pass
//   SIM_GAP_TOL = 1e-10 (a cloud 1e-5 as thick as it is long), the minimal solver passes 0 behind its own test
//   s = sum_ij R_ij C_ij / vx (1 for with_scale = 0, R as it is), rejected when not finite and positive; t = my - s R mx
// The minimal sample is rejected by P3P's collinearity test in both clouds: |(p2 - p1) x (p3 - p1)| <= 1e-6 |p2 - p1| |p3 - p1|.
//
// Refinement: cost = sum over the usable matches (finite, allowed by mask_in) of min(e, thr^2), e the squared distance in Y units.
// A round is the closed form on the matches with e < thr^2 under the current model; it is kept when cost' < cost (1 - 1e-12), the first
// round that is not kept ends the loop, as do `iters` rounds.  Fewer than 3 weighted matches, a rejected closed form, an input model
// that is not finite or no round kept: the input comes back bit for bit with steps = 0 and its own mask, cost and count.
#include "ransac_common.h"

namespace roma {
namespace {

constexpr int SIM_S = 3, SIM_R = 1;
constexpr int SIM_SOLVE_THREADS = 128;
constexpr int SIM_THREADS = 256, SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_NSUM = 20;                                    // the 18 sums + cost + count
constexpr int SIM_COST = 18, SIM_COUNT = 19;
constexpr int SIM_MIN_MATCHES = 3;
constexpr int SIM_SWEEPS = 8;
constexpr double SIM_GAP_TOL = 1e-10, SIM_ACCEPT_REL = 1e-12;
constexpr double SQRT3 = 1.7320508075688772;

struct Sim {
  double s, R[9], t[3];
};

__device__ __forceinline__ bool sim_finite(const Sim& m) {
  bool f = isfinite(m.s);
#pragma unroll
  for (int i = 0; i < 9; ++i) f = f && isfinite(m.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) f = f && isfinite(m.t[i]);
  return f;
}

// ------------------------------------------------------------------------------------------------------- closed form (fp64)
// S[0..17] += w (1, x, y, y x^T row by row, |x|^2, |y|^2)
__device__ __forceinline__ void sim_accumulate(const double* x, const double* y, double w, double* S) {
  S[0] += w;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double wx = w * x[i], wy = w * y[i];
    S[1 + i] += wx;
    S[4 + i] += wy;
#pragma unroll
    for (int j = 0; j < 3; ++j) S[7 + 3 * i + j] += wy * x[j];
    S[16] += wx * x[i];
    S[17] += wy * y[i];
  }
}

// Cyclic Jacobi on the symmetric 4 x 4 matrix A in registers, eigenvectors into the columns of V
__device__ __forceinline__ void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sw = 0; sw < SIM_SWEEPS; ++sw) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
        if (apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          A[p][p] = app - t * apq;
          A[q][q] = aqq + t * apq;
          A[p][q] = 0.0;
          A[q][p] = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k != p && k != q) {
              const double akp = A[k][p], akq = A[k][q];
              const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
              A[k][p] = nkp; A[p][k] = nkp;
              A[k][q] = nkq; A[q][k] = nkq;
            }
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq;
            V[k][q] = s * vkp + c * vkq;
          }
        }
      }
    }
  }
}

// (s, R, t) of the 18 sums S; false when rejected (the header has the rules).  m is written either way.
__device__ __forceinline__ bool sim_closed_form(const double* S, bool with_scale, double gap_tol, Sim& m) {
  const double W = S[0], iw = 1.0 / W;
  double mx[3], my[3], C[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) { mx[i] = S[1 + i] * iw; my[i] = S[4 + i] * iw; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = S[7 + 3 * i + j] - S[4 + i] * mx[j];
  const double vx = S[16] - (S[1] * mx[0] + S[2] * mx[1] + S[3] * mx[2]);
  const double vy = S[17] - (S[4] * my[0] + S[5] * my[1] + S[6] * my[2]);
  // Horn: S_ab = sum x_a y_b = C[b][a]
  const double Sxx = C[0], Sxy = C[3], Sxz = C[6], Syx = C[1], Syy = C[4], Syz = C[7], Szx = C[2], Szy = C[5], Szz = C[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy}};
  double V[4][4];
  jacobi4(A, V);
  int k = 0;
  double l1 = A[0][0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const bool gt = A[i][i] > l1;
    k = gt ? i : k;
    l1 = gt ? A[i][i] : l1;
  }
  double l2 = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) l2 = (i != k && A[i][i] > l2) ? A[i][i] : l2;
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = k == 0 ? V[i][0] : (k == 1 ? V[i][1] : (k == 2 ? V[i][2] : V[i][3]));
  const double iq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double q0 = q[0] * iq, qx = q[1] * iq, qy = q[2] * iq, qz = q[3] * iq;
  m.R[0] = q0 * q0 + qx * qx - qy * qy - qz * qz;
  m.R[1] = 2.0 * (qx * qy - q0 * qz);
  m.R[2] = 2.0 * (qx * qz + q0 * qy);
  m.R[3] = 2.0 * (qy * qx + q0 * qz);
  m.R[4] = q0 * q0 - qx * qx + qy * qy - qz * qz;
  m.R[5] = 2.0 * (qy * qz - q0 * qx);
  m.R[6] = 2.0 * (qz * qx - q0 * qy);
  m.R[7] = 2.0 * (qz * qy + q0 * qx);
  m.R[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) tr += m.R[i] * C[i];
  m.s = with_scale ? tr / vx : 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) m.t[i] = my[i] - m.s * (m.R[3 * i] * mx[0] + m.R[3 * i + 1] * mx[1] + m.R[3 * i + 2] * mx[2]);
  return W > 0.0 && vx > 0.0 && vy > 0.0 && (l1 - l2) > gap_tol * sqrt(vx * vy) && m.s > 0.0 && sim_finite(m);
}

// squared distance |y - (s R x + t)|^2 in fp64; NaN for a row that is not finite
__device__ __forceinline__ double sim_error(const Sim& m, const double* x, const double* y) {
  double e = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double d = y[r] - (m.s * (m.R[3 * r] * x[0] + m.R[3 * r + 1] * x[1] + m.R[3 * r + 2] * x[2]) + m.t[r]);
    e += d * d;
  }
  return e;
}

// The 20 sums of one model over the pair's matches, reduced: on return every thread holds the same s[].  load(i, x, y) gives match i in
// the coordinates of the model and says whether it may carry weight.  WEIGHT = SCORE_MAGSAC: an inlier is weighted by W(e / thr^2) of
// magsac_table.h, else by 1.
template <int WEIGHT, class Load>
__device__ __forceinline__ void sim_evaluate(const Sim& m, Load load, int N, double t2, double (*red)[SIM_NSUM], double (&s)[SIM_NSUM]) {
#pragma unroll
  for (int k = 0; k < SIM_NSUM; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < N; i += SIM_THREADS) {
    double x[3], y[3];
    const bool ok = load(i, x, y);
    const double e = sim_error(m, x, y);
    const bool in = ok && e < t2;
    double wgt = in ? 1.0 : 0.0;
    if constexpr (WEIGHT == SCORE_MAGSAC) {
      if (in) wgt = (double)magsac_lookup(magsac_weight_cells, (float)e, (float)MAGSAC_CELLS / (float)t2);
    }
    s[SIM_COST] += ok ? (in ? e : t2) : 0.0;
    s[SIM_COUNT] += in ? 1.0 : 0.0;
    if (!in) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { x[k] = 0.0; y[k] = 0.0; }
    }
    sim_accumulate(x, y, wgt, s);
  }
  block_sum<SIM_NSUM, SIM_WAVES>(s, red);
}

__device__ __forceinline__ bool finite6(const double* x, const double* y) {
  return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
}

// scale of a cloud from its mean distance md to the centroid; 1 for identical points (or none): every sample is degenerate then
__device__ __forceinline__ double cloud_scale(double md) {
  const double s = SQRT3 / md;
  return (md > 0.0 && isfinite(s)) ? s : 1.0;
}

// ------------------------------------------------------------------------------------------------------------------ prepare
// norm[p*8 + 0..7] = (cX, sX, cY, sY); pts: (P,N) float4 (X', Y'_x); py: (P,N) float2 (Y'_y, Y'_z); xn: (P,N,6) fp64 (X', Y')
__global__ __launch_bounds__(256) void sim_prepare_kernel(const double* __restrict__ Xw, const double* __restrict__ Yw, int N,
                                                          int with_scale, double* __restrict__ norm, float4* __restrict__ pts,
                                                          float2* __restrict__ py, double* __restrict__ xn) {
  __shared__ double red[6][256];
  __shared__ int ired[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* X = Xw + (size_t)p * N * 3;
  const double* Y = Yw + (size_t)p * N * 3;
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int n = 0;
  for (int i = tid; i < N; i += 256)
    if (finite6(X + 3 * (size_t)i, Y + 3 * (size_t)i)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { a[k] += X[3 * (size_t)i + k]; a[3 + k] += Y[3 * (size_t)i + k]; }
      ++n;
    }
#pragma unroll
  for (int k = 0; k < 6; ++k) red[k][tid] = a[k];
  ired[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 6; ++k) red[k][tid] += red[k][tid + o];
      ired[tid] += ired[tid + o];
    }
    __syncthreads();
  }
  const int cnt = ired[0];
  double c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = cnt > 0 ? red[k][0] / cnt : 0.0;
  __syncthreads();
  double dx = 0.0, dy = 0.0;
  for (int i = tid; i < N; i += 256)
    if (finite6(X + 3 * (size_t)i, Y + 3 * (size_t)i)) {
      const double x0 = X[3 * (size_t)i] - c[0], x1 = X[3 * (size_t)i + 1] - c[1], x2 = X[3 * (size_t)i + 2] - c[2];
      const double y0 = Y[3 * (size_t)i] - c[3], y1 = Y[3 * (size_t)i + 1] - c[4], y2 = Y[3 * (size_t)i + 2] - c[5];
      dx += sqrt(x0 * x0 + x1 * x1 + x2 * x2);
      dy += sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    }
  red[0][tid] = dx;
  red[1][tid] = dy;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  const double sY = cloud_scale(cnt > 0 ? red[1][0] / cnt : 0.0);
  const double sX = with_scale ? cloud_scale(cnt > 0 ? red[0][0] / cnt : 0.0) : sY;
  if (tid < 8) norm[p * 8 + tid] = tid < 3 ? c[tid] : (tid == 3 ? sX : (tid < 7 ? c[tid - 1] : sY));
  const double nan = __builtin_nan("");
  const float nanf = __builtin_nanf("");
  for (int i = tid; i < N; i += 256) {
    const size_t q = (size_t)p * N + i;
    double o[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = (X[3 * (size_t)i + k] - c[k]) * sX; o[3 + k] = (Y[3 * (size_t)i + k] - c[3 + k]) * sY; }
    const bool ok = finite6(X + 3 * (size_t)i, Y + 3 * (size_t)i) && finite6(o, o + 3);
#pragma unroll
    for (int k = 0; k < 6; ++k) xn[q * 6 + k] = ok ? o[k] : nan;
    pts[q] = ok ? make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]) : make_float4(nanf, nanf, nanf, nanf);
    py[q] = ok ? make_float2((float)o[4], (float)o[5]) : make_float2(nanf, nanf);
  }
}

// ------------------------------------------------------------------------------------------------------------------- solver
// samples: (P, iters, 3) int32; models: (P, iters, 9) fp64 R; ts: (P, iters, 4) fp64 (t', s'); valid: (P, iters)
__global__ __launch_bounds__(SIM_SOLVE_THREADS) void sim_solve_kernel(const double* __restrict__ xn, const float4* __restrict__ pts, int P,
                                                                      int N, int iters, uint32_t stream, int p0, int with_scale,
                                                                      int* __restrict__ samples, double* __restrict__ models,
                                                                      double* __restrict__ ts, int* __restrict__ valid) {
  const long t = (long)blockIdx.x * SIM_SOLVE_THREADS + threadIdx.x;
  if (t >= (long)P * iters) return;
  const int p = (int)(t / iters), h = (int)(t % iters);
  const size_t base = (size_t)p * N;

  int idx[SIM_S];
  bool ok;
  draw_sample<SIM_S>(stream, (uint32_t)(p0 + p), iters, h, N, [&](int i) { const float v = pts[base + i].x; return v == v; }, idx, ok);
#pragma unroll
  for (int k = 0; k < SIM_S; ++k) samples[(size_t)t * SIM_S + k] = ok ? idx[k] : -1;

  double xs[3][3], ys[3][3], S[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) S[k] = 0.0;
#pragma unroll
  for (int k = 0; k < SIM_S; ++k) {
    const double* q = xn + (base + (ok ? idx[k] : 0)) * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) { xs[k][i] = q[i]; ys[k][i] = q[3 + i]; }
    sim_accumulate(xs[k], ys[k], 1.0, S);
  }
  bool good = ok;
#pragma unroll
  for (int cloud = 0; cloud < 2; ++cloud) {
    const double(*pt)[3] = cloud == 0 ? xs : ys;
    double e1[3], e2[3], cr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { e1[i] = pt[1][i] - pt[0][i]; e2[i] = pt[2][i] - pt[0][i]; }
    cross3(e1, e2, cr);
    const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), n2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    good = good && sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) > COLLINEAR_TOL * n1 * n2;
  }
  Sim m;
  good = sim_closed_form(S, with_scale != 0, 0.0, m) && good;
#pragma unroll
  for (int i = 0; i < 9; ++i) models[(size_t)t * 9 + i] = good ? m.R[i] : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) ts[(size_t)t * 4 + i] = good ? m.t[i] : 0.0;
  ts[(size_t)t * 4 + 3] = good ? m.s : 0.0;
  valid[t] = good ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ scoring (fp32)
// the squared threshold of a pair in normalised Y units, from threshold^2 in Y units (fp32, as the host squares it)
__device__ __forceinline__ float normalised_t2(float thr2, double sY) { return (float)((double)thr2 * sY * sY); }

// M = s' R (row major 3 x 3) and t' in fp32
__device__ __forceinline__ void compose_similarity(const Sim& m, float* M) {
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = (float)(m.s * m.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) M[9 + i] = (float)m.t[i];
}

// squared distance of the record q = (X', Y'_x), r = (Y'_y, Y'_z) in normalised Y units; NaN for a NaN record
__device__ __forceinline__ float sim_point_error(const float* M, float4 q, float2 r) {
  const float d0 = q.w - __builtin_fmaf(M[0], q.x, __builtin_fmaf(M[1], q.y, __builtin_fmaf(M[2], q.z, M[9])));
  const float d1 = r.x - __builtin_fmaf(M[3], q.x, __builtin_fmaf(M[4], q.y, __builtin_fmaf(M[5], q.z, M[10])));
  const float d2 = r.y - __builtin_fmaf(M[6], q.x, __builtin_fmaf(M[7], q.y, __builtin_fmaf(M[8], q.z, M[11])));
  return __builtin_fmaf(d0, d0, __builtin_fmaf(d1, d1, d2 * d2));
}

__device__ __forceinline__ Sim load_slot(const double* __restrict__ models, const double* __restrict__ ts, size_t slot) {
  Sim m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.R[i] = models[slot * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) m.t[i] = ts[slot * 4 + i];
  m.s = ts[slot * 4 + 3];
  return m;
}

// slab_cost / slab_cnt: (P, S, M) with M = iters slots and S = ceil(N / CHUNK) chunks, as score_kernel of ransac_common.h
template <int SCORE>
__global__ __launch_bounds__(256) void sim_score_kernel(const float4* __restrict__ pts, const float2* __restrict__ py,
                                                        const double* __restrict__ models, const double* __restrict__ ts,
                                                        const int* __restrict__ valid, const double* __restrict__ norm, int N,
                                                        int M, float thr2, float* __restrict__ slab_cost,
                                                        int* __restrict__ slab_cnt) {
  __shared__ float4 sp[CHUNK];
  __shared__ float2 sy[CHUNK];
  __shared__ float sl[SCORE == SCORE_MAGSAC ? MAGSAC_CELLS : 1];
  const int p = blockIdx.z, s = blockIdx.y, S = gridDim.y;
  const int i0 = s * CHUNK, n = min(CHUNK, N - i0);
  const size_t src = (size_t)p * N + i0;
  const float t2 = normalised_t2(thr2, norm[p * 8 + 7]);
  for (int i = threadIdx.x; i < n; i += 256) { sp[i] = pts[src + i]; sy[i] = py[src + i]; }
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
    compose_similarity(load_slot(models, ts, slot), md);
    if constexpr (SCORE == SCORE_MSAC) {
      for (int j = 0; j < n; ++j) {
        const float e = sim_point_error(md, sp[j], sy[j]);
        const bool in = e < t2;
        cnt += in ? 1 : 0;
        cost += in ? e : t2;
      }
    } else {
      const float scale = (float)MAGSAC_CELLS / t2;
      for (int j = 0; j < n; ++j) {
        const float e = sim_point_error(md, sp[j], sy[j]);
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

// Cost and inlier count of the model over the pair's N records: block_cost of ransac_common.h
template <int SCORE>
__device__ void sim_block_score(const Sim& mdl, const float4* pq, const float2* pyq, int N, float t2, double* dred, int* ired,
                                double& cost, int& cnt) {
  float m[12];
  compose_similarity(mdl, m);
  block_cost<SCORE>(N, t2, [&](int i) { return sim_point_error(m, pq[i], pyq[i]); }, dred, ired, cost, cnt);
}

// ------------------------------------------------------------------------------------------ selection + local optimisation
template <int SCORE>
__global__ __launch_bounds__(SIM_THREADS) void sim_select_kernel(const double* __restrict__ norm, const float4* __restrict__ pts,
                                                                 const float2* __restrict__ py, const double* __restrict__ xn,
                                                                 const double* __restrict__ models, const double* __restrict__ ts,
                                                                 const double* __restrict__ cost, int N, int M, float thr2, int with_scale,
                                                                 int lo_iters, double* __restrict__ s_out, double* __restrict__ R_out,
                                                                 double* __restrict__ t_out, unsigned char* __restrict__ mask,
                                                                 int* __restrict__ valid_out) {
  __shared__ double dred[256];
  __shared__ int ired[256];
  __shared__ double red[SIM_WAVES][SIM_NSUM], in[21];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  const float4* pq = pts + base;
  const float2* pyq = py + base;

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
    if (tid == 0) { s_out[p] = 0.0; valid_out[p] = 0; }
    for (int i = tid; i < N; i += 256) mask[base + i] = 0;
    return;
  }
  // the pair's constants through LDS, so that every thread holds them in vector registers (pose_refine.hip)
  if (tid < 9) in[tid] = models[((size_t)p * M + bm) * 9 + tid];
  if (tid < 4) in[9 + tid] = ts[((size_t)p * M + bm) * 4 + tid];
  if (tid < 8) in[13 + tid] = norm[p * 8 + tid];
  __syncthreads();
  Sim cur;
#pragma unroll
  for (int i = 0; i < 9; ++i) cur.R[i] = in[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) cur.t[i] = in[9 + i];
  cur.s = in[12];
  const double cX[3] = {in[13], in[14], in[15]}, sX = in[16], cY[3] = {in[17], in[18], in[19]}, sY = in[20];
  const float t2 = normalised_t2(thr2, sY);
  double cc;
  int cn;
  sim_block_score<SCORE>(cur, pq, pyq, N, t2, dred, ired, cc, cn);

  // 2. local optimisation: the closed form on the inliers, kept only if the re-scored cost is lower
  const double* xq = xn + base * 6;
  auto load = [&](int i, double* x, double* y) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = xq[(size_t)i * 6 + k]; y[k] = xq[(size_t)i * 6 + 3 + k]; }
    return true;                                                  // a row that is not usable is NaN: its error is no inlier's
  };
  for (int round = 0; round < lo_iters; ++round) {
    if (cn < SIM_MIN_MATCHES) break;
    double s[SIM_NSUM];
    sim_evaluate<SCORE>(cur, load, N, (double)t2, red, s);
    Sim cand;
    if (!(s[SIM_COUNT] >= (double)SIM_MIN_MATCHES) || !sim_closed_form(s, with_scale != 0, SIM_GAP_TOL, cand)) break;
    double c2;
    int n2;
    sim_block_score<SCORE>(cand, pq, pyq, N, t2, dred, ired, c2, n2);
    if (!(c2 < cc)) break;
    cur = cand;
    cc = c2;
    cn = n2;
  }

  // 3. back to the caller's units: s = s' sX / sY, t = t' / sY + cY - s R cX; mask under the model that is returned
  const double so = cur.s * sX / sY;
  if (tid < 9) R_out[p * 9 + tid] = cur.R[tid];
  if (tid < 3)
    t_out[p * 3 + tid] = cur.t[tid] / sY + cY[tid] - so * (cur.R[3 * tid] * cX[0] + cur.R[3 * tid + 1] * cX[1] + cur.R[3 * tid + 2] * cX[2]);
  if (tid == 0) { s_out[p] = so; valid_out[p] = 1; }
  float m[12];
  compose_similarity(cur, m);
  for (int i = tid; i < N; i += 256) mask[base + i] = sim_point_error(m, pq[i], pyq[i]) < t2 ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------------- refinement
__global__ __launch_bounds__(SIM_THREADS) void refine_similarity_kernel(const double* __restrict__ Xw, const double* __restrict__ Yw,
                                                                        const double* __restrict__ s_in, const double* __restrict__ R_in,
                                                                        const double* __restrict__ t_in, const unsigned char* mask_in,
                                                                        int N, double thr2, int iters, int with_scale,
                                                                        double* __restrict__ s_out, double* __restrict__ R_out,
                                                                        double* __restrict__ t_out, unsigned char* __restrict__ mask_out,
                                                                        double* __restrict__ cost_out, int* __restrict__ count_out,
                                                                        int* __restrict__ steps_out) {
  __shared__ double red[SIM_WAVES][SIM_NSUM], in[13];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)p * N;
  if (tid < 9) in[tid] = R_in[p * 9 + tid];
  if (tid < 3) in[9 + tid] = t_in[p * 3 + tid];
  if (tid == 0) in[12] = s_in[p];
  __syncthreads();
  Sim given;
#pragma unroll
  for (int i = 0; i < 9; ++i) given.R[i] = in[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) given.t[i] = in[9 + i];
  given.s = in[12];
  const bool good = sim_finite(given);

  // the normalisation of sim_prepare_kernel over the usable matches: centroids, then the mean distances
  const double* X = Xw + base * 3;
  const double* Y = Yw + base * 3;
  auto usable = [&](int i) { return finite6(X + 3 * (size_t)i, Y + 3 * (size_t)i) && (!mask_in || mask_in[base + i] != 0); };
  double c[6], sX, sY;
  {
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += SIM_THREADS)
      if (usable(i)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] += X[3 * (size_t)i + k]; a[3 + k] += Y[3 * (size_t)i + k]; }
        a[6] += 1.0;
      }
    block_sum<7, SIM_WAVES>(a, red);
    const double inv = a[6] > 0.0 ? 1.0 / a[6] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = a[k] * inv;
    double d[2] = {0.0, 0.0};
    for (int i = tid; i < N; i += SIM_THREADS)
      if (usable(i)) {
        const double x0 = X[3 * (size_t)i] - c[0], x1 = X[3 * (size_t)i + 1] - c[1], x2 = X[3 * (size_t)i + 2] - c[2];
        const double y0 = Y[3 * (size_t)i] - c[3], y1 = Y[3 * (size_t)i + 1] - c[4], y2 = Y[3 * (size_t)i + 2] - c[5];
        d[0] += sqrt(x0 * x0 + x1 * x1 + x2 * x2);
        d[1] += sqrt(y0 * y0 + y1 * y1 + y2 * y2);
      }
    block_sum<2, SIM_WAVES>(d, red);
    sY = cloud_scale(d[1] * inv);
    sX = with_scale ? cloud_scale(d[0] * inv) : sY;
  }
  auto load = [&](int i, double* x, double* y) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = (X[3 * (size_t)i + k] - c[k]) * sX; y[k] = (Y[3 * (size_t)i + k] - c[3 + k]) * sY; }
    return usable(i);
  };
  const double t2 = thr2 * sY * sY;
  Sim cur = given;                                               // the input in the normalised frame
  cur.s = given.s * sY / sX;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    cur.t[i] = sY * (given.s * (given.R[3 * i] * c[0] + given.R[3 * i + 1] * c[1] + given.R[3 * i + 2] * c[2]) + given.t[i] - c[3 + i]);

  double s[SIM_NSUM];
  sim_evaluate<SCORE_MSAC>(cur, load, N, t2, red, s);
  int steps = 0;
  if (good) {
    for (int it = 0; it < iters; ++it) {
      Sim cand;
      double sn[SIM_NSUM];
      if (!(s[SIM_COUNT] >= (double)SIM_MIN_MATCHES) || !sim_closed_form(s, with_scale != 0, SIM_GAP_TOL, cand)) break;
      sim_evaluate<SCORE_MSAC>(cand, load, N, t2, red, sn);
      if (!(sn[SIM_COST] < s[SIM_COST] * (1.0 - SIM_ACCEPT_REL))) break;
      cur = cand;
#pragma unroll
      for (int k = 0; k < SIM_NSUM; ++k) s[k] = sn[k];
      ++steps;
    }
  }
  const bool kept = steps > 0;                                  // else the input model, as it came
  const double so = kept ? cur.s * sX / sY : given.s;
  if (tid < 9) R_out[p * 9 + tid] = cur.R[tid];
  if (tid < 3)
    t_out[p * 3 + tid] = kept ? cur.t[tid] / sY + c[3 + tid] - so * (cur.R[3 * tid] * c[0] + cur.R[3 * tid + 1] * c[1] + cur.R[3 * tid + 2] * c[2])
                              : given.t[tid];
  if (tid == 0) {
    s_out[p] = so;
    cost_out[p] = s[SIM_COST] / (sY * sY);
    count_out[p] = (int)s[SIM_COUNT];
    steps_out[p] = steps;
  }
  for (int i = tid; i < N; i += SIM_THREADS) {
    double x[3], y[3];
    const bool ok = load(i, x, y);
    mask_out[base + i] = (ok && sim_error(cur, x, y) < t2) ? 1 : 0;
  }
}

// --------------------------------------------------------------------------------------------------------------- workspace
// ransac_common.h's regions with S = 3 and R = 1 ([3] holds R), then (t', s'), the (Y'_y, Y'_z) of the scoring records and the fp64 copy
constexpr int WM_TS = WS_N, WM_PY = WS_N + 1, WM_XN = WS_N + 2, WM_N = WS_N + 3;

long layout_sim(int P, int N, int iters, long* off) {
  const long extra[3] = {(long)P * iters * SIM_R * 32, (long)P * N * 8, (long)P * N * 48};
  return ws_layout(SIM_S, SIM_R, P, N, iters, extra, 3, off);
}

int check_args_sim(const char* fn, const void* X, const void* Y, const void* ws, int P, int N, int iters, float threshold, int scoring,
                   long ws_bytes) {
  ROMA_REQUIRE(X && Y && ws, ROMA_E_ARG, "%s: null pointer", fn);
  int rc = check_problem(fn, P, N, iters, SIM_S, SIM_SOLVE_THREADS, threshold);
  if (rc) return rc;
  rc = check_scoring(fn, scoring);                               // before the workspace here, behind it in the other three files
  if (rc) return rc;
  rc = check_workspace(fn, ws_bytes, layout_sim(P, N, iters, nullptr));
  if (rc) return rc;
  ROMA_REQUIRE(aligned16(ws), ROMA_E_ALIGN, "%s: the workspace must be 16-byte aligned", fn);
  ROMA_REQUIRE(aligned8(X) && aligned8(Y), ROMA_E_ALIGN, "%s: X and Y must be 8-byte aligned", fn);
  return 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_similarity_workspace(int P, int N, int iters, long* offsets) {
  if (P < 1 || N < 1 || iters < 1) {
    set_error("roma_similarity_workspace: bad arguments P=%d N=%d iters=%d", P, N, iters);
    return ROMA_E_ARG;
  }
  return layout_sim(P, N, iters, offsets);
}

extern "C" int roma_similarity_hypotheses(const double* X, const double* Y, int P, int N, int iters, float threshold, int scoring,
                                          int with_scale, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  const char* fn = __func__;
  int rc = check_args_sim(fn, X, Y, ws, P, N, iters, threshold, scoring, ws_bytes);
  if (rc) return rc;
  rc = check_pair_offset(fn, p0);
  if (rc) return rc;
  long off[WM_N];
  layout_sim(P, N, iters, off);
  const Regions r = regions(ws, off);
  double* ts = region<double>(ws, off, WM_TS);
  float2* py = region<float2>(ws, off, WM_PY);
  double* xn = region<double>(ws, off, WM_XN);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int M = iters * SIM_R, C = (N + CHUNK - 1) / CHUNK;
  const uint32_t sstream = sample_stream(seed, STAGE_SIM);
  const float thr2 = threshold * threshold;                      // in Y units; the kernels scale it by the pair's sY^2
  const Grids g = ransac_grids(P, N, iters, SIM_R, SIM_SOLVE_THREADS);
  hipLaunchKernelGGL(sim_prepare_kernel, dim3(P), dim3(256), 0, st, X, Y, N, with_scale, r.norm, r.pts, py, xn);
  hipLaunchKernelGGL(sim_solve_kernel, g.solve, dim3(SIM_SOLVE_THREADS), 0, st, xn, r.pts, P, N, iters, sstream, p0, with_scale, r.samples,
                     r.models, ts, r.valid);
  const auto score = by_scoring(scoring, sim_score_kernel<SCORE_MSAC>, sim_score_kernel<SCORE_MAGSAC>);
  hipLaunchKernelGGL(score, g.score, dim3(256), 0, st, r.pts, py, r.models, ts, r.valid, r.norm, N, M, thr2, r.slab_cost, r.slab_cnt);
  hipLaunchKernelGGL(reduce_kernel, g.reduce, dim3(256), 0, st, r.slab_cost, r.slab_cnt, r.valid, P, M, C, r.cost, r.count);
  return check_launch(fn);
}

extern "C" int roma_similarity_select(const double* X, const double* Y, int P, int N, int iters, float threshold, int scoring,
                                      int with_scale, int lo_iters, const void* ws, long ws_bytes, double* s, double* R, double* t,
                                      unsigned char* mask, int* valid, void* stream) {
  const char* fn = __func__;
  int rc = check_args_sim(fn, X, Y, ws, P, N, iters, threshold, scoring, ws_bytes);
  if (rc) return rc;
  ROMA_REQUIRE(s && R && t && mask && valid, ROMA_E_ARG, "%s: null pointer", fn);
  rc = check_lo_iters(fn, lo_iters);
  if (rc) return rc;
  long off[WM_N];
  layout_sim(P, N, iters, off);
  const Regions r = regions(ws, off);
  const auto sel = by_scoring(scoring, sim_select_kernel<SCORE_MSAC>, sim_select_kernel<SCORE_MAGSAC>);
  // X and Y are not read again: the kernel works on the normalised copy that roma_similarity_hypotheses left in the workspace
  hipLaunchKernelGGL(sel, dim3(P), dim3(SIM_THREADS), 0, static_cast<hipStream_t>(stream), r.norm, r.pts, region<float2>(ws, off, WM_PY),
                     region<double>(ws, off, WM_XN), r.models, region<double>(ws, off, WM_TS), r.cost, N, iters * SIM_R,
                     threshold * threshold, with_scale, lo_iters, s, R, t, mask, valid);
  return check_launch(fn);
}

extern "C" int roma_refine_similarity(const double* X, const double* Y, const double* s_in, const double* R_in, const double* t_in,
                                      const unsigned char* mask_in, int P, int N, double threshold, int iters, int with_scale, double* s,
                                      double* R, double* t, unsigned char* mask, double* cost, int* count, int* steps, void* stream) {
  const char* fn = __func__;
  ROMA_REQUIRE(X && Y && s_in && R_in && t_in && s && R && t && mask && cost && count && steps, ROMA_E_ARG, "%s: null pointer", fn);
  ROMA_REQUIRE(P >= 1 && P <= (1 << 24), ROMA_E_SHAPE, "%s: bad shape P=%d", fn, P);
  ROMA_REQUIRE(N >= SIM_MIN_MATCHES && N <= (1 << 26), ROMA_E_SHAPE, "%s: N=%d matches, need at least %d", fn, N, SIM_MIN_MATCHES);
  ROMA_REQUIRE(threshold > 0.0 && threshold < 1e18, ROMA_E_ARG, "%s: threshold must be positive, got %g", fn, threshold);
  ROMA_REQUIRE(iters >= 0 && iters <= (1 << 16), ROMA_E_ARG, "%s: iters must be in [0, 65536], got %d", fn, iters);
  ROMA_REQUIRE(aligned8(X) && aligned8(Y), ROMA_E_ALIGN, "%s: X and Y must be 8-byte aligned", fn);
  hipLaunchKernelGGL(refine_similarity_kernel, dim3(P), dim3(SIM_THREADS), 0, static_cast<hipStream_t>(stream), X, Y, s_in, R_in, t_in,
                     mask_in, N, threshold * threshold, iters, with_scale, s, R, t, mask, cost, count, steps);
  return check_launch(fn);
}
