// Robust two-view geometry: RANSAC (MSAC scoring + least-squares local optimisation; on request MAGSAC++ scoring + iteratively
// re-weighted least squares, the *_ex entry points) for fundamental matrices (7-point) and
// homographies (4-point DLT).  Replaces the estimator every caller of the reference runs after match -> sample ->
// to_pixel_coordinates: cv2.findFundamentalMat (demo/demo_fundamental.py:28-34, romatch/utils/utils.py:54-62) and
// cv2.findHomography (romatch/benchmarks/hpatches_sequences_homog_benchmark.py:72-86).  DESIGN.md §3.4.
//
// Pipeline, one call of roma_ransac_hypotheses + one of roma_ransac_select (P pairs of N matches, H = iters samples each):
//   normalize_kernel  (P,2) blocks      Hartley normalisation per pair and image, fp64, fixed-order LDS tree; fp32 copy of the
//                                       normalised points (NaN where a match is not finite: never sampled, never an inlier)
//   minimal_kernel    one thread/sample draws the sample and solves the minimal problem in fp64 -> R slots (R = 3 for F, 1 for H)
//   score_kernel      (slots/256, S, P)  every slot against one 1024-point chunk staged in LDS (broadcast reads), fp32 VALU;
//                                       partial MSAC cost + inlier count per (chunk, slot) into a slab, no atomics
//   reduce_kernel     one thread/slot   sums the slab in chunk order -> cost (fp64) and count per slot
//   select_kernel     one block/pair    lowest cost (lowest slot index on ties), lo_iters rounds of least-squares refit
//                                       (9x9 normal matrix, fixed-order fp64 tree, Jacobi on one wave), de-normalisation, mask
//
// Sample draw (tests/geometry_ref.py restates it bit for bit):
//   stream = fmix32(seed ^ (stage * 0x9E3779B9)), stage = 2 for F, 3 for H
//   ctr    = ((p * iters + h) * 8 + k)                                  p = pair index in the call, h = sample, k = point of it
//   hash   = fmix32(stream + ctr * 0x9E3779B1 + attempt * 0x7FEB352D)   attempt = 0..15; all arithmetic uint32, wrapping
//   index  = (uint32)(((uint64)hash * N) >> 32)
// An index that repeats an earlier index of the same sample, or names a match that is not finite, is drawn again with the next
// attempt; after 16 attempts the sample is invalid (all its indices are written as -1).
//
// Rank test of the minimal systems: Gaussian elimination with partial pivoting; a pivot with |pivot| <= 1e-10 * (largest
// |entry| of the system) rejects the sample.  H samples are also rejected when any 3 of the 4 points are collinear in either
// image: |(b - a) x (c - a)| <= 1e-6 |b - a| |c - a| (normalised coordinates).
//
// Shared code: ransac_common.h has the scoring (score_kernel, reduce_kernel, block_score), the workspace layout, the host helpers
// and the checks that essential.hip, absolute_pose.hip and similarity.hip use too; twoview_math.h the fp64 helpers (elimination, jacobi_lds, Norm / to_pixels) that the refinement
// kernels use as well.  Steps 1 and 2 of select_kernel are repeated in essential_select_kernel, statement for statement.
#include "ransac_common.h"

namespace roma {
namespace {

// ---------------------------------------------------------------------------------------------------------------- normalise
// norm[p*8 + img*4 + {0,1,2}] = (cx, cy, s): x_hat = (x - c) * s.
__global__ __launch_bounds__(256) void normalize_kernel(const double* __restrict__ xa, const double* __restrict__ xb, int N,
                                                        double* __restrict__ norm, float* __restrict__ pts) {
  __shared__ double red[2][256];
  __shared__ int ired[256];
  const int p = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const double* a = xa + (size_t)p * N * 2;
  const double* b = xb + (size_t)p * N * 2;
  const double* x = img == 0 ? a : b;
  double sx = 0.0, sy = 0.0;
  int n = 0;
  for (int i = tid; i < N; i += 256) {
    const bool ok = isfinite(a[2 * i]) && isfinite(a[2 * i + 1]) && isfinite(b[2 * i]) && isfinite(b[2 * i + 1]);
    if (ok) { sx += x[2 * i]; sy += x[2 * i + 1]; ++n; }
  }
  red[0][tid] = sx; red[1][tid] = sy; ired[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; ired[tid] += ired[tid + o]; }
    __syncthreads();
  }
  const int cnt = ired[0];
  const double cx = cnt > 0 ? red[0][0] / cnt : 0.0, cy = cnt > 0 ? red[1][0] / cnt : 0.0;
  __syncthreads();
  double sd = 0.0;
  for (int i = tid; i < N; i += 256) {
    const bool ok = isfinite(a[2 * i]) && isfinite(a[2 * i + 1]) && isfinite(b[2 * i]) && isfinite(b[2 * i + 1]);
    if (ok) { const double dx = x[2 * i] - cx, dy = x[2 * i + 1] - cy; sd += sqrt(dx * dx + dy * dy); }
  }
  red[0][tid] = sd;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[0][tid] += red[0][tid + o];
    __syncthreads();
  }
  const double md = cnt > 0 ? red[0][0] / cnt : 0.0;
  double s = 1.4142135623730951 / md;
  if (!(md > 0.0) || !isfinite(s)) s = 1.0;                    // identical points (or none finite): every sample is degenerate
  if (tid == 0) {
    norm[p * 8 + img * 4 + 0] = cx;
    norm[p * 8 + img * 4 + 1] = cy;
    norm[p * 8 + img * 4 + 2] = s;
    norm[p * 8 + img * 4 + 3] = 0.0;
  }
  for (int i = tid; i < N; i += 256) {
    const bool ok = isfinite(a[2 * i]) && isfinite(a[2 * i + 1]) && isfinite(b[2 * i]) && isfinite(b[2 * i + 1]);
    float* q = pts + ((size_t)p * N + i) * 4 + img * 2;
    q[0] = ok ? (float)((x[2 * i] - cx) * s) : __builtin_nanf("");
    q[1] = ok ? (float)((x[2 * i + 1] - cy) * s) : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------------------------------------------ minimal solvers (fp64)
// f2 + a * (f1 - f2), determinant
__device__ __forceinline__ double det_mix(const double* f1, const double* f2, double a) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = f2[i] + a * (f1[i] - f2[i]);
  return det3(m);
}

// two Newton steps on the cubic
__device__ __forceinline__ double newton2(double c3, double c2, double c1, double c0, double x) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double f = ((c3 * x + c2) * x + c1) * x + c0;
    const double df = (3.0 * c3 * x + 2.0 * c2) * x + c1;
    if (df != 0.0) x -= f / df;
  }
  return x;
}

// Real roots of c3 a^3 + c2 a^2 + c1 a + c0 (closed form, then two Newton steps on the cubic).  Returns the count (0..3).
__device__ __forceinline__ int cubic_roots(double c3, double c2, double c1, double c0, double& r0, double& r1, double& r2) {
  const double cmax = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
  int n = 0;
  r0 = r1 = r2 = 0.0;
  if (!(cmax > 0.0)) return 0;
  if (fabs(c3) <= 1e-12 * cmax) {                                // degree drops: the root at infinity is not a model
    if (fabs(c2) <= 1e-12 * cmax) {
      if (fabs(c1) <= 1e-12 * cmax) return 0;
      r0 = -c0 / c1;
      return 1;
    }
    const double d = c1 * c1 - 4.0 * c2 * c0;
    if (d < 0.0) return 0;
    const double sq = sqrt(d);
    const double q = -0.5 * (c1 + (c1 >= 0.0 ? sq : -sq));
    if (q == 0.0) { r0 = 0.0; return 1; }
    r0 = q / c2;
    r1 = c0 / q;
    return 2;
  }
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  const double pp = b - a * a / 3.0;
  const double qq = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c;
  const double disc = 0.25 * qq * qq + pp * pp * pp / 27.0;
  if (pp < 0.0 && disc <= 0.0) {
    const double r = 2.0 * sqrt(-pp / 3.0);
    double arg = 3.0 * qq / (2.0 * pp) * sqrt(-3.0 / pp);
    arg = fmin(1.0, fmax(-1.0, arg));
    const double phi = acos(arg) / 3.0;
    r0 = r * cos(phi) - a / 3.0;
    r1 = r * cos(phi - 2.0943951023931957) - a / 3.0;
    r2 = r * cos(phi - 4.1887902047863905) - a / 3.0;
    n = 3;
  } else {
    const double sq = sqrt(fmax(disc, 0.0));
    r0 = cbrt(-0.5 * qq + sq) + cbrt(-0.5 * qq - sq) - a / 3.0;
    n = 1;
  }
  r0 = newton2(c3, c2, c1, c0, r0);
  if (n == 3) { r1 = newton2(c3, c2, c1, c0, r1); r2 = newton2(c3, c2, c1, c0, r2); }
  return n;
}

__device__ __forceinline__ bool collinear(double ax, double ay, double bx, double by, double cx, double cy) {
  const double ux = bx - ax, uy = by - ay, vx = cx - ax, vy = cy - ay;
  return fabs(ux * vy - uy * vx) <= COLLINEAR_TOL * sqrt(ux * ux + uy * uy) * sqrt(vx * vx + vy * vy);
}

// samples: (P, iters, S) int32; models: (P, iters, R, 9) fp64 in normalised coordinates (unit Frobenius norm); valid: (P, iters, R)
template <int KIND>
__global__ __launch_bounds__(128) void minimal_kernel(const double* __restrict__ xa, const double* __restrict__ xb,
                                                      const double* __restrict__ norm, const float* __restrict__ pts, int P, int N,
                                                      int iters, uint32_t stream, int p0, int* __restrict__ samples,
                                                      double* __restrict__ models, int* __restrict__ valid) {
  constexpr int S = Kind<KIND>::S, R = Kind<KIND>::R;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)P * iters) return;
  const int p = (int)(t / iters), h = (int)(t % iters);
  const size_t base = (size_t)p * N;
  int idx[S];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const uint32_t ctr = (((uint32_t)(p0 + p) * (uint32_t)iters + (uint32_t)h) * 8u + (uint32_t)k);
    int got = -1;
    for (uint32_t att = 0; att < 16; ++att) {
      const uint32_t hs = fmix32(stream + ctr * 0x9E3779B1u + att * 0x7FEB352Du);
      const int i = (int)(((uint64_t)hs * (uint64_t)(uint32_t)N) >> 32);
      const float v = pts[(base + i) * 4];
      bool good = v == v;                                         // not finite -> NaN in the normalised copy
#pragma unroll
      for (int j = 0; j < k; ++j) good = good && idx[j] != i;
      if (good) { got = i; break; }
    }
    idx[k] = got;
    ok = ok && got >= 0;
  }
#pragma unroll
  for (int k = 0; k < S; ++k) samples[(size_t)t * S + k] = ok ? idx[k] : -1;

  double mdl[R][9];
  bool vld[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    vld[r] = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) mdl[r][i] = 0.0;
  }
  if (ok) {
    const double cxA = norm[p * 8 + 0], cyA = norm[p * 8 + 1], sA = norm[p * 8 + 2];
    const double cxB = norm[p * 8 + 4], cyB = norm[p * 8 + 5], sB = norm[p * 8 + 6];
    double X[S], Y[S], U[S], V[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const size_t q = (base + idx[k]) * 2;
      X[k] = (xa[q] - cxA) * sA; Y[k] = (xa[q + 1] - cyA) * sA;
      U[k] = (xb[q] - cxB) * sB; V[k] = (xb[q + 1] - cyB) * sB;
    }
    if constexpr (KIND == KIND_F) {
      // x'^T F x = 0, F row-major: row = [u x, u y, u, v x, v y, v, x, y, 1]
      double A[7][9];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        A[k][0] = U[k] * X[k]; A[k][1] = U[k] * Y[k]; A[k][2] = U[k];
        A[k][3] = V[k] * X[k]; A[k][4] = V[k] * Y[k]; A[k][5] = V[k];
        A[k][6] = X[k]; A[k][7] = Y[k]; A[k][8] = 1.0;
      }
      if (eliminate<7>(A)) {
        double f1[9], f2[9];
        f1[7] = 1.0; f1[8] = 0.0; f2[7] = 0.0; f2[8] = 1.0;
        back_substitute<7>(A, f1);
        back_substitute<7>(A, f2);
        unit_frobenius(f1);
        unit_frobenius(f2);
        // det(f2 + a (f1 - f2)) = c3 a^3 + c2 a^2 + c1 a + c0 from its values at a = 0, 1, -1, 2
        const double d0 = det_mix(f1, f2, 0.0), d1 = det_mix(f1, f2, 1.0), dm = det_mix(f1, f2, -1.0), d2 = det_mix(f1, f2, 2.0);
        const double c0 = d0, c2 = 0.5 * (d1 + dm) - d0;
        const double m = 0.5 * (d1 - dm), nn = 0.5 * (d2 - d0 - 4.0 * c2);
        const double c3 = (nn - m) / 3.0, c1 = m - c3;
        double rt[3];
        const int nr = cubic_roots(c3, c2, c1, c0, rt[0], rt[1], rt[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (r < nr) {
#pragma unroll
            for (int i = 0; i < 9; ++i) mdl[r][i] = f2[i] + rt[r] * (f1[i] - f2[i]);
            unit_frobenius(mdl[r]);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 9; ++i) fin = fin && isfinite(mdl[r][i]);
            vld[r] = fin;
            if (!fin) {
#pragma unroll
              for (int i = 0; i < 9; ++i) mdl[r][i] = 0.0;
            }
          }
        }
      }
    } else {
      bool deg = false;
      deg = deg || collinear(X[0], Y[0], X[1], Y[1], X[2], Y[2]) || collinear(X[0], Y[0], X[1], Y[1], X[3], Y[3]);
      deg = deg || collinear(X[0], Y[0], X[2], Y[2], X[3], Y[3]) || collinear(X[1], Y[1], X[2], Y[2], X[3], Y[3]);
      deg = deg || collinear(U[0], V[0], U[1], V[1], U[2], V[2]) || collinear(U[0], V[0], U[1], V[1], U[3], V[3]);
      deg = deg || collinear(U[0], V[0], U[2], V[2], U[3], V[3]) || collinear(U[1], V[1], U[2], V[2], U[3], V[3]);
      if (!deg) {
        // x' ~ H x: [x y 1 0 0 0 -u x -u y -u], [0 0 0 x y 1 -v x -v y -v]
        double A[8][9];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          A[2 * k][0] = X[k]; A[2 * k][1] = Y[k]; A[2 * k][2] = 1.0;
          A[2 * k][3] = 0.0; A[2 * k][4] = 0.0; A[2 * k][5] = 0.0;
          A[2 * k][6] = -U[k] * X[k]; A[2 * k][7] = -U[k] * Y[k]; A[2 * k][8] = -U[k];
          A[2 * k + 1][0] = 0.0; A[2 * k + 1][1] = 0.0; A[2 * k + 1][2] = 0.0;
          A[2 * k + 1][3] = X[k]; A[2 * k + 1][4] = Y[k]; A[2 * k + 1][5] = 1.0;
          A[2 * k + 1][6] = -V[k] * X[k]; A[2 * k + 1][7] = -V[k] * Y[k]; A[2 * k + 1][8] = -V[k];
        }
        if (eliminate<8>(A)) {
          mdl[0][8] = 1.0;
          back_substitute<8>(A, mdl[0]);
          unit_frobenius(mdl[0]);
          bool fin = true;
#pragma unroll
          for (int i = 0; i < 9; ++i) fin = fin && isfinite(mdl[0][i]);
          vld[0] = fin;
          if (!fin) {
#pragma unroll
            for (int i = 0; i < 9; ++i) mdl[0][i] = 0.0;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    valid[(size_t)t * R + r] = vld[r] ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) models[((size_t)t * R + r) * 9 + i] = mdl[r][i];
  }
}

template <int KIND, int SCORE>
__global__ __launch_bounds__(256) void select_kernel(const double* __restrict__ xa, const double* __restrict__ xb,
                                                     const float4* __restrict__ pts, const double* __restrict__ norm,
                                                     const double* __restrict__ models, const double* __restrict__ cost, int N, int M,
                                                     float t2, int lo_iters, double* __restrict__ out_model,
                                                     unsigned char* __restrict__ mask) {
  __shared__ double dred[256];
  __shared__ int ired[256];
  __shared__ double A[81], V[81], cur[9], cand[9], wsum[4][45];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float4* pq = pts + (size_t)p * N;
  const double* nrm = norm + p * 8;

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
  float ka, kb;
  error_scales<KIND>(nrm, ka, kb);
  double cc;
  int cn;
  block_score<KIND, SCORE>(cur, pq, N, ka, kb, t2, dred, ired, cc, cn);

  // 2. local optimisation: least-squares refit on the inliers (SCORE_MAGSAC: weighted by W under the current model, the rows scaled
  // by sqrt W), kept only if its cost is lower
  const Norm nm{nrm[0], nrm[1], nrm[2], nrm[4], nrm[5], nrm[6]};
  for (int round = 0; round < lo_iters; ++round) {
    if (cn < Kind<KIND>::LO_MIN) break;
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (float)cur[i];
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.0;
    for (int i = tid; i < N; i += 256) {
      const float e = point_error<KIND>(m, pq[i], ka, kb);
      if (!(e < t2)) continue;
      const size_t q = ((size_t)p * N + i) * 2;
      const double x = (xa[q] - nm.cxA) * nm.sA, y = (xa[q + 1] - nm.cyA) * nm.sA, u = (xb[q] - nm.cxB) * nm.sB,
                   v = (xb[q + 1] - nm.cyB) * nm.sB;
      double sw = 1.0;
      if constexpr (SCORE == SCORE_MAGSAC) sw = sqrt((double)magsac_lookup(magsac_weight_cells, e, (float)MAGSAC_CELLS / t2));
      if constexpr (KIND == KIND_F) {
        double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        if constexpr (SCORE == SCORE_MAGSAC) {
#pragma unroll
          for (int r = 0; r < 9; ++r) a[r] *= sw;
        }
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
          for (int c = r; c < 9; ++c) { acc[k] = __builtin_fma(a[r], a[c], acc[k]); ++k; }
      } else {
        double a[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u};
        double b[9] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v};
        if constexpr (SCORE == SCORE_MAGSAC) {
#pragma unroll
          for (int r = 0; r < 9; ++r) { a[r] *= sw; b[r] *= sw; }
        }
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
          for (int c = r; c < 9; ++c) { acc[k] = __builtin_fma(a[r], a[c], __builtin_fma(b[r], b[c], acc[k])); ++k; }
      }
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
    if (tid < 9) cand[tid] = V[tid * 9 + j];
    __syncthreads();
    if constexpr (KIND == KIND_F) {
      // rank 2: F <- F - (F v) v^T, v the right singular vector of the smallest singular value (eigenvector of F^T F)
      if (tid < 9) {
        const int r = tid / 3, c = tid % 3;
        A[r * 9 + c] = cand[r] * cand[c] + cand[3 + r] * cand[3 + c] + cand[6 + r] * cand[6 + c];
        V[r * 9 + c] = r == c ? 1.0 : 0.0;
      }
      __syncthreads();
      jacobi_lds(A, V, 3);
      if (tid == 0) {
        const int j3 = argmin_diag(A, 3);
        const double v0 = V[0 * 9 + j3], v1 = V[1 * 9 + j3], v2 = V[2 * 9 + j3];
        double f[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double fv = cand[3 * r] * v0 + cand[3 * r + 1] * v1 + cand[3 * r + 2] * v2;
          f[3 * r] = cand[3 * r] - fv * v0;
          f[3 * r + 1] = cand[3 * r + 1] - fv * v1;
          f[3 * r + 2] = cand[3 * r + 2] - fv * v2;
        }
        unit_frobenius(f);
#pragma unroll
        for (int i = 0; i < 9; ++i) cand[i] = f[i];
      }
      __syncthreads();
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(cand[i]);
    if (!fin) break;                                              // block-uniform (LDS)
    double c2;
    int n2;
    block_score<KIND, SCORE>(cand, pq, N, ka, kb, t2, dred, ired, c2, n2);
    if (!(c2 < cc)) break;
    if (tid < 9) cur[tid] = cand[tid];
    __syncthreads();
    cc = c2;
    cn = n2;
  }

  // 3. de-normalise (F = T_B^T F^ T_A, H = T_B^-1 H^ T_A), fix scale and sign; mask from the final model
  if (tid == 0) {
    double o[9];
    if constexpr (KIND == KIND_F) {
      to_pixels(cur, nm, o);
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
    } else {
      double g[9];
      times_t_a(cur, nm, g);
      // T_B^-1 G: rows 0,1 = row / sB + cB * row 2
#pragma unroll
      for (int cc2 = 0; cc2 < 3; ++cc2) {
        o[cc2] = g[cc2] / nm.sB + nm.cxB * g[6 + cc2];
        o[3 + cc2] = g[3 + cc2] / nm.sB + nm.cyB * g[6 + cc2];
        o[6 + cc2] = g[6 + cc2];
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
#pragma unroll
    for (int i = 0; i < 9; ++i) out_model[p * 9 + i] = o[i];
  }
  float m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = (float)cur[i];
  for (int i = tid; i < N; i += 256) mask[(size_t)p * N + i] = point_error<KIND>(m, pq[i], ka, kb) < t2 ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------------- workspace
long layout(int kind, int P, int N, int iters, long* off) {
  return ws_layout(kind == KIND_F ? 7 : 4, kind == KIND_F ? 3 : 1, P, N, iters, nullptr, 0, off);
}

int check_args(const char* fn, int kind, const void* xa, const void* xb, const void* ws, int P, int N, int iters, long ws_bytes) {
  ROMA_REQUIRE(xa && xb && ws, ROMA_E_ARG, "%s: null pointer", fn);
  ROMA_REQUIRE(kind == KIND_F || kind == KIND_H, ROMA_E_ARG, "%s: kind must be 0 (fundamental) or 1 (homography), got %d", fn, kind);
  const int rc = check_shape(fn, P, N, iters, kind == KIND_F ? 7 : 4);
  return rc ? rc : check_workspace(fn, ws_bytes, layout(kind, P, N, iters, nullptr));
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_ransac_workspace(int kind, int P, int N, int iters, long* offsets) {
  if ((kind != KIND_F && kind != KIND_H) || P < 1 || N < 1 || iters < 1) {
    set_error("roma_ransac_workspace: bad arguments kind=%d P=%d N=%d iters=%d", kind, P, N, iters);
    return ROMA_E_ARG;
  }
  return layout(kind, P, N, iters, offsets);
}

namespace {

int ransac_hypotheses(const char* fn, int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold,
                      int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  int rc = check_args(fn, kind, xa, xb, ws, P, N, iters, ws_bytes);
  if (rc) return rc;
  rc = check_threshold(fn, threshold);
  if (rc) return rc;
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_pair_offset(fn, p0);
  if (rc) return rc;
  long off[WS_N];
  layout(kind, P, N, iters, off);
  const Regions r = regions(ws, off);
  float* pts = (float*)r.pts;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int R = kind == KIND_F ? 3 : 1, M = iters * R, C = (N + CHUNK - 1) / CHUNK;
  const uint32_t sstream = sample_stream(seed, kind == KIND_F ? STAGE_F : STAGE_H);
  const float t2 = threshold * threshold;
  const Grids g = ransac_grids(P, N, iters, R, 128);
  hipLaunchKernelGGL(normalize_kernel, dim3(P, 2), dim3(256), 0, st, xa, xb, N, r.norm, pts);
  if (kind == KIND_F)
    hipLaunchKernelGGL(minimal_kernel<KIND_F>, g.solve, dim3(128), 0, st, xa, xb, r.norm, pts, P, N, iters, sstream, p0, r.samples, r.models,
                       r.valid);
  else
    hipLaunchKernelGGL(minimal_kernel<KIND_H>, g.solve, dim3(128), 0, st, xa, xb, r.norm, pts, P, N, iters, sstream, p0, r.samples, r.models,
                       r.valid);
  const auto score = kind == KIND_F ? by_scoring(scoring, score_kernel<KIND_F, SCORE_MSAC>, score_kernel<KIND_F, SCORE_MAGSAC>)
                                    : by_scoring(scoring, score_kernel<KIND_H, SCORE_MSAC>, score_kernel<KIND_H, SCORE_MAGSAC>);
  hipLaunchKernelGGL(score, g.score, dim3(256), 0, st, r.pts, r.norm, r.models, r.valid, N, M, t2, r.slab_cost, r.slab_cnt);
  hipLaunchKernelGGL(reduce_kernel, g.reduce, dim3(256), 0, st, r.slab_cost, r.slab_cnt, r.valid, P, M, C, r.cost, r.count);
  return check_launch(fn);
}

int ransac_select(const char* fn, int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int scoring,
                  int lo_iters, const void* ws, long ws_bytes, double* model, unsigned char* mask, void* stream) {
  int rc = check_args(fn, kind, xa, xb, ws, P, N, iters, ws_bytes);
  if (rc) return rc;
  ROMA_REQUIRE(model && mask, ROMA_E_ARG, "%s: null pointer", fn);
  rc = check_threshold(fn, threshold);
  if (rc) return rc;
  rc = check_scoring(fn, scoring);
  if (rc) return rc;
  rc = check_lo_iters(fn, lo_iters);
  if (rc) return rc;
  long off[WS_N];
  layout(kind, P, N, iters, off);
  const Regions r = regions(ws, off);
  const int M = iters * (kind == KIND_F ? 3 : 1);
  const float t2 = threshold * threshold;
  const auto sel = kind == KIND_F ? by_scoring(scoring, select_kernel<KIND_F, SCORE_MSAC>, select_kernel<KIND_F, SCORE_MAGSAC>)
                                  : by_scoring(scoring, select_kernel<KIND_H, SCORE_MSAC>, select_kernel<KIND_H, SCORE_MAGSAC>);
  hipLaunchKernelGGL(sel, dim3(P), dim3(256), 0, static_cast<hipStream_t>(stream), xa, xb, r.pts, r.norm, r.models, r.cost, N, M, t2,
                     lo_iters, model, mask);
  return check_launch(fn);
}

}  // namespace

extern "C" int roma_ransac_hypotheses(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold,
                                      unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  return ransac_hypotheses(__func__, kind, xa, xb, P, N, iters, threshold, SCORE_MSAC, seed, p0, ws, ws_bytes, stream);
}

extern "C" int roma_ransac_hypotheses_ex(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold,
                                         int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream) {
  return ransac_hypotheses(__func__, kind, xa, xb, P, N, iters, threshold, scoring, seed, p0, ws, ws_bytes, stream);
}

extern "C" int roma_ransac_select(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int lo_iters,
                                  const void* ws, long ws_bytes, double* model, unsigned char* mask, void* stream) {
  return ransac_select(__func__, kind, xa, xb, P, N, iters, threshold, SCORE_MSAC, lo_iters, ws, ws_bytes, model, mask, stream);
}

extern "C" int roma_ransac_select_ex(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int scoring,
                                     int lo_iters, const void* ws, long ws_bytes, double* model, unsigned char* mask, void* stream) {
  return ransac_select(__func__, kind, xa, xb, P, N, iters, threshold, scoring, lo_iters, ws, ws_bytes, model, mask, stream);
}

extern "C" int roma_magsac_table(float* loss, float* weight) {
  ROMA_REQUIRE(loss && weight, ROMA_E_ARG, "roma_magsac_table: null pointer");
  for (int i = 0; i < MAGSAC_NODES; ++i) { loss[i] = MAGSAC_LOSS[i]; weight[i] = MAGSAC_WEIGHT[i]; }
  return 0;
}
