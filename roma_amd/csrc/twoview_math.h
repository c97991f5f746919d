// The fp64 device helpers of the two-view geometry kernels (geometry.hip, essential.hip, pose_refine.hip, fundamental_refine.hip,
// homography_refine.hip, triangulate.hip; absolute_pose.hip and similarity.hip through ransac_common.h) and, through multiview.h, of
// the multi-view kernels (triangulate_nview.hip, tracks.hip, bundle.hip, depth_fuse.hip, motion_average.hip): small 3 x 3 algebra,
// the skew product, the Gram-Schmidt on a rotation's rows, the unrolled elimination, the LDS Jacobi, the Sampson residual written out
// in fused multiply-adds, the series of exp([w]x), the de-normalisation (select_kernel, the F
// refinement), and what the refinement kernels run
// alike: the fixed-order block reduction, the damped Cholesky step, (F and H) the Hartley normalisation over the usable matches and
// (host) the checks of their entry points.  No __global__ code and no
// device data: what the RANSAC scoring needs beyond this is ransac_common.h.  DESIGN.md §3.4.
// The floating-point expressions in here are pinned: operand order, the explicit __builtin_fma calls, the bracketing of the sums
// and the order of the butterflies are what the numpy restatements under tests/ repeat bit for bit.
#pragma once
#include "common.h"

namespace roma {
namespace {

constexpr double PIVOT_TOL = 1e-10;
constexpr int JACOBI_SWEEPS = 10;

__device__ __forceinline__ double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

__device__ __forceinline__ void unit_frobenius(double* m) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s += m[i] * m[i];
  const double inv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] *= inv;
}

// [fx s cx; 0 fy cy; 0 0 1]^-1 -> ki = (1/fx, -s/(fx fy), (s cy - cx fy)/(fx fy), 1/fy, -cy/fy); false when not invertible
__device__ __forceinline__ bool invert_k(const double* K, double* ki) {
  const double fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5];
  const double d = fx * fy;
  const bool ok = isfinite(fx) && isfinite(s) && isfinite(cx) && isfinite(fy) && isfinite(cy) && d != 0.0 && isfinite(1.0 / d);
  ki[0] = 1.0 / fx; ki[1] = -s / d; ki[2] = (s * cy - cx * fy) / d; ki[3] = 1.0 / fy; ki[4] = -cy / fy;
  return ok;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// out = [v]x A (3 x 3, row major)
__device__ __forceinline__ void skew_times(const double* v, const double* A, double* out) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[c] = v[1] * A[6 + c] - v[2] * A[3 + c];
    out[3 + c] = v[2] * A[c] - v[0] * A[6 + c];
    out[6 + c] = v[0] * A[3 + c] - v[1] * A[c];
  }
}

// Gram-Schmidt on the rows of X into Rc: r0, r1 made orthogonal to r0, r2 = r0 x r1
__device__ __forceinline__ void orthonormalise_rows(const double* X, double* Rc) {
  const double i0 = 1.0 / sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) Rc[i] = X[i] * i0;
  const double d = Rc[0] * X[3] + Rc[1] * X[4] + Rc[2] * X[5];
#pragma unroll
  for (int i = 0; i < 3; ++i) Rc[3 + i] = X[3 + i] - d * Rc[i];
  const double i1 = 1.0 / sqrt(Rc[3] * Rc[3] + Rc[4] * Rc[4] + Rc[5] * Rc[5]);
#pragma unroll
  for (int i = 0; i < 3; ++i) Rc[3 + i] *= i1;
  cross3(Rc, Rc + 3, Rc + 6);
}

// ------------------------------------------------------------------------------------------------ Hartley normalisation record
// x^ = (x - c) s per image
struct Norm {
  double cxA, cyA, sA, cxB, cyB, sB;
};

// g = c T_A: columns 0,1 scaled by sA, column 2 = -sA (cA . cols 0,1) + col 2
__device__ __forceinline__ void times_t_a(const double* c, const Norm& n, double* g) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = c[3 * r] * n.sA;
    g[3 * r + 1] = c[3 * r + 1] * n.sA;
    g[3 * r + 2] = c[3 * r + 2] - n.sA * (n.cxA * c[3 * r] + n.cyA * c[3 * r + 1]);
  }
}

// o = T_B^T c T_A: an F in pixels from normalised coordinates.  T_B^T g: rows 0,1 scaled by sB, row 2 = -sB (cB . rows 0,1) + row 2
__device__ __forceinline__ void to_pixels(const double* c, const Norm& n, double* o) {
  double g[9];
  times_t_a(c, n, g);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o[j] = n.sB * g[j];
    o[3 + j] = n.sB * g[3 + j];
    o[6 + j] = g[6 + j] - n.sB * (n.cxB * g[j] + n.cyB * g[3 + j]);
  }
}

// ---------------------------------------------------------------------------------------------------------- Sampson residual
// (m x_A)_{0,1,2} and (m^T x_B)_{0,1} for x_A = (x, y, 1), x_B = (u, v, 1); every operation is written out, so the passes that
// use it agree bit for bit
__device__ __forceinline__ void apply_model(const double* m, double x, double y, double u, double v, double* mx, double* mt) {
#pragma unroll
  for (int r = 0; r < 3; ++r) mx[r] = __builtin_fma(m[3 * r], x, __builtin_fma(m[3 * r + 1], y, m[3 * r + 2]));
#pragma unroll
  for (int c = 0; c < 2; ++c) mt[c] = __builtin_fma(m[c], u, __builtin_fma(m[3 + c], v, m[6 + c]));
}

// numerator n and denominator d of the Sampson residual r = n / sqrt d
__device__ __forceinline__ void sampson_terms(const double* ex, const double* et, double u, double v, double& n, double& d) {
  n = __builtin_fma(u, ex[0], __builtin_fma(v, ex[1], ex[2]));
  d = __builtin_fma(ex[0], ex[0], __builtin_fma(ex[1], ex[1], __builtin_fma(et[0], et[0], et[1] * et[1])));
}

// r^2 from n and d, the one expression every pass uses (NaN when d = 0 or the match is not finite: then it is no inlier)
__device__ __forceinline__ double squared_residual(double n, double d, double& isd, double& r) {
  isd = 1.0 / sqrt(d);
  r = n * isd;
  return r * r;
}

// exp([w]x) = I + A [w]x + B [w]x^2: A = sin(th) / th and B = (1 - cos(th)) / th^2 by their series in th2 = th^2, nested, 11 terms:
// exact to rounding for th <= 1, which the callers ensure (libm's sin would cost a spill of scalar registers).  The 20 coefficients
// come from `coef`: So3Literals (immediates, 38 scalar registers where the series sits in a loop) or So3Table (a table, e.g. in
// LDS, that so3_fill_table wrote: the same 20 values)
constexpr int SO3_EXP_TERMS = 10;
constexpr double so3_coef_a(int k) { return 1.0 / (double)((2 * k + 2) * (2 * k + 3)); }
constexpr double so3_coef_b(int k) { return 1.0 / (double)((2 * k + 3) * (2 * k + 4)); }
struct So3Literals {
  __device__ __forceinline__ double a(int k) const { return so3_coef_a(k); }
  __device__ __forceinline__ double b(int k) const { return so3_coef_b(k); }
};
struct So3Table {
  const double* t;                                              // 2 * SO3_EXP_TERMS values
  __device__ __forceinline__ double a(int k) const { return t[k]; }
  __device__ __forceinline__ double b(int k) const { return t[SO3_EXP_TERMS + k]; }
};
__device__ __forceinline__ void so3_fill_table(double* t) {
#pragma unroll
  for (int k = 0; k < SO3_EXP_TERMS; ++k) { t[k] = so3_coef_a(k); t[SO3_EXP_TERMS + k] = so3_coef_b(k); }
}
template <class Coef> __device__ __forceinline__ void so3_exp_series(double th2, double& A, double& B, const Coef& coef) {
  A = 1.0;
  B = 1.0;
#pragma unroll
  for (int k = SO3_EXP_TERMS - 1; k >= 0; --k) {
    A = 1.0 - th2 * coef.a(k) * A;
    B = 1.0 - th2 * coef.b(k) * B;
  }
  B *= 0.5;
}

// ------------------------------------------------------------------------------------------------------- elimination (fp64)
// Forward elimination with partial pivoting of the ROWS x 9 system, fully unrolled (rows are swapped by conditional selects, so
// every index is a compile-time constant and A stays in registers).  Returns false when a pivot fails the relative tolerance.
template <int ROWS> __device__ __forceinline__ bool eliminate(double (&A)[ROWS][9]) {
  double scale = 0.0;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < 9; ++c) scale = fmax(scale, fabs(A[r][c]));
  bool ok = scale > 0.0;
#pragma unroll
  for (int c = 0; c < ROWS; ++c) {
#pragma unroll
    for (int r = c + 1; r < ROWS; ++r) {
      const bool sw = fabs(A[r][c]) > fabs(A[c][c]);
#pragma unroll
      for (int j = c; j < 9; ++j) {
        const double t = A[c][j];
        A[c][j] = sw ? A[r][j] : t;
        A[r][j] = sw ? t : A[r][j];
      }
    }
    const double piv = A[c][c];
    ok = ok && fabs(piv) > PIVOT_TOL * scale;
    const double inv = piv != 0.0 ? 1.0 / piv : 0.0;
#pragma unroll
    for (int r = c + 1; r < ROWS; ++r) {
      const double f = A[r][c] * inv;
#pragma unroll
      for (int j = c + 1; j < 9; ++j) A[r][j] = __builtin_fma(-f, A[c][j], A[r][j]);
    }
  }
  return ok;
}

// x[k] for k < ROWS from the upper-triangular system, with x[ROWS..8] given
template <int ROWS> __device__ __forceinline__ void back_substitute(const double (&A)[ROWS][9], double* x) {
#pragma unroll
  for (int k = ROWS - 1; k >= 0; --k) {
    double s = 0.0;
#pragma unroll
    for (int j = k + 1; j < 9; ++j) s = __builtin_fma(A[k][j], x[j], s);
    x[k] = -s / A[k][k];
  }
}

// --------------------------------------------------------------------------------------------------------------- Jacobi (LDS)
// Cyclic Jacobi on the symmetric n x n matrix A (LDS, leading dimension 9), eigenvectors into the columns of V (LDS, set to the
// identity by the caller).  Lane k < n owns row k; two barriers per rotation.  Every thread of the block calls it.
__device__ void jacobi_lds(double* A, double* V, int n) {
  const int k = threadIdx.x;
  for (int sw = 0; sw < JACOBI_SWEEPS; ++sw) {
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double app = A[p * 9 + p], aqq = A[q * 9 + q], apq = A[p * 9 + q];
        double akp = 0.0, akq = 0.0, vkp = 0.0, vkq = 0.0;
        if (k < n) { akp = A[k * 9 + p]; akq = A[k * 9 + q]; vkp = V[k * 9 + p]; vkq = V[k * 9 + q]; }
        __syncthreads();
        if (apq != 0.0 && k < n) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          if (k == p) {
            A[p * 9 + p] = app - t * apq;
            A[p * 9 + q] = 0.0;
            A[q * 9 + p] = 0.0;
          } else if (k == q) {
            A[q * 9 + q] = aqq + t * apq;
          } else {
            const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
            A[k * 9 + p] = nkp; A[p * 9 + k] = nkp;
            A[k * 9 + q] = nkq; A[q * 9 + k] = nkq;
          }
          V[k * 9 + p] = c * vkp - s * vkq;
          V[k * 9 + q] = s * vkp + c * vkq;
        }
        __syncthreads();
      }
    }
  }
}

// index of the smallest diagonal entry (lowest index on ties)
__device__ __forceinline__ int argmin_diag(const double* A, int n) {
  int j = 0;
  for (int i = 1; i < n; ++i)
    if (A[i * 9 + i] < A[j * 9 + j]) j = i;
  return j;
}

// ------------------------------------------- what the refinement kernels share (pose_refine, fundamental_refine, homography_refine)
// one match in the coordinates of the residual; ok: finite and allowed by mask_in
struct Match {
  double x, y, u, v;
  bool ok;
};

// the K sums of every thread reduced in a fixed order (wave butterfly, then the WAVES waves in order through red, LDS): on return
// every thread holds the same s[]
template <int K, int WAVES, int LD> __device__ __forceinline__ void block_sum(double (&s)[K], double (*red)[LD]) {
  static_assert(K <= LD, "the LDS rows hold K sums");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double acc = red[0][k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) acc += red[w][k];
    s[k] = acc;
  }
  __syncthreads();
}

// match q in pixels; ok: finite and allowed by mask_in (the refinements in pixels: fundamental_refine, homography_refine)
__device__ __forceinline__ Match load_pixels(const double2* __restrict__ xa, const double2* __restrict__ xb,
                                             const unsigned char* mask_in, size_t q) {
  const double2 a = xa[q], b = xb[q];
  Match m;
  m.x = a.x; m.y = a.y; m.u = b.x; m.v = b.y;
  m.ok = isfinite(a.x) && isfinite(a.y) && isfinite(b.x) && isfinite(b.y) && (!mask_in || mask_in[q] != 0);
  return m;
}

// Hartley normalisation of both images over the usable matches (geometry.hip's normalize_kernel, with the mask)
template <int THREADS, int LD>
__device__ __forceinline__ Norm normalisation(const double2* __restrict__ xa, const double2* __restrict__ xb, const unsigned char* mask_in,
                                              size_t base, int N, double (*red)[LD]) {
  double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < N; i += THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    if (m.ok) { c[0] += m.x; c[1] += m.y; c[2] += m.u; c[3] += m.v; c[4] += 1.0; }
  }
  block_sum<5, THREADS / 64>(c, red);
  const double cnt = c[4], inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
  Norm n;
  n.cxA = c[0] * inv; n.cyA = c[1] * inv; n.cxB = c[2] * inv; n.cyB = c[3] * inv;
  double d[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < N; i += THREADS) {
    const Match m = load_pixels(xa, xb, mask_in, base + i);
    if (m.ok) {
      const double ax = m.x - n.cxA, ay = m.y - n.cyA, bx = m.u - n.cxB, by = m.v - n.cyB;
      d[0] += sqrt(ax * ax + ay * ay);
      d[1] += sqrt(bx * bx + by * by);
    }
  }
  block_sum<2, THREADS / 64>(d, red);
  const double mdA = d[0] * inv, mdB = d[1] * inv;
  n.sA = 1.4142135623730951 / mdA;
  n.sB = 1.4142135623730951 / mdB;
  if (!(mdA > 0.0) || !isfinite(n.sA)) n.sA = 1.0;
  if (!(mdB > 0.0) || !isfinite(n.sB)) n.sB = 1.0;
  return n;
}

// delta of (A + lambda diag A) delta = -g by a Cholesky in registers; tri: the upper triangle of A row by row, g: J^T r.  False
// on a pivot that is not positive (NaN included)
template <int NPAR> __device__ __forceinline__ bool solve_step(const double* tri, const double* g, double lambda, double (&delta)[NPAR]) {
  double L[NPAR][NPAR];
  int o = 0;
#pragma unroll
  for (int a = 0; a < NPAR; ++a)
#pragma unroll
    for (int b = a; b < NPAR; ++b) {
      const double v = tri[o++];
      L[b][a] = a == b ? v + lambda * v : v;               // lower triangle, overwritten by the factor
    }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NPAR; ++j) {
    double p = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    ok = ok && p > 0.0 && isfinite(p);
    const double dj = sqrt(p), inv = 1.0 / dj;
    L[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < NPAR; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v * inv;
    }
  }
  double y[NPAR];
#pragma unroll
  for (int i = 0; i < NPAR; ++i) {
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = NPAR - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < NPAR; ++k) v -= L[k][i] * delta[k];
    delta[i] = v / L[i][i];
  }
  return ok;
}

// host: what the entry points of the refinements check alike (fn names the entry point in the message)
inline int check_refine(const char* fn, const void* xa, const void* xb, int P, int N, int min_matches, double threshold, int iters) {
  ROMA_REQUIRE(P >= 1 && P <= (1 << 24), ROMA_E_SHAPE, "%s: bad shape P=%d", fn, P);
  ROMA_REQUIRE(N >= min_matches && N <= (1 << 26), ROMA_E_SHAPE, "%s: N=%d matches, need at least %d", fn, N, min_matches);
  ROMA_REQUIRE(threshold > 0.0 && threshold < 1e18, ROMA_E_ARG, "%s: threshold must be positive, got %g", fn, threshold);
  ROMA_REQUIRE(iters >= 0 && iters <= (1 << 16), ROMA_E_ARG, "%s: iters must be in [0, 65536], got %d", fn, iters);
  ROMA_REQUIRE(aligned16(xa) && aligned16(xb), ROMA_E_ALIGN, "%s: xa and xb must be 16-byte aligned", fn);
  return 0;
}

}  // namespace
}  // namespace roma
