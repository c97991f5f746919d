// What the RANSAC translation units share (geometry.hip: F / H, essential.hip: E): the counter-hash of the sample draw, the
// fully unrolled fp64 elimination, fp32 scoring of every slot (score_kernel / reduce_kernel, no atomics; MSAC, or MAGSAC++ by the
// loss and weight tables of magsac_table.h), the block-wide re-score and the LDS Jacobi of the select kernels.  geometry.hip's
// header pins the draw and the tolerances.  DESIGN.md §3.4.
// Plus what the refinement kernels share (pose_refine.hip, fundamental_refine.hip): the Sampson residual written out in fused
// multiply-adds and the series of exp([w]x).
#pragma once
#include "common.h"
#include "magsac_table.h"

namespace roma {
namespace {

constexpr int KIND_F = 0, KIND_H = 1;
constexpr int CHUNK = 1024;             // points per scoring workgroup (the slab's chunk)
constexpr double PIVOT_TOL = 1e-10;
constexpr double COLLINEAR_TOL = 1e-6;
constexpr int JACOBI_SWEEPS = 10;

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

template <int KIND> struct Kind;
template <> struct Kind<KIND_F> { static constexpr int S = 7, R = 3, LO_MIN = 8; };
template <> struct Kind<KIND_H> { static constexpr int S = 4, R = 1, LO_MIN = 4; };

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

// ------------------------------------------------------------------ what the refinement kernels share (pose_refine, fundamental_refine)
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

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

// --------------------------------------------------------------------------------------------------------------- scoring (fp32)
// Squared error in pixels of one normalised point (xa, ya, xb, yb) under a normalised model m.  F: Sampson error, with
// ka = sA^2, kb = sB^2.  H: forward transfer error, with kb = 1 / sB^2 (ka unused).  NaN / inf -> not an inlier.
template <int KIND>
__device__ __forceinline__ float point_error(const float* m, float4 q, float ka, float kb) {
  if constexpr (KIND == KIND_F) {
    const float fx0 = __builtin_fmaf(m[0], q.x, __builtin_fmaf(m[1], q.y, m[2]));
    const float fx1 = __builtin_fmaf(m[3], q.x, __builtin_fmaf(m[4], q.y, m[5]));
    const float fx2 = __builtin_fmaf(m[6], q.x, __builtin_fmaf(m[7], q.y, m[8]));
    const float ft0 = __builtin_fmaf(m[0], q.z, __builtin_fmaf(m[3], q.w, m[6]));
    const float ft1 = __builtin_fmaf(m[1], q.z, __builtin_fmaf(m[4], q.w, m[7]));
    const float num = __builtin_fmaf(q.z, fx0, __builtin_fmaf(q.w, fx1, fx2));
    const float den = __builtin_fmaf(kb, __builtin_fmaf(fx0, fx0, fx1 * fx1), ka * __builtin_fmaf(ft0, ft0, ft1 * ft1));
    return num * num / den;
  } else {
    const float hx = __builtin_fmaf(m[0], q.x, __builtin_fmaf(m[1], q.y, m[2]));
    const float hy = __builtin_fmaf(m[3], q.x, __builtin_fmaf(m[4], q.y, m[5]));
    const float hw = __builtin_fmaf(m[6], q.x, __builtin_fmaf(m[7], q.y, m[8]));
    const float iw = 1.0f / hw;
    const float dx = __builtin_fmaf(-hx, iw, q.z), dy = __builtin_fmaf(-hy, iw, q.w);
    return __builtin_fmaf(dx, dx, dy * dy) * kb;
  }
}

template <int KIND> __device__ __forceinline__ void error_scales(const double* nrm, float& ka, float& kb) {
  const double sA = nrm[2], sB = nrm[6];
  ka = (float)(sA * sA);
  kb = KIND == KIND_F ? (float)(sB * sB) : (float)(1.0 / (sB * sB));
}

// MAGSAC++ scoring: loss L and IRLS weight W of u = e / threshold^2 are the piecewise-linear interpolants of the
// nodes of magsac_table.h.  A cell is {node, next node - node} (one fp32 subtraction); static device data, nothing is copied in a call.
constexpr int SCORE_MSAC = 0, SCORE_MAGSAC = 1;
struct MagsacCell { float v, s; };
struct MagsacCells { MagsacCell c[MAGSAC_CELLS]; };
constexpr MagsacCells magsac_cells(const float (&t)[MAGSAC_NODES]) {
  MagsacCells r{};
  for (int i = 0; i < MAGSAC_CELLS; ++i) { r.c[i].v = t[i]; r.c[i].s = t[i + 1] - t[i]; }
  return r;
}
__device__ const MagsacCells magsac_loss_cells = magsac_cells(MAGSAC_LOSS);
__device__ const MagsacCells magsac_weight_cells = magsac_cells(MAGSAC_WEIGHT);

// f = e * (1024 / threshold^2) -> cell i = min((int)f, 1023), fraction f - i; the caller has checked e < threshold^2
__device__ __forceinline__ int magsac_cell(float e, float scale, float& frac) {
  const float f = e * scale;
  const int i = min((int)f, MAGSAC_CELLS - 1);
  frac = f - (float)i;
  return i;
}
__device__ __forceinline__ float magsac_lookup(const MagsacCells& tab, float e, float scale) {
  float frac;
  const MagsacCell c = tab.c[magsac_cell(e, scale, frac)];
  return __builtin_fmaf(frac, c.s, c.v);
}

// host: what the entry points and their *_ex forms share (fn names the entry point in the message)
inline int check_scoring(const char* fn, int scoring) {
  ROMA_REQUIRE(scoring == SCORE_MSAC || scoring == SCORE_MAGSAC, ROMA_E_ARG, "%s: scoring must be 0 (MSAC) or 1 (MAGSAC), got %d", fn,
               scoring);
  return 0;
}
inline int check_launch(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", fn, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// slab_cost / slab_cnt: (P, S, M) with M = iters * R slots and S = ceil(N / CHUNK) chunks.  SCORE_MAGSAC: the partial cost is
// threshold^2 * (outliers of the chunk + sum of L over its inliers).  The loss nodes 0..1023 sit in LDS beside the points (4 KB: with
// 8 KB of cells a fifth of the workgroups would no longer fit a CU); node 1024 is L(1) = 1.
template <int KIND, int SCORE>
__global__ __launch_bounds__(256) void score_kernel(const float4* __restrict__ pts, const double* __restrict__ norm,
                                                    const double* __restrict__ models, const int* __restrict__ valid, int N, int M,
                                                    float t2, float* __restrict__ slab_cost, int* __restrict__ slab_cnt) {
  __shared__ float4 sp[CHUNK];
  __shared__ float sl[SCORE == SCORE_MAGSAC ? MAGSAC_CELLS : 1];
  const int p = blockIdx.z, s = blockIdx.y, S = gridDim.y;
  const int i0 = s * CHUNK, n = min(CHUNK, N - i0);
  const float4* src = pts + (size_t)p * N + i0;
  for (int i = threadIdx.x; i < n; i += 256) sp[i] = src[i];
  if constexpr (SCORE == SCORE_MAGSAC)
    for (int i = threadIdx.x; i < MAGSAC_CELLS; i += 256) sl[i] = magsac_loss_cells.c[i].v;
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  float cost = 0.f;
  int cnt = 0;
  if (valid[slot]) {
    float md[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) md[i] = (float)models[slot * 9 + i];
    float ka, kb;
    error_scales<KIND>(norm + p * 8, ka, kb);
    if constexpr (SCORE == SCORE_MSAC) {
      for (int j = 0; j < n; ++j) {
        const float e = point_error<KIND>(md, sp[j], ka, kb);
        const bool in = e < t2;
        cnt += in ? 1 : 0;
        cost += in ? e : t2;
      }
    } else {
      const float scale = (float)MAGSAC_CELLS / t2;
      for (int j = 0; j < n; ++j) {
        const float e = point_error<KIND>(md, sp[j], ka, kb);
        if (e < t2) {                                               // most slot x point pairs are outliers: no lookup
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

__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ slab_cost, const int* __restrict__ slab_cnt,
                                                     const int* __restrict__ valid, int P, int M, int S, double* __restrict__ cost,
                                                     int* __restrict__ count) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)P * M) return;
  const int p = (int)(t / M), m = (int)(t % M);
  double c = 0.0;
  int n = 0;
  for (int s = 0; s < S; ++s) {
    const size_t o = ((size_t)p * S + s) * M + m;
    c += (double)slab_cost[o];
    n += slab_cnt[o];
  }
  const bool v = valid[t] != 0;
  cost[t] = v ? c : INFINITY;
  count[t] = v ? n : 0;
}

// ---------------------------------------------------------------------------------------------- selection + local optimisation
// Cost (fp32 errors, fp64 sum in a fixed tree) and inlier count of the model in LDS `mdl` over the pair's N points.
template <int KIND, int SCORE>
__device__ void block_score(const double* mdl, const float4* pq, int N, float ka, float kb, float t2, double* dred, int* ired,
                            double& cost, int& cnt) {
  const int tid = threadIdx.x;
  float m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = (float)mdl[i];
  double c = 0.0;
  int n = 0;
  for (int i = tid; i < N; i += 256) {
    const float e = point_error<KIND>(m, pq[i], ka, kb);
    const bool in = e < t2;
    n += in ? 1 : 0;
    if constexpr (SCORE == SCORE_MSAC) c += (double)(in ? e : t2);
    else c += (double)(in ? magsac_lookup(magsac_loss_cells, e, (float)MAGSAC_CELLS / t2) : 1.f);
  }
  if constexpr (SCORE == SCORE_MAGSAC) c *= (double)t2;
  dred[tid] = c;
  ired[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { dred[tid] += dred[tid + o]; ired[tid] += ired[tid + o]; }
    __syncthreads();
  }
  cost = dred[0];
  cnt = ired[0];
  __syncthreads();
}

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

}  // namespace
}  // namespace roma
