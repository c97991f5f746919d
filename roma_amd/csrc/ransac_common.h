// What the RANSAC translation units share (geometry.hip: F / H, essential.hip: E, absolute_pose.hip, similarity.hip) on top of the
// fp64 helpers of twoview_math.h.  Device: the counter-hash of the sample draw and, where it compiles to the written-out loop,
// the draw itself (draw_sample); fp32 scoring of every slot (score_kernel / reduce_kernel, no atomics; MSAC, or MAGSAC++ by the
// loss and weight tables of magsac_table.h; absolute pose and similarity have score kernels of their own around their point error,
// and all four use reduce_kernel); the block-wide re-score of every select kernel (block_cost).  Host: the workspace layout and
// the typed pointers to its nine common regions, the stream of a call's draw with the stage of each estimator, the grids, the
// choice of a kernel's MSAC or MAGSAC++ instance and the argument checks of the entry points.  geometry.hip's header pins the draw
// and the tolerances.  DESIGN.md §3.4.
// The refinement kernels (pose_refine.hip, fundamental_refine.hip, homography_refine.hip) score nothing and include twoview_math.h
// alone.
#pragma once
#include "magsac_table.h"
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int KIND_F = 0, KIND_H = 1;
constexpr int CHUNK = 1024;             // points per scoring workgroup (the slab's chunk)
constexpr double COLLINEAR_TOL = 1e-6;

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// The sample draw (geometry.hip's header pins it): S distinct usable indices for sample h of pair `pair`, the pair's index in the
// whole call; ok = all S were found.  usable(i): point i may be sampled.  Used where it compiles to the written-out loop
// (p3p_kernel, sim_solve_kernel); minimal_kernel and five_point_kernel keep that loop (profiles/ransac_shared_code_isa.txt).
template <int S, typename Usable>
__device__ __forceinline__ void draw_sample(uint32_t stream, uint32_t pair, int iters, int h, int N, Usable usable, int* idx, bool& ok) {
  ok = true;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const uint32_t ctr = ((pair * (uint32_t)iters + (uint32_t)h) * 8u + (uint32_t)k);
    int got = -1;
    for (uint32_t att = 0; att < 16; ++att) {
      const uint32_t hs = fmix32(stream + ctr * 0x9E3779B1u + att * 0x7FEB352Du);
      const int i = (int)(((uint64_t)hs * (uint64_t)(uint32_t)N) >> 32);
      bool good = usable(i);
#pragma unroll
      for (int j = 0; j < k; ++j) good = good && idx[j] != i;
      if (good) { got = i; break; }
    }
    idx[k] = got;
    ok = ok && got >= 0;
  }
}

template <int KIND> struct Kind;
template <> struct Kind<KIND_F> { static constexpr int S = 7, R = 3, LO_MIN = 8; };
template <> struct Kind<KIND_H> { static constexpr int S = 4, R = 1, LO_MIN = 4; };

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

// The workspace of one call: the nine regions every estimator has, then `n_extra` of its own; each is rounded up to 256 bytes.
// S = points per sample, R = slots per sample.  off (may be null) gets the 9 + n_extra offsets; returns the size in bytes.
constexpr int WS_NORM = 0, WS_PTS = 1, WS_SAMPLES = 2, WS_MODELS = 3, WS_VALID = 4, WS_SLAB_COST = 5, WS_SLAB_CNT = 6,
              WS_COST = 7, WS_COUNT = 8, WS_N = 9;
inline long ws_layout(long S, long R, int P, int N, int iters, const long* extra, int n_extra, long* off) {
  const long M = (long)iters * R, C = (N + CHUNK - 1) / CHUNK;
  const long bytes[WS_N] = {(long)P * 8 * 8, (long)P * N * 16, (long)P * iters * S * 4, (long)P * M * 72, (long)P * M * 4,
                            (long)P * C * M * 4, (long)P * C * M * 4, (long)P * M * 8, (long)P * M * 4};
  long o = 0;
  for (int i = 0; i < WS_N + n_extra; ++i) {
    if (off) off[i] = o;
    o += ((i < WS_N ? bytes[i] : extra[i - WS_N]) + 255) / 256 * 256;
  }
  return o;
}
inline int check_shape(const char* fn, int P, int N, int iters, int smin) {
  ROMA_REQUIRE(P >= 1 && P <= 65535 && iters >= 1 && iters <= (1 << 24), ROMA_E_SHAPE, "%s: bad shape P=%d iters=%d", fn, P, iters);
  ROMA_REQUIRE(N >= smin && N <= (1 << 26), ROMA_E_SHAPE, "%s: N=%d matches, need at least %d for the minimal sample", fn, N, smin);
  return 0;
}
inline int check_workspace(const char* fn, long ws_bytes, long need) {
  ROMA_REQUIRE(ws_bytes >= need, ROMA_E_ARG, "%s: workspace of %ld bytes, need %ld", fn, ws_bytes, need);
  return 0;
}
inline int check_threshold(const char* fn, float threshold) {
  ROMA_REQUIRE(threshold > 0.f && threshold < 1e18f, ROMA_E_ARG, "%s: threshold must be positive, got %g", fn, (double)threshold);
  return 0;
}
// The checks of a *_hypotheses / *_select entry point behind its null-pointer test, in the order of essential.hip, absolute_pose.hip
// and similarity.hip: shape, the solver's grid (per_block samples per workgroup), threshold.  geometry.hip checks the workspace
// before the threshold and has no grid limit, so it calls the pieces itself.
inline int check_problem(const char* fn, int P, int N, int iters, int smin, int per_block, float threshold) {
  const int rc = check_shape(fn, P, N, iters, smin);
  if (rc) return rc;
  ROMA_REQUIRE(((long)P * iters + per_block - 1) / per_block <= 0x7FFFFFFFL, ROMA_E_SHAPE, "%s: P * iters = %ld samples in one call", fn,
               (long)P * iters);
  return check_threshold(fn, threshold);
}
// ... and the last check of each: the pair offset of *_hypotheses, the rounds of *_select
inline int check_pair_offset(const char* fn, int p0) {
  ROMA_REQUIRE(p0 >= 0, ROMA_E_ARG, "%s: negative pair offset %d", fn, p0);
  return 0;
}
inline int check_lo_iters(const char* fn, int lo_iters) {
  ROMA_REQUIRE(lo_iters >= 0, ROMA_E_ARG, "%s: negative lo_iters %d", fn, lo_iters);
  return 0;
}

// The nine common regions of a workspace as typed pointers, from ws_layout's offsets.  *_select only reads through them.
struct Regions {
  double* norm;
  float4* pts;
  int* samples;
  double* models;
  int* valid;
  float* slab_cost;
  int* slab_cnt;
  double* cost;
  int* count;
};
inline Regions regions(const void* ws, const long* off) {
  char* w = static_cast<char*>(const_cast<void*>(ws));
  return {(double*)(w + off[WS_NORM]),      (float4*)(w + off[WS_PTS]),     (int*)(w + off[WS_SAMPLES]),
          (double*)(w + off[WS_MODELS]),    (int*)(w + off[WS_VALID]),      (float*)(w + off[WS_SLAB_COST]),
          (int*)(w + off[WS_SLAB_CNT]),     (double*)(w + off[WS_COST]),    (int*)(w + off[WS_COUNT])};
}
template <typename T> inline T* region(const void* ws, const long* off, int i) {      // an estimator's own region
  return (T*)(static_cast<char*>(const_cast<void*>(ws)) + off[i]);
}

// The stream of a call's draw (geometry.hip's header): one stage per estimator, so that no two draw the same samples from one seed
constexpr uint32_t STAGE_F = 2u, STAGE_H = 3u, STAGE_E = 4u, STAGE_AP = 5u, STAGE_SIM = 6u;
inline uint32_t sample_stream(unsigned seed, uint32_t stage) { return fmix32((uint32_t)seed ^ (stage * 0x9E3779B9u)); }

// The grids of one *_hypotheses call: the minimal solver (per_block samples per workgroup), the scoring (256 slots x one chunk x one
// pair per workgroup) and the reduction (256 slots per workgroup).  R = slots per sample.
struct Grids { dim3 solve, score, reduce; };
inline Grids ransac_grids(int P, int N, int iters, int R, int per_block) {
  const long nt = (long)P * iters, M = (long)iters * R;
  return {dim3((unsigned)((nt + per_block - 1) / per_block)), dim3((unsigned)((M + 255) / 256), (unsigned)((N + CHUNK - 1) / CHUNK), (unsigned)P),
          dim3((unsigned)((P * M + 255) / 256))};
}

// kernel<..., SCORE_MSAC> or kernel<..., SCORE_MAGSAC>: the caller names both instances, `scoring` (checked) picks
template <typename K> inline K by_scoring(int scoring, K msac, K magsac) { return scoring == SCORE_MAGSAC ? magsac : msac; }

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

// Cost (fp32 errors, fp64 sum in a fixed tree) and inlier count of one model over the pair's N points, by the 256 threads of a
// block: err(i) = squared error of point i under it.  The re-score of every select kernel.
template <int SCORE, typename Err>
__device__ __forceinline__ void block_cost(int N, float t2, Err err, double* dred, int* ired, double& cost, int& cnt) {
  const int tid = threadIdx.x;
  double c = 0.0;
  int n = 0;
  for (int i = tid; i < N; i += 256) {
    const float e = err(i);
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

// ... of the model in LDS `mdl` (F, H, E)
template <int KIND, int SCORE>
__device__ void block_score(const double* mdl, const float4* pq, int N, float ka, float kb, float t2, double* dred, int* ired,
                            double& cost, int& cnt) {
  float m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = (float)mdl[i];
  block_cost<SCORE>(N, t2, [&](int i) { return point_error<KIND>(m, pq[i], ka, kb); }, dred, ired, cost, cnt);
}

}  // namespace
}  // namespace roma
