// Point-cloud rendering: a z-buffered splat of N points into the depth maps of V posed views (1 <= V <= 32) and, per point, the views that
// see it — the first consumer of what fuse_depth_maps leaves.  DESIGN.md §3.4, "Point-cloud rendering"; tests/render_points_ref.py
// restates the definition in numpy.
//
// Convention (depth_fuse.hip): x_v ~ K_v (R_v X + t_v); pixel (row i, column j) covers [j, j+1) x [i, i+1).  All views share one map
// shape (H, W).  A view is usable when K is upper triangular with fx fy k22 != 0 and K, R, t are finite; a point is live when its three
// coordinates are finite and its mask byte (where a mask is given) is not 0.
//
// Four launches on the caller's stream:
//   clear     thread per word: the V H W keys to all ones, the four counts to 0.
//   splat     grid (ceil(N / 1024), V), 256 threads, four points per thread one after the other.  The view is a grid dimension, so P_v
//     = K_v [R_v | t_v] is formed once per workgroup (thread 0, into LDS) and is uniform over it.  A live point that projects inside the
//     map (project_point below) makes key = bits(z32) << 32 | n — a positive float orders as its bit pattern — and applies a 64-bit
//     unsigned atomicMin of it to every pixel of its (2 radius + 1)^2 footprint that lies inside the map.  Before each atomic the word is
//     read with a plain load and the atomic is skipped when key >= what was read: the word only ever decreases, so a stale read can
//     cost an atomic and can never lose a winner.  The winner of a pixel is the nearest point and, on exactly equal z32, the lowest
//     index, whatever order the points arrive in.
//   resolve   16 pixels per thread: depth = the winner's z32, index = its n; 0.0f and -1 where nothing was drawn.
//   visible   four points per thread, every P_v in LDS (3 KB): over the usable views in ascending order the same projection by the same
//     function, bit v set when (double) z32 <= (double) depth[v, i, j] (1 + depth_tol) at the point's own pixel.
// counts: covered pixels (resolve); projections inside a map, set bits and points that are not live (visible, which runs every
// projection of the splat again).  Each block sums — ballots and popcounts, a wave butterfly for the per-lane sums, the waves through
// LDS — and adds once per count with an INTEGER atomicAdd.  Integer adds commute, so the values are the same from run to run, as are
// the maps: an unsigned min commutes too.  No float atomics.  All blocks add to the same four words, and such adds go through one at a
// time: with a block per 256 pixels and points they were most of resolve's and visibility's time, hence the fatter blocks and no
// count in the splat ("what was tried").
//
// A block never waits for another: what a launch needs from an earlier one is ordered by the stream.  Every loop has a trip count fixed
// by (N, V, H, W, radius); every __syncthreads is reached by the whole block (the one early return, of an unusable view's blocks in the
// splat, is uniform over the block and comes before the first barrier).
//
// Same bits in both kernels.  P_v and the projection are written with explicit fma() under `fp contract(off)`, so the splat and the
// visibility kernel round identically whatever the compiler would have fused in either: the pixel a point is tested at is the pixel it
// was drawn into.  Addressing as sample_depth of depth_fuse.hip: a projection may be NaN, inf or 1e30, so it is range-checked IN
// FLOATING POINT by a negated conjunction (NaN fails it) before anything becomes an integer, and the integers are checked again.
#pragma clang fp contract(off)
#include "multiview.h"

#include <climits>

namespace roma {
namespace {

constexpr int THREADS = 256, ITEMS = 4, POINTS_PER_BLOCK = THREADS * ITEMS, WAVES = THREADS / 64;
constexpr int PIXEL_ITEMS = 16, PIXELS_PER_BLOCK = THREADS * PIXEL_ITEMS;
constexpr int MAX_SIDE = 32768, MAX_RADIUS = 4;
constexpr unsigned long long EMPTY = ~0ull;

struct RenderParams {
  long N;
  int V, H, W, radius;
  double lim;                      // 1 + depth_tol
};

// all of K, R, t finite, K upper triangular, fx fy k22 != 0 (with a finite reciprocal, as depth_fuse.hip's view_constants)
__device__ __forceinline__ bool usable_view(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t) {
  bool ok = upper_triangular(K);
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && isfinite(K[i]) && isfinite(R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) ok = ok && isfinite(t[i]);
  const double det = K[0] * K[4] * K[8];
  return ok && det != 0.0 && isfinite(1.0 / det);
}

// P = K [R | t], row major 3 x 4; one thread forms all twelve entries, in both kernels by this code
__device__ __forceinline__ void view_matrix(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t, double* P) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) P[4 * i + j] = fma(K[3 * i + 2], R[6 + j], fma(K[3 * i + 1], R[3 + j], K[3 * i] * R[j]));
    P[4 * i + 3] = fma(K[3 * i + 2], t[2], fma(K[3 * i + 1], t[1], K[3 * i] * t[0]));
  }
}

// the pixel (i, j) and the fp32 depth of a point in a view; false where it is not drawn
__device__ __forceinline__ bool project_point(const double* P, float x, float y, float z, int H, int W, int& i, int& j, float& z32) {
  const double X = (double)x, Y = (double)y, Z = (double)z;
  const double qx = fma(P[2], Z, fma(P[1], Y, fma(P[0], X, P[3])));
  const double qy = fma(P[6], Z, fma(P[5], Y, fma(P[4], X, P[7])));
  const double qz = fma(P[10], Z, fma(P[9], Y, fma(P[8], X, P[11])));
  if (!(qz > 0.0 && isfinite(qx) && isfinite(qy) && isfinite(qz))) return false;
  const double iz = 1.0 / qz;
  const double u = qx * iz, w = qy * iz;
  if (!(u >= 0.0 && u < (double)W && w >= 0.0 && w < (double)H)) return false;
  z32 = (float)qz;
  if (!(z32 > 0.f && z32 <= 3.402823466e+38f)) return false;
  j = (int)floor(u);
  i = (int)floor(w);
  return j >= 0 && j < W && i >= 0 && i < H;
}

__device__ __forceinline__ bool load_point(const float* __restrict__ points, const unsigned char* __restrict__ mask, long n, long N, float& x,
                                           float& y, float& z) {
  if (n >= N) return false;
  x = points[3 * (size_t)n];
  y = points[3 * (size_t)n + 1];
  z = points[3 * (size_t)n + 2];
  const bool on = mask ? mask[n] != 0 : true;
  return on && isfinite(x) && isfinite(y) && isfinite(z);
}

// the block's sum of wave-uniform per-wave counts, added to *out once; every thread of the block calls it (one barrier)
__device__ __forceinline__ void block_add(unsigned mine, unsigned* s_n, int* out) {
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_n[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) n += s_n[w];
    if (n) atomicAdd(out, (int)n);
  }
}

// -------------------------------------------------------------------------------------------------------------- clear
__global__ __launch_bounds__(THREADS) void render_clear_kernel(long words, unsigned long long* __restrict__ keys, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i < words) keys[i] = EMPTY;
  if (i < 4) counts[i] = 0;
}

// -------------------------------------------------------------------------------------------------------------- splat
__global__ __launch_bounds__(THREADS) void render_splat_kernel(RenderParams prm, const float* __restrict__ points,
                                                               const unsigned char* __restrict__ mask, const double* __restrict__ K,
                                                               const double* __restrict__ R, const double* __restrict__ t,
                                                               unsigned long long* keys) {
  __shared__ double s_P[12];
  const int v = blockIdx.y, tid = threadIdx.x, H = prm.H, W = prm.W, rad = prm.radius;
  if (!usable_view(K + 9 * v, R + 9 * v, t + 3 * v)) return;     // uniform over the block, before the first barrier
  if (tid == 0) view_matrix(K + 9 * v, R + 9 * v, t + 3 * v, s_P);
  __syncthreads();
  unsigned long long* map = keys + (size_t)v * (size_t)H * (size_t)W;
  const long n0 = (long)blockIdx.x * POINTS_PER_BLOCK + tid;
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {
    const long n = n0 + (long)it * THREADS;
    float x, y, z, z32;
    int i, j;
    if (!(load_point(points, mask, n, prm.N, x, y, z) && project_point(s_P, x, y, z, H, W, i, j, z32))) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z32) << 32) | (unsigned long long)(unsigned)n;
    for (int di = -rad; di <= rad; ++di) {
      const int ii = i + di;
      if (ii < 0 || ii >= H) continue;
      for (int dj = -rad; dj <= rad; ++dj) {
        const int jj = j + dj;
        if (jj < 0 || jj >= W) continue;
        unsigned long long* p = map + (size_t)ii * (size_t)W + (size_t)jj;
        if (key < *p) atomicMin(p, key);
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- resolve
__global__ __launch_bounds__(THREADS) void render_resolve_kernel(long words, const unsigned long long* __restrict__ keys,
                                                                 float* __restrict__ depth, int* __restrict__ index, int* __restrict__ counts) {
  __shared__ unsigned s_n[WAVES];
  const long p0 = (long)blockIdx.x * PIXELS_PER_BLOCK + threadIdx.x;
  unsigned n_cov = 0;                                            // wave-uniform
#pragma unroll 4
  for (int it = 0; it < PIXEL_ITEMS; ++it) {                     // no break: every lane takes part in the ballot
    const long p = p0 + (long)it * THREADS;
    bool covered = false;
    if (p < words) {
      const unsigned long long key = keys[p];
      covered = key != EMPTY;
      depth[p] = covered ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
      index[p] = covered ? (int)(unsigned)(key & 0xffffffffull) : -1;
    }
    n_cov += (unsigned)__popcll(__ballot(covered));
  }
  block_add(n_cov, s_n, counts + 1);
}

// -------------------------------------------------------------------------------------------------------------- visible
__global__ __launch_bounds__(THREADS) void render_visible_kernel(RenderParams prm, const float* __restrict__ points,
                                                                 const unsigned char* __restrict__ mask, const double* __restrict__ K,
                                                                 const double* __restrict__ R, const double* __restrict__ t,
                                                                 const float* __restrict__ depth, int* __restrict__ visible,
                                                                 unsigned char* __restrict__ num_views, int* __restrict__ counts) {
  __shared__ double s_P[MAX_VIEWS][12];
  __shared__ int s_ok[MAX_VIEWS];
  __shared__ unsigned s_n[3][WAVES];
  const int tid = threadIdx.x, V = prm.V, H = prm.H, W = prm.W;
  if (tid < V) {
    s_ok[tid] = usable_view(K + 9 * tid, R + 9 * tid, t + 3 * tid) ? 1 : 0;
    view_matrix(K + 9 * tid, R + 9 * tid, t + 3 * tid, s_P[tid]);
  }
  __syncthreads();
  const long n0 = (long)blockIdx.x * POINTS_PER_BLOCK + tid;
  unsigned inside = 0, bits = 0, dead = 0;                       // per lane, per lane, wave-uniform
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {                           // no break: every lane takes part in the ballot
    const long n = n0 + (long)it * THREADS;
    float x = 0.f, y = 0.f, z = 0.f;
    const bool live = load_point(points, mask, n, prm.N, x, y, z);
    unsigned seen = 0;
    if (live) {
#pragma unroll 1
      for (int v = 0; v < V; ++v) {
        if (!s_ok[v]) continue;
        int i, j;
        float z32;
        if (!project_point(s_P[v], x, y, z, H, W, i, j, z32)) continue;
        ++inside;
        const float d = depth[((size_t)v * (size_t)H + (size_t)i) * (size_t)W + (size_t)j];
        if ((double)z32 <= (double)d * prm.lim) seen |= 1u << v;
      }
    }
    if (n < prm.N) {
      visible[n] = (int)seen;
      num_views[n] = (unsigned char)__popc(seen);
    }
    bits += (unsigned)__popc(seen);
    dead += (unsigned)__popcll(__ballot(n < prm.N && !live));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inside += __shfl_xor(inside, o, 64);
    bits += __shfl_xor(bits, o, 64);
  }
  block_add(inside, s_n[0], counts + 0);
  block_add(bits, s_n[1], counts + 2);
  block_add(dead, s_n[2], counts + 3);
}

// host: 0, or a negative code with the error set
int check_shape(const char* fn, int V, int H, int W) {
  ROMA_REQUIRE(V >= 1 && V <= MAX_VIEWS, ROMA_E_SHAPE, "%s: bad shape V=%d (1 to %d views)", fn, V, MAX_VIEWS);
  ROMA_REQUIRE(H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE, ROMA_E_SHAPE, "%s: bad shape maps of %dx%d (sides 1 to %d)", fn, H, W,
               MAX_SIDE);
  ROMA_REQUIRE((long)V * H * W <= (long)INT_MAX, ROMA_E_SHAPE, "%s: bad shape: %d maps of %dx%d have more than 2^31 - 1 pixels in all", fn, V,
               H, W);
  return 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_render_points_workspace(int V, int H, int W, long* out_bytes) {
  if (const int rc = check_shape("roma_render_points_workspace", V, H, W)) return rc;
  const long bytes[1] = {8L * V * H * W};
  long off[1];
  const long total = layout_regions(bytes, 1, off);
  if (out_bytes) out_bytes[0] = total;
  return total;
}

extern "C" int roma_render_points(const float* points, const unsigned char* mask, long N, const double* K, const double* R, const double* t,
                                  int V, int H, int W, int radius, double depth_tol, float* depth, int* index, int* visible,
                                  unsigned char* num_views, int* counts, void* workspace, long workspace_bytes, void* stream) {
  ROMA_REQUIRE(points && K && R && t, ROMA_E_ARG, "roma_render_points: null pointer");
  ROMA_REQUIRE(depth && index && visible && num_views && counts && workspace, ROMA_E_ARG,
               "roma_render_points: null pointer (every output and the workspace are required)");
  if (const int rc = check_shape("roma_render_points", V, H, W)) return rc;
  ROMA_REQUIRE(N >= 1 && N <= (long)INT_MAX, ROMA_E_SHAPE, "roma_render_points: bad shape N=%ld (1 to 2^31 - 1 points)", N);
  ROMA_REQUIRE(radius >= 0 && radius <= MAX_RADIUS, ROMA_E_ARG, "roma_render_points: radius must be in [0, %d], got %d", MAX_RADIUS, radius);
  ROMA_REQUIRE(depth_tol >= 0.0 && depth_tol <= 1.7976931348623157e308, ROMA_E_ARG,
               "roma_render_points: depth_tol must be finite and not negative, got %g", depth_tol);
  ROMA_REQUIRE(aligned4(points), ROMA_E_ALIGN, "roma_render_points: points must be 4-byte aligned");
  const long words = (long)V * H * W;
  const long bytes[1] = {8 * words};
  const long need = layout_regions(bytes, 1, nullptr);
  ROMA_REQUIRE(workspace_bytes >= need, ROMA_E_ARG, "roma_render_points: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  ROMA_REQUIRE(aligned16(workspace), ROMA_E_ALIGN, "roma_render_points: the workspace must be 16-byte aligned");
  RenderParams prm;
  prm.N = N; prm.V = V; prm.H = H; prm.W = W; prm.radius = radius;
  prm.lim = 1.0 + depth_tol;
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned point_blocks = (unsigned)((N + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK);
  hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)((words + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, words, keys, counts);
  hipLaunchKernelGGL(render_splat_kernel, dim3(point_blocks, (unsigned)V), dim3(THREADS), 0, s, prm, points, mask, K, R, t, keys);
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((words + PIXELS_PER_BLOCK - 1) / PIXELS_PER_BLOCK)), dim3(THREADS), 0, s, words,
                     keys, depth, index, counts);
  hipLaunchKernelGGL(render_visible_kernel, dim3(point_blocks), dim3(THREADS), 0, s, prm, points, mask, K, R, t, depth, visible, num_views,
                     counts);
  ROMA_CHECK_LAUNCH();
}
