// Multi-view depth-map fusion: the forward-backward reprojection test between the depth maps of V posed views (2 <= V <= 32), the
// choice of one owner per surface point, and the compacted cloud — what follows depth_from_warps once every image has a depth map of
// its own.  DESIGN.md §3.4, "Depth-map fusion"; tests/fuse_depth_ref.py restates the three passes in numpy.
//
// Convention (find_absolute_pose / triangulate_nview): x_v ~ K_v (R_v X + t_v).  Pixel (row i, column j) of a map is at (u, v) =
// (j + 0.5, i + 0.5) in the pixels K_v refers to.  A depth that is not a finite positive number is a hole.  The maps are read in place:
// their V base pointers and shapes are kernel arguments by value (FuseTable); every per-pixel output is ONE flat array in which view
// v's map starts at the sum of the pixel counts of the views before it.
//
// Five launches; three of them over one grid (blocks of PIXELS_PER_BLOCK pixels, reference view r), where a block beyond the end of its
// view's map returns.
//   Per block, fp64: threads 0 .. V-1 leave K_v, K_v^-1 (closed form of an upper-triangular K), R_v, t_v in LDS and whether the view is
//   usable (K upper triangular with fx fy k22 != 0, everything finite); then thread s leaves the pair constants of (r, s):
//     M_rs = K_s R_s R_r^T K_r^-1,  e_rs = K_s (t_s - R_s R_r^T t_r),  and M_sr, e_sr the other way round,
//   so that a pixel (u, v) of r at depth d projects into s as q = d M_rs (u, v, 1) + e_rs.  The world's origin cancels in e before any
//   pixel is touched: t_s and R_s R_r^T t_r are both of the size of the offset, their difference is of the size of the scene.
//   consistency (pass 1)   per pixel with a depth, every usable s != r in ascending order: q, skip unless q.z > 0; d_s = the bilinear
//     sample of map s at q.xy / q.z, skip unless all four taps are inside and none is a hole; p = d_s M_sr (u_s, v_s, 1) + e_sr, skip
//     unless p.z > 0; s is consistent when |p.xy / p.z - (u, v)| < max_reproj_error and |p.z - d| / d < max_depth_error — compared as
//     squares, with one reciprocal per projection and one per pixel ("What binds it").  views = bit r and the consistent
//     bits, num_views its popcount, valid = num_views >= min_views, depth = the mean of d and the consistent p.z (added in view order,
//     fp64, rounded once), 0 where not valid.  Reads the input maps only.
//   ownership (pass 2)     a valid pixel is a duplicate when for some s < r with bit s set the pixel (floor v_s, floor u_s) of s is valid
//     and has bit r set; (u_s, v_s) is pass 1's projection, recomputed from the same constants by the same code.  Leaves one flag per
//     pixel (valid and not a duplicate) and three counts per block in the workspace.
//   scan                   one workgroup: exclusive scan of the blocks' flag counts in block order, the totals into counts.
//   cloud (pass 3)         rank of a flagged pixel = its block's offset + the flags before it in the block (ballots and popcounts, the
//     waves through LDS in order); rank < max_points writes the row.  A launch before it clears the cloud, so the rows past the end
//     are 0 with pixel = -1.
// A block never waits for another: what a phase needs from an earlier one is a later launch on the same stream.  No atomics anywhere,
// so the outputs are bitwise the same from run to run.  Every loop has a trip count fixed by V and the shapes.
//
// Gather addressing (as sample_depth in depth_warp.hip).  A projection may be NaN, inf or 1e30, so the un-normalised coordinate is
// range-checked IN FLOATING POINT with a negated conjunction (NaN fails it) before anything is converted to an integer, and every tap
// index is checked against the map again.  No address is formed from an unchecked value; the ownership lookup does the same.
#include "multiview.h"

#include <climits>

namespace roma {
namespace {

constexpr int THREADS = 256, ITEMS = 4, PIXELS_PER_BLOCK = THREADS * ITEMS, WAVES = THREADS / 64;
constexpr int MAX_SIDE = 32768, SCAN_THREADS = 1024;

// kernel arguments by value
struct FuseTable {
  const float* depth[MAX_VIEWS];
  int H[MAX_VIEWS], W[MAX_VIEWS];
  int off[MAX_VIEWS];              // first pixel of view v in the flat per-pixel arrays
  int blk[MAX_VIEWS];              // first block of view v in the per-block counts
};

struct FuseParams {
  int V, min_views, max_points;
  double max_reproj2, max_depth;   // the squared pixel threshold
};

// fp64 per-view constants, in LDS
struct ViewConst {
  double k[9], ki[9], r[9], t[3];
  int ok;
};

// fp64 constants of the pair (r, s), in LDS: q = d m (u, v, 1) + e takes a pixel of r into s, mb / eb a pixel of s into r
struct PairConst {
  double m[9], e[3], mb[9], eb[3];
  int ok;                          // s is usable and s != r (and r is usable)
};

__device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ void mat3_vec(const double* a, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = a[3 * i] * x[0] + a[3 * i + 1] * x[1] + a[3 * i + 2] * x[2];
}

// thread v: K, K^-1, R, t of view v and whether it is usable
__device__ void view_constants(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t, ViewConst& c) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    c.k[i] = K[i];
    c.r[i] = R[i];
    ok = ok && isfinite(K[i]) && isfinite(R[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    c.t[i] = t[i];
    ok = ok && isfinite(t[i]);
  }
  const double fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5], w = K[8];
  const double det = fx * fy * w;
  ok = ok && K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && det != 0.0 && isfinite(1.0 / det);
  c.ki[0] = 1.0 / fx; c.ki[1] = -s / (fx * fy); c.ki[2] = (s * cy - cx * fy) / det;
  c.ki[3] = 0.0;      c.ki[4] = 1.0 / fy;       c.ki[5] = -cy / (fy * w);
  c.ki[6] = 0.0;      c.ki[7] = 0.0;            c.ki[8] = 1.0 / w;
  c.ok = ok ? 1 : 0;
}

// thread s: the pair constants of (r, s)
__device__ void pair_constants(const ViewConst& vr, const ViewConst& vs, bool same, PairConst& c) {
  double a[9], at[9], b[9], x[3], y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a[3 * i + j] = vs.r[3 * i] * vr.r[3 * j] + vs.r[3 * i + 1] * vr.r[3 * j + 1] + vs.r[3 * i + 2] * vr.r[3 * j + 2];   // R_s R_r^T
      at[3 * j + i] = a[3 * i + j];
    }
  mat3_mul(vs.k, a, b);
  mat3_mul(b, vr.ki, c.m);
  mat3_vec(a, vr.t, x);
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = vs.t[i] - x[i];
  mat3_vec(vs.k, y, c.e);
  mat3_mul(vr.k, at, b);
  mat3_mul(b, vs.ki, c.mb);
  mat3_vec(at, vs.t, x);
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = vr.t[i] - x[i];
  mat3_vec(vr.k, y, c.eb);
  c.ok = (vr.ok && vs.ok && !same) ? 1 : 0;
}

// every thread of the block calls it; two barriers
__device__ __forceinline__ void block_constants(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t, int V,
                                                int r, ViewConst* s_view, PairConst* s_pair) {
  const int tid = threadIdx.x;
  if (tid < V) view_constants(K + 9 * tid, R + 9 * tid, t + 3 * tid, s_view[tid]);
  __syncthreads();
  if (tid < V) pair_constants(s_view[r], s_view[tid], tid == r, s_pair[tid]);
  __syncthreads();
}

__device__ __forceinline__ bool is_depth(float d) { return d > 0.f && d <= 3.402823466e+38f; }      // false for NaN, inf, 0, negative

struct Proj {
  double x, y, z;
};
// d m (u, v, 1) + e
__device__ __forceinline__ Proj transfer(const double* m, const double* e, double u, double v, double d) {
  Proj q;
  q.x = d * (m[0] * u + m[1] * v + m[2]) + e[0];
  q.y = d * (m[3] * u + m[4] * v + m[5]) + e[1];
  q.z = d * (m[6] * u + m[7] * v + m[8]) + e[2];
  return q;
}
// q.xy / q.z through ONE division: both passes take a projection's pixel from here, so they agree bit for bit
__device__ __forceinline__ void pixel_of(const Proj& q, double& u, double& v) {
  const double iz = 1.0 / q.z;
  u = q.x * iz;
  v = q.y * iz;
}

// the bilinear sample of a map at pixel coordinates (u, v), taken only when all four taps are inside and none is a hole.  See
// "gather addressing" above: the range test comes first and NaN fails it.
__device__ __forceinline__ bool sample_map(const float* __restrict__ d, int H, int W, double u, double v, double& out) {
  const double ix = u - 0.5, iy = v - 0.5;
  if (!(ix >= 0.0 && ix < (double)(W - 1) && iy >= 0.0 && iy < (double)(H - 1))) return false;
  const double fx = floor(ix), fy = floor(iy);
  const int x0 = (int)fx, y0 = (int)fy;                          // in [0, W-2], [0, H-2]
  if (!(x0 >= 0 && x0 + 1 < W && y0 >= 0 && y0 + 1 < H)) return false;
  const size_t at = (size_t)y0 * (size_t)W + (size_t)x0;
  const float nw = d[at], ne = d[at + 1], sw = d[at + W], se = d[at + W + 1];
  if (!(is_depth(nw) && is_depth(ne) && is_depth(sw) && is_depth(se))) return false;
  const double wx1 = ix - fx, wx0 = (fx + 1.0) - ix, wy1 = iy - fy, wy0 = (fy + 1.0) - iy;
  out = (double)nw * (wx0 * wy0) + (double)ne * (wx1 * wy0) + (double)sw * (wx0 * wy1) + (double)se * (wx1 * wy1);
  return true;
}

// ------------------------------------------------------------------------------------------------------------ pass 1
__global__ __launch_bounds__(THREADS) void fuse_consistency_kernel(FuseTable tab, FuseParams prm, const double* __restrict__ K,
                                                                   const double* __restrict__ R, const double* __restrict__ t,
                                                                   float* __restrict__ depth_out, unsigned char* __restrict__ valid_out,
                                                                   int* __restrict__ views_out, unsigned char* __restrict__ num_out) {
  __shared__ ViewConst s_view[MAX_VIEWS];
  __shared__ PairConst s_pair[MAX_VIEWS];
  const int r = blockIdx.y, tid = threadIdx.x, V = prm.V;
  const int H = tab.H[r], W = tab.W[r];
  const long npix = (long)H * W, n0 = (long)blockIdx.x * PIXELS_PER_BLOCK + tid;
  if ((long)blockIdx.x * PIXELS_PER_BLOCK >= npix) return;       // uniform over the block
  block_constants(K, R, t, V, r, s_view, s_pair);
  const float* __restrict__ dr = tab.depth[r];
  const bool usable = s_view[r].ok != 0;
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {
    const long n = n0 + (long)it * THREADS;
    if (n >= npix) break;
    const float df = dr[n];
    unsigned seen = 0;
    double sum = 0.0;
    if (usable && is_depth(df)) {
      const int i = (int)(n / W), j = (int)(n - (long)i * W);
      const double u = (double)j + 0.5, v = (double)i + 0.5, d = (double)df, inv_d = 1.0 / d;
      seen = 1u << r;
      sum = d;
#pragma unroll 1
      for (int s = 0; s < V; ++s) {
        const PairConst& c = s_pair[s];
        if (!c.ok) continue;
        const Proj q = transfer(c.m, c.e, u, v, d);
        if (!(q.z > 0.0)) continue;
        double us, vs, ds;
        pixel_of(q, us, vs);
        if (!sample_map(tab.depth[s], tab.H[s], tab.W[s], us, vs, ds)) continue;
        const Proj p = transfer(c.mb, c.eb, us, vs, ds);
        if (!(p.z > 0.0)) continue;
        double pu, pv;
        pixel_of(p, pu, pv);
        const double du = pu - u, dv = pv - v;
        if (du * du + dv * dv < prm.max_reproj2 && fabs(p.z - d) * inv_d < prm.max_depth) {
          seen |= 1u << s;
          sum += p.z;
        }
      }
    }
    const int cnt = __popc(seen);
    const bool ok = cnt >= prm.min_views;
    const size_t o = (size_t)tab.off[r] + (size_t)n;
    depth_out[o] = ok ? (float)(sum / (double)cnt) : 0.f;
    valid_out[o] = ok ? 1 : 0;
    views_out[o] = (int)seen;
    num_out[o] = (unsigned char)cnt;
  }
}

// ------------------------------------------------------------------------------------------------------------ pass 2
__global__ __launch_bounds__(THREADS) void fuse_ownership_kernel(FuseTable tab, FuseParams prm, const double* __restrict__ K,
                                                                 const double* __restrict__ R, const double* __restrict__ t,
                                                                 const unsigned char* __restrict__ valid, const int* __restrict__ views,
                                                                 unsigned char* __restrict__ flag, unsigned* __restrict__ block_counts) {
  __shared__ ViewConst s_view[MAX_VIEWS];
  __shared__ PairConst s_pair[MAX_VIEWS];
  __shared__ unsigned s_n[3][WAVES];
  const int r = blockIdx.y, tid = threadIdx.x, V = prm.V;
  const int H = tab.H[r], W = tab.W[r];
  const long npix = (long)H * W, n0 = (long)blockIdx.x * PIXELS_PER_BLOCK + tid;
  if ((long)blockIdx.x * PIXELS_PER_BLOCK >= npix) return;
  block_constants(K, R, t, V, r, s_view, s_pair);
  const float* __restrict__ dr = tab.depth[r];
  unsigned n_emit = 0, n_valid = 0, n_dup = 0;                   // wave-uniform
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {                           // no break: every lane takes part in the ballots
    const long n = n0 + (long)it * THREADS;
    const bool in = n < npix;
    const size_t o = (size_t)tab.off[r] + (size_t)(in ? n : 0);
    const bool ok = in && valid[o] != 0;
    bool dup = false;
    if (ok) {
      const unsigned seen = (unsigned)views[o];
      const int i = (int)(n / W), j = (int)(n - (long)i * W);
      const double u = (double)j + 0.5, v = (double)i + 0.5, d = (double)dr[n];
#pragma unroll 1
      for (int s = 0; s < r; ++s) {
        if (!((seen >> s) & 1u)) continue;
        const PairConst& c = s_pair[s];
        const Proj q = transfer(c.m, c.e, u, v, d);
        double us, vs;
        pixel_of(q, us, vs);
        const int Hs = tab.H[s], Ws = tab.W[s];
        if (!(us >= 0.0 && us < (double)Ws && vs >= 0.0 && vs < (double)Hs)) continue;
        const int col = (int)floor(us), row = (int)floor(vs);
        if (!(col >= 0 && col < Ws && row >= 0 && row < Hs)) continue;
        const size_t os = (size_t)tab.off[s] + (size_t)row * (size_t)Ws + (size_t)col;
        if (valid[os] != 0 && (((unsigned)views[os] >> r) & 1u)) dup = true;
      }
    }
    if (in) flag[o] = (ok && !dup) ? 1 : 0;
    n_emit += (unsigned)__popcll(__ballot(ok && !dup));
    n_valid += (unsigned)__popcll(__ballot(ok));
    n_dup += (unsigned)__popcll(__ballot(ok && dup));
  }
  if ((tid & 63) == 0) {
    s_n[0][tid >> 6] = n_emit;
    s_n[1][tid >> 6] = n_valid;
    s_n[2][tid >> 6] = n_dup;
  }
  __syncthreads();
  if (tid < 3) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) n += s_n[tid][w];
    block_counts[3 * ((size_t)tab.blk[r] + blockIdx.x) + tid] = n;
  }
}

// ------------------------------------------------------------------------------------------------------------ scan
// (the loop of tracks.hip's tracks_scan_kernel, written out in both: profiles/multiview_shared_code_micro.txt)
// one workgroup: block_counts[b][0] becomes the number of flagged pixels in the blocks before b; counts = the totals and a status of 0
__global__ __launch_bounds__(SCAN_THREADS) void fuse_scan_kernel(unsigned* __restrict__ block_counts, int blocks, int* __restrict__ counts) {
  __shared__ unsigned s_wave[SCAN_THREADS / 64];
  __shared__ unsigned s_tot[2][SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0, n_valid = 0, n_dup = 0;
  for (int b0 = 0; b0 < blocks; b0 += SCAN_THREADS) {
    const int b = b0 + threadIdx.x;
    const unsigned v = b < blocks ? block_counts[3 * (size_t)b] : 0u;
    if (b < blocks) {
      n_valid += block_counts[3 * (size_t)b + 1];
      n_dup += block_counts[3 * (size_t)b + 2];
    }
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const unsigned n = s_wave[w];
      if (w < wave) before += n;
      total += n;
    }
    if (b < blocks) block_counts[3 * (size_t)b] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_valid += __shfl_xor(n_valid, o, 64);
    n_dup += __shfl_xor(n_dup, o, 64);
  }
  if (lane == 0) { s_tot[0][wave] = n_valid; s_tot[1][wave] = n_dup; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = 0, d = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) { a += s_tot[0][w]; d += s_tot[1][w]; }
    counts[0] = (int)carry;
    counts[1] = (int)a;
    counts[2] = (int)d;
    counts[3] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------ pass 3
__global__ __launch_bounds__(THREADS) void fuse_clear_kernel(int T, float* __restrict__ points, unsigned char* __restrict__ view,
                                                             int* __restrict__ pixel, int* __restrict__ point_views) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= T) return;
  points[3 * i] = 0.f; points[3 * i + 1] = 0.f; points[3 * i + 2] = 0.f;
  view[i] = 0;
  pixel[i] = -1;
  point_views[i] = 0;
}

__global__ __launch_bounds__(THREADS) void fuse_cloud_kernel(FuseTable tab, FuseParams prm, const double* __restrict__ K,
                                                             const double* __restrict__ R, const double* __restrict__ t,
                                                             const float* __restrict__ depth, const int* __restrict__ views,
                                                             const unsigned char* __restrict__ flag, const unsigned* __restrict__ block_counts,
                                                             float* __restrict__ points, unsigned char* __restrict__ view,
                                                             int* __restrict__ pixel, int* __restrict__ point_views) {
  __shared__ ViewConst s_view;
  __shared__ unsigned s_n[ITEMS][WAVES];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = tab.W[r];
  const long npix = (long)tab.H[r] * W, n0 = (long)blockIdx.x * PIXELS_PER_BLOCK + tid;
  if ((long)blockIdx.x * PIXELS_PER_BLOCK >= npix) return;
  if (tid == 0) view_constants(K + 9 * r, R + 9 * r, t + 3 * r, s_view);
  unsigned before[ITEMS];                                        // flagged lanes of this wave below this one, per item; bit 31 = own flag
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const long n = n0 + (long)it * THREADS;
    const bool f = n < npix && flag[(size_t)tab.off[r] + (size_t)n] != 0;
    const unsigned long long votes = __ballot(f);
    before[it] = (unsigned)__popcll(votes & ((1ull << lane) - 1ull)) | (f ? 0x80000000u : 0u);
    if (lane == 0) s_n[it][wave] = (unsigned)__popcll(votes);
  }
  __syncthreads();
  unsigned base = block_counts[3 * ((size_t)tab.blk[r] + blockIdx.x)];
  const ViewConst& c = s_view;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    unsigned rank = base + (before[it] & 0x7fffffffu);
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) rank += s_n[it][w];
      base += s_n[it][w];
    }
    if (!(before[it] >> 31) || rank >= (unsigned)prm.max_points) continue;
    const long n = n0 + (long)it * THREADS;
    const size_t o = (size_t)tab.off[r] + (size_t)n;
    const int i = (int)(n / W), j = (int)(n - (long)i * W);
    const double u = (double)j + 0.5, v = (double)i + 0.5, d = (double)depth[o];
    const double a0 = (c.ki[0] * u + c.ki[1] * v + c.ki[2]) * d - c.t[0], a1 = (c.ki[4] * v + c.ki[5]) * d - c.t[1],
                 a2 = c.ki[8] * d - c.t[2];
    points[3 * (size_t)rank] = (float)(c.r[0] * a0 + c.r[3] * a1 + c.r[6] * a2);
    points[3 * (size_t)rank + 1] = (float)(c.r[1] * a0 + c.r[4] * a1 + c.r[7] * a2);
    points[3 * (size_t)rank + 2] = (float)(c.r[2] * a0 + c.r[5] * a1 + c.r[8] * a2);
    view[rank] = (unsigned char)r;
    pixel[rank] = (int)n;
    point_views[rank] = views[o];
  }
}

inline long align256(long v) { return (v + 255) & ~255L; }
inline long most_blocks(int V, long total) { return total / PIXELS_PER_BLOCK + V; }      // sum over views of ceil(pixels / block) at most

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_depth_fuse_workspace(int V, long total_pixels, long* out_bytes) {
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "roma_depth_fuse_workspace: bad shape V=%d (2 to %d views)", V, MAX_VIEWS);
  ROMA_REQUIRE(total_pixels >= V && total_pixels <= (long)INT_MAX, ROMA_E_SHAPE,
               "roma_depth_fuse_workspace: bad shape total_pixels=%ld (at least one pixel per view, at most 2^31 - 1 in all)", total_pixels);
  const long flags = align256(total_pixels), blocks = align256(12 * most_blocks(V, total_pixels));
  if (out_bytes) {
    out_bytes[0] = flags;
    out_bytes[1] = blocks;
  }
  return flags + blocks;
}

extern "C" int roma_depth_fuse(const float* const* depths, const int* dims, const double* K, const double* R, const double* t, int V,
                               double max_reproj_error, double max_depth_error, int min_views, int max_points, float* depth,
                               unsigned char* valid, int* views, unsigned char* num_views, float* points, unsigned char* view, int* pixel,
                               int* point_views, int* counts, void* workspace, long workspace_bytes, void* stream) {
  ROMA_REQUIRE(depths && dims && K && R && t, ROMA_E_ARG, "roma_depth_fuse: null pointer");
  ROMA_REQUIRE(depth && valid && views && num_views && points && view && pixel && point_views && counts && workspace, ROMA_E_ARG,
               "roma_depth_fuse: null pointer (every output and the workspace are required)");
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "roma_depth_fuse: bad shape V=%d (2 to %d views)", V, MAX_VIEWS);
  ROMA_REQUIRE(max_reproj_error > 0.0 && max_depth_error > 0.0, ROMA_E_ARG,
               "roma_depth_fuse: max_reproj_error and max_depth_error must be positive, got %g and %g", max_reproj_error, max_depth_error);
  ROMA_REQUIRE(min_views >= 2 && min_views <= V, ROMA_E_ARG, "roma_depth_fuse: min_views must be in [2, V=%d], got %d", V, min_views);
  ROMA_REQUIRE(max_points >= 1, ROMA_E_ARG, "roma_depth_fuse: max_points must be at least 1, got %d", max_points);
  FuseTable tab;
  long total = 0, blocks = 0, most = 0;
  for (int v = 0; v < V; ++v) {
    const int H = dims[2 * v], W = dims[2 * v + 1];
    ROMA_REQUIRE(H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE, ROMA_E_SHAPE, "roma_depth_fuse: bad shape map %d is %dx%d (sides 1 to %d)",
                 v, H, W, MAX_SIDE);
    ROMA_REQUIRE(depths[v] != nullptr, ROMA_E_ARG, "roma_depth_fuse: null pointer (depth map of view %d)", v);
    ROMA_REQUIRE(aligned4(depths[v]), ROMA_E_ALIGN, "roma_depth_fuse: the depth map of view %d must be 4-byte aligned",
                 v);
    const long n = (long)H * W, nb = (n + PIXELS_PER_BLOCK - 1) / PIXELS_PER_BLOCK;
    tab.depth[v] = depths[v];
    tab.H[v] = H;
    tab.W[v] = W;
    tab.off[v] = (int)total;
    tab.blk[v] = (int)blocks;
    total += n;
    blocks += nb;
    most = nb > most ? nb : most;
    ROMA_REQUIRE(total <= (long)INT_MAX, ROMA_E_SHAPE, "roma_depth_fuse: bad shape: the maps have more than 2^31 - 1 pixels in all");
  }
  for (int v = V; v < MAX_VIEWS; ++v) {
    tab.depth[v] = depths[0];
    tab.H[v] = tab.W[v] = 1;
    tab.off[v] = tab.blk[v] = 0;
  }
  const long flag_bytes = align256(total), need = flag_bytes + align256(12 * most_blocks(V, total));
  ROMA_REQUIRE(workspace_bytes >= need, ROMA_E_ARG, "roma_depth_fuse: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  ROMA_REQUIRE(aligned16(workspace), ROMA_E_ALIGN, "roma_depth_fuse: the workspace must be 16-byte aligned");
  FuseParams prm;
  prm.V = V; prm.min_views = min_views; prm.max_points = max_points;
  prm.max_reproj2 = max_reproj_error * max_reproj_error; prm.max_depth = max_depth_error;
  unsigned char* flag = static_cast<unsigned char*>(workspace);
  unsigned* block_counts = reinterpret_cast<unsigned*>(flag + flag_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)most, (unsigned)V);
  hipLaunchKernelGGL(fuse_consistency_kernel, grid, dim3(THREADS), 0, s, tab, prm, K, R, t, depth, valid, views, num_views);
  hipLaunchKernelGGL(fuse_ownership_kernel, grid, dim3(THREADS), 0, s, tab, prm, K, R, t, valid, views, flag, block_counts);
  hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, block_counts, (int)blocks, counts);
  hipLaunchKernelGGL(fuse_clear_kernel, dim3((unsigned)((max_points + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, max_points, points, view,
                     pixel, point_views);
  hipLaunchKernelGGL(fuse_cloud_kernel, grid, dim3(THREADS), 0, s, tab, prm, K, R, t, depth, views, flag, block_counts, points, view, pixel,
                     point_views);
  ROMA_CHECK_LAUNCH();
}
