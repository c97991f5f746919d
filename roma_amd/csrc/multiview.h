// What the multi-view kernels share (triangulate_nview.hip, tracks.hip, bundle.hip, depth_fuse.hip, motion_average.hip): MAX_VIEWS, the
// table of per-view observations and the host loop that fills it, the pixel of one observation, the upper-triangular test of K, small
// index and 3 x 3 helpers, the body of the partial-sum reduce kernels and the 256-byte workspace layout.  Device helpers and host checks
// only: no __global__ code and no device data.  DESIGN.md §3.4.  What was tried in here and went back into its kernels (the scan of
// per-block counts, the rotation step, the usable-view predicate): profiles/multiview_shared_code_isa.txt and _micro.txt.
// Nothing in here fixes a contraction mode: a file that compiles its kernels under `#pragma clang fp contract(off)`
// (motion_average.hip) includes this header AFTER the pragma, so that these functions round there as the file's own code does.
#pragma once
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int MAX_VIEWS = 32;

// ------------------------------------------------------------------------------------------------------------- observations
// kernel arguments by value: base pointers, visibility pointers (null = always visible), pixel = s * c + o per coordinate.  Entries
// at and above V repeat view 0, so that no entry is ever an address that cannot be read
struct ObsTable {
  const float* obs[MAX_VIEWS];
  const unsigned char* vis[MAX_VIEWS];
  float px[MAX_VIEWS][4];          // sx, ox, sy, oy
};

// host: the table of an entry point's V views; 0, or a negative code with the error set (fn names the entry point in the message)
inline int fill_obs_table(const char* fn, const float* const* obs, const float* to_px, const unsigned char* const* visible, int V, ObsTable& tab) {
  for (int v = 0; v < MAX_VIEWS; ++v) {
    const int u = v < V ? v : 0;
    ROMA_REQUIRE(obs[u] != nullptr, ROMA_E_ARG, "%s: null pointer (observations of view %d)", fn, u);
    ROMA_REQUIRE(aligned8(obs[u]), ROMA_E_ALIGN, "%s: the observations of view %d must be 8-byte aligned", fn, u);
    tab.obs[v] = obs[u];
    tab.vis[v] = visible ? visible[u] : nullptr;
    for (int i = 0; i < 4; ++i) tab.px[v][i] = to_px ? to_px[4 * u + i] : ((i & 1) ? 0.f : 1.f);
  }
  return 0;
}

// the pixel (x, y) of (v, n), points `stride` floats apart; false where not seen (not visible, or not finite)
__device__ __forceinline__ bool load_px(const ObsTable& tab, int v, long n, long stride, float& x, float& y) {
  const float2 q = *reinterpret_cast<const float2*>(tab.obs[v] + n * stride);
  const unsigned char* vis = tab.vis[v];
  const bool see = vis ? vis[n] != 0 : true;
  x = q.x * tab.px[v][0] + tab.px[v][1];
  y = q.y * tab.px[v][2] + tab.px[v][3];
  return see && isfinite(x) && isfinite(y);
}
// the same as one value, NaN where not seen
__device__ __forceinline__ float2 load_px(const ObsTable& tab, int v, long n, long stride) {
  float x, y;
  const float nanf = __builtin_nanf("");
  return load_px(tab, v, n, stride, x, y) ? make_float2(x, y) : make_float2(nanf, nanf);
}

// ------------------------------------------------------------------------------------------------------------------- views
// the half of "view v is usable" that no caller spells differently: K is upper triangular with a finite last entry.  (That K^-1
// exists, that R and t are finite and the centre -R^T t stay written out in the init code of triangulate_nview.hip, bundle.hip and
// motion_average.hip: behind a shared function the first two are no longer the parent's instructions, and motion_average.hip must not
// contract its K^-1 — profiles/multiview_shared_code_isa.txt)
__device__ __forceinline__ bool upper_triangular(const double* K) { return K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && isfinite(K[8]); }

// ------------------------------------------------------------------------------------------------------------ small helpers
// entries of the packed lower triangle before row n
__host__ __device__ inline int tri(int n) { return n * (n + 1) / 2; }

// y = S x, S symmetric 3 x 3 as (s00, s01, s02, s11, s12, s22)
__device__ __forceinline__ void sym3_times(const double* s, const double* x, double* y) {
  y[0] = s[0] * x[0] + s[1] * x[1] + s[2] * x[2];
  y[1] = s[1] * x[0] + s[3] * x[1] + s[4] * x[2];
  y[2] = s[2] * x[0] + s[4] * x[1] + s[5] * x[2];
}

// ------------------------------------------------------------------------------------------------------ partial sums, layout
// the body of a reduce kernel, a thread per entry: entry e of sys = its P partials (part is P x M) added in block order.  The kernels
// stay in their files under their names: they unpack their own workspace records, and the tests' resource reports count them.  M and
// P by reference: a field of the caller's record is read where it is used
__device__ __forceinline__ void reduce_partials(const double* part, double* sys, const int& M, const int& P, int e) {
  if (e >= M) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += part[(size_t)p * M + e];
  sys[e] = s;
}

// host: bytes of a workspace of n regions and (off != null) their offsets, each 256-byte aligned
inline long layout_regions(const long* bytes, int n, long* off) {
  long at = 0;
  for (int i = 0; i < n; ++i) {
    if (off) off[i] = at;
    at += (bytes[i] + 255) / 256 * 256;
  }
  return at;
}

}  // namespace
}  // namespace roma
