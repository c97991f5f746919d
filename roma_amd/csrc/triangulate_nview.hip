// N-view triangulation of one reconstruction: a point seen in V posed views (2 <= V <= 32), triangulated from all of them with the
// views that disagree left out — what follows find_absolute_pose when the third, fourth, ... camera is to add structure, and what
// turns the k warps of one reference image against k others into ONE depth map.  DESIGN.md §3.4, "N-view triangulation".
//
// Convention (find_absolute_pose): x_v ~ K_v (R_v X + t_v), v = 0 .. V-1.  There is no batch of reconstructions: the views are the
// batch.  The observations are read in place: view v's point n = r * row_len + c is the float2 at obs[v] + r * row_stride +
// c * point_stride (floats), so V warps in V tensors need no copy; the V base pointers, the optional per-view map to pixels and the
// optional per-view visibility pointers are kernel arguments by value (multiview.h's ObsTable).
//
// One launch, grid (blocks of THREADS columns, rows): a 2-D grid, no integer division per point.
//   Per block, threads 0 .. V-1 in fp64: K_v^-1 (invert_k), the centre C_v = -R_v^T t_v; then c0 = the mean of the centres of the
//   usable views, summed in view order, and everything relative to it: C'_v = C_v - c0, t'_v = t_v + R_v c0 (R_v X + t_v = R_v X' + t'_v
//   with X' = X - c0).  They are left as fp32 in LDS (ViewConst).  That is the fp64 / fp32 boundary, and why fp32 does not care where
//   the world's origin is; c0 comes back in fp64 when the point is written.  A view with a singular K or a pose that is not finite
//   is unobservable for every point.
//   Per point, one thread, fp32, IEEE operations (no fast-math; the compiler may fuse a multiply with an add):
//     load: each observation comes from HBM once, is mapped to pixels and parked in the thread's own column of an LDS slab
//       (V x THREADS float2, dynamic, view-major: lane-contiguous 8-byte reads, no bank conflict); NaN where not observed (not
//       visible, not finite, view unusable).  Every later pass — the robust search, the linear start, each LM step — reads the slab;
//       the view set is a bit mask in a register, never a per-thread array.
//     view set: max_view_error = inf: the observed views.  Otherwise every pair (a, b), a < b, of observed views gives the midpoint
//       of its two rays; a view is an inlier of it with positive depth and a pixel error <= max_view_error; the hypothesis counts if
//       a and b are inliers; score = sum over the observed views of (inlier ? e^2 : thr^2); lowest score, first pair on a tie; the
//       set is the winner's inliers.  O(V^3) per point on purpose: a least-squares fit over all views is pulled by one gross outlier
//       until every view fails the gate.
//     linear start: the point closest to the rays of the set, (sum I - d d^T) X = sum (I - d d^T) C', unit d = R^T K^-1 x~.
//     refinement: `iters` Levenberg-Marquardt steps on the sum of squared pixel errors over the set, analytic Jacobians, lambda_0 =
//       1e-3 on the scaled diagonal, a step kept only if the cost drops (lambda / 10, else lambda * 10).
//     outputs: points (world, fp32 of the fp64 sum X' + c0), depth = z in view ref_view, reproj = sqrt(mean over the set of e^2),
//       cos_parallax = the smallest cosine over pairs of the set between the rays from the point to the centres, views = the set,
//       valid = |set| >= min_views && finite && every depth of the set > 0 && reproj <= max_reproj && cos_parallax <= max_cos.
//   A point with fewer than two views in its set, or without a finite solution, gets exact zeros everywhere (views = 0); any other
//   point its values, valid or not; no NaN or inf is ever written.  No atomics, no workspace; tests/triangulate_nview_ref.py restates
//   it in numpy.
#include "multiview.h"

namespace roma {
namespace {

constexpr int THREADS = 256;

// fp32 per-view constants, in LDS
struct ViewConst {
  float k[5];                      // fx, s, cx, fy, cy
  float ki[5];                     // invert_k's five entries of K^-1
  float r[9];
  float c[3];                      // C' = C - c0
  float t[3];                      // t' = t + R c0
  float pad[3];
};
static_assert(sizeof(ViewConst) == 112, "ViewConst is 28 floats");

struct NviewParams {
  int V, row_len, iters, min_views, ref_view, robust;
  long row_stride, point_stride, vis_row_stride;
  float thr2, max_reproj, max_cos;
};

struct Vec3 {
  float x, y, z;
};

// unit bearing d = R^T K^-1 (x, y, 1) of a pixel, in the world frame
__device__ __forceinline__ Vec3 bearing(const ViewConst& c, float2 p) {
  const float a0 = c.ki[0] * p.x + c.ki[1] * p.y + c.ki[2], a1 = c.ki[3] * p.y + c.ki[4];
  const float d0 = c.r[0] * a0 + c.r[3] * a1 + c.r[6], d1 = c.r[1] * a0 + c.r[4] * a1 + c.r[7], d2 = c.r[2] * a0 + c.r[5] * a1 + c.r[8];
  const float inv = 1.f / sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  return {d0 * inv, d1 * inv, d2 * inv};
}

// q = R X' + t' and the pixel residual (ru, rv) = pi(q) - p
struct Proj {
  float q0, q1, z, iz, ru, rv;
};
__device__ __forceinline__ Proj project(const ViewConst& c, Vec3 X, float2 p) {
  Proj o;
  o.q0 = c.r[0] * X.x + c.r[1] * X.y + c.r[2] * X.z + c.t[0];
  o.q1 = c.r[3] * X.x + c.r[4] * X.y + c.r[5] * X.z + c.t[1];
  o.z = c.r[6] * X.x + c.r[7] * X.y + c.r[8] * X.z + c.t[2];
  o.iz = 1.f / o.z;
  o.ru = (c.k[0] * o.q0 + c.k[1] * o.q1) * o.iz + c.k[2] - p.x;
  o.rv = c.k[3] * o.q1 * o.iz + c.k[4] - p.y;
  return o;
}

// symmetric 3 x 3 solve by cofactors, static indexing; a singular matrix gives inf / NaN, which the caller's tests catch
struct Sym3 {
  float a00, a01, a02, a11, a12, a22;
};
__device__ __forceinline__ Vec3 solve_sym3(const Sym3& a, Vec3 b) {
  const float c00 = a.a11 * a.a22 - a.a12 * a.a12, c01 = a.a02 * a.a12 - a.a01 * a.a22, c02 = a.a01 * a.a12 - a.a02 * a.a11;
  const float c11 = a.a00 * a.a22 - a.a02 * a.a02, c12 = a.a01 * a.a02 - a.a00 * a.a12, c22 = a.a00 * a.a11 - a.a01 * a.a01;
  const float det = a.a00 * c00 + a.a01 * c01 + a.a02 * c02;
  return {(c00 * b.x + c01 * b.y + c02 * b.z) / det, (c01 * b.x + c11 * b.y + c12 * b.z) / det, (c02 * b.x + c12 * b.y + c22 * b.z) / det};
}

// cost, smallest depth, J^T J and J^T r of the pixel residuals of X over the view set
struct Normal {
  float cost, minz;
  Sym3 h;
  Vec3 g;
};
__device__ __forceinline__ Normal evaluate(const ViewConst* vc, const float2* col, int V, unsigned set, Vec3 X) {
  Normal n;
  n.cost = 0.f;
  n.minz = __builtin_inff();
  n.h = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  n.g = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int v = 0; v < V; ++v) {
    if (!((set >> v) & 1u)) continue;
    const ViewConst& c = vc[v];
    const Proj p = project(c, X, col[v * THREADS]);
    n.cost += p.ru * p.ru + p.rv * p.rv;
    n.minz = p.z < n.minz ? p.z : n.minz;
    // d pi / d q, then times R
    const float u0 = c.k[0] * p.iz, u1 = c.k[1] * p.iz, u2 = -(c.k[0] * p.q0 + c.k[1] * p.q1) * p.iz * p.iz;
    const float v1 = c.k[3] * p.iz, v2 = -(c.k[3] * p.q1) * p.iz * p.iz;
    const float ju0 = u0 * c.r[0] + u1 * c.r[3] + u2 * c.r[6], ju1 = u0 * c.r[1] + u1 * c.r[4] + u2 * c.r[7],
                ju2 = u0 * c.r[2] + u1 * c.r[5] + u2 * c.r[8];
    const float jv0 = v1 * c.r[3] + v2 * c.r[6], jv1 = v1 * c.r[4] + v2 * c.r[7], jv2 = v1 * c.r[5] + v2 * c.r[8];
    n.h.a00 += ju0 * ju0 + jv0 * jv0; n.h.a01 += ju0 * ju1 + jv0 * jv1; n.h.a02 += ju0 * ju2 + jv0 * jv2;
    n.h.a11 += ju1 * ju1 + jv1 * jv1; n.h.a12 += ju1 * ju2 + jv1 * jv2; n.h.a22 += ju2 * ju2 + jv2 * jv2;
    n.g.x += ju0 * p.ru + jv0 * p.rv; n.g.y += ju1 * p.ru + jv1 * p.rv; n.g.z += ju2 * p.ru + jv2 * p.rv;
  }
  return n;
}

__global__ __launch_bounds__(THREADS) void triangulate_nview_kernel(ObsTable tab, NviewParams prm, const double* __restrict__ K,
                                                                    const double* __restrict__ R, const double* __restrict__ t,
                                                                    float* __restrict__ points, float* __restrict__ depth,
                                                                    float* __restrict__ reproj_out, float* __restrict__ cos_out,
                                                                    unsigned* __restrict__ views, unsigned char* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* slab = reinterpret_cast<float2*>(smem);                 // [V][THREADS]
  __shared__ ViewConst s_view[MAX_VIEWS];
  __shared__ double s_centre[MAX_VIEWS][3];
  __shared__ double s_c0[3];
  __shared__ int s_ok[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V;

  // ---- per-view constants, fp64 -> fp32
  double ki[5], c[3];
  if (tid < V) {
    const double* Kv = K + 9 * tid;
    const double* Rv = R + 9 * tid;
    const double* tv = t + 3 * tid;
    bool ok = invert_k(Kv, ki);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(Rv[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && isfinite(tv[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      c[j] = -(Rv[j] * tv[0] + Rv[3 + j] * tv[1] + Rv[6 + j] * tv[2]);
      s_centre[tid][j] = c[j];
    }
    s_ok[tid] = ok ? 1 : 0;
  }
  __syncthreads();
  if (tid < V) {
    double c0[3] = {0.0, 0.0, 0.0};
    int n = 0;
    for (int u = 0; u < V; ++u) {
      if (!s_ok[u]) continue;
      c0[0] += s_centre[u][0]; c0[1] += s_centre[u][1]; c0[2] += s_centre[u][2];
      ++n;
    }
    if (n > 0) { c0[0] /= n; c0[1] /= n; c0[2] /= n; }
    const double* Kv = K + 9 * tid;
    const double* Rv = R + 9 * tid;
    const double* tv = t + 3 * tid;
    ViewConst& o = s_view[tid];
    o.k[0] = (float)Kv[0]; o.k[1] = (float)Kv[1]; o.k[2] = (float)Kv[2]; o.k[3] = (float)Kv[4]; o.k[4] = (float)Kv[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) o.ki[i] = (float)ki[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) o.r[i] = (float)Rv[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      o.c[j] = (float)(c[j] - c0[j]);
      o.t[j] = (float)(tv[j] + (Rv[3 * j] * c0[0] + Rv[3 * j + 1] * c0[1] + Rv[3 * j + 2] * c0[2]));
      o.pad[j] = 0.f;
    }
    if (tid == 0) { s_c0[0] = c0[0]; s_c0[1] = c0[1]; s_c0[2] = c0[2]; }
  }
  __syncthreads();

  const int col_i = blockIdx.x * THREADS + tid, row = blockIdx.y;
  if (col_i >= prm.row_len) return;                               // no barrier below: the slab column is the thread's own
  float2* col = slab + tid;

  // ---- observations: HBM -> pixels -> the thread's slab column
  unsigned obs = 0;
  {
    const long off = (long)row * prm.row_stride + (long)col_i * prm.point_stride;
    const long voff = (long)row * prm.vis_row_stride + (long)col_i;
    const float nan = __builtin_nanf("");
#pragma unroll 4
    for (int v = 0; v < V; ++v) {
      float2 p = {nan, nan};
      if (s_ok[v]) {
        const float2 q = *reinterpret_cast<const float2*>(tab.obs[v] + off);
        const unsigned char* vis = tab.vis[v];
        const bool see = vis ? vis[voff] != 0 : true;
        const float x = q.x * tab.px[v][0] + tab.px[v][1], y = q.y * tab.px[v][2] + tab.px[v][3];
        if (see && isfinite(x) && isfinite(y)) {
          p = {x, y};
          obs |= 1u << v;
        }
      }
      col[v * THREADS] = p;
    }
  }

  // ---- the view set
  unsigned set = obs;
  if (prm.robust) {
    set = 0;
    float best = __builtin_inff();
    const float thr2 = prm.thr2;
#pragma unroll 1
    for (int a = 0; a < V - 1; ++a) {
      if (!((obs >> a) & 1u)) continue;
      const Vec3 da = bearing(s_view[a], col[a * THREADS]);
      const Vec3 ca = {s_view[a].c[0], s_view[a].c[1], s_view[a].c[2]};
#pragma unroll 1
      for (int b = a + 1; b < V; ++b) {
        if (!((obs >> b) & 1u)) continue;
        const Vec3 db = bearing(s_view[b], col[b * THREADS]);
        const Vec3 cb = {s_view[b].c[0], s_view[b].c[1], s_view[b].c[2]};
        // the midpoint of the two rays' closest points
        const float w0 = ca.x - cb.x, w1 = ca.y - cb.y, w2 = ca.z - cb.z;
        const float ab = da.x * db.x + da.y * db.y + da.z * db.z;
        const float aw = da.x * w0 + da.y * w1 + da.z * w2, bw = db.x * w0 + db.y * w1 + db.z * w2;
        const float den = 1.f - ab * ab;
        const float sa = (ab * bw - aw) / den, sb = (bw - ab * aw) / den;
        const Vec3 M = {0.5f * ((ca.x + sa * da.x) + (cb.x + sb * db.x)), 0.5f * ((ca.y + sa * da.y) + (cb.y + sb * db.y)),
                        0.5f * ((ca.z + sa * da.z) + (cb.z + sb * db.z))};
        float score = 0.f;
        unsigned inl = 0;
#pragma unroll 1
        for (int v = 0; v < V; ++v) {
          if (!((obs >> v) & 1u)) continue;
          const Proj p = project(s_view[v], M, col[v * THREADS]);
          const float e2 = p.ru * p.ru + p.rv * p.rv;
          const bool in = p.z > 0.f && e2 <= thr2;
          score += in ? e2 : thr2;
          inl |= (in ? 1u : 0u) << v;
        }
        if (((inl >> a) & 1u) && ((inl >> b) & 1u) && score < best) {
          best = score;
          set = inl;
        }
      }
    }
  }
  const int nset = __popc(set);

  // ---- linear start and refinement
  Vec3 X = {0.f, 0.f, 0.f};
  Normal cur;
  cur.cost = 0.f;
  cur.minz = 0.f;
  if (nset >= 2) {
    Sym3 A = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Vec3 rhs = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      if (!((set >> v) & 1u)) continue;
      const Vec3 d = bearing(s_view[v], col[v * THREADS]);
      const float c0 = s_view[v].c[0], c1 = s_view[v].c[1], c2 = s_view[v].c[2];
      const float dc = d.x * c0 + d.y * c1 + d.z * c2;
      A.a00 += 1.f - d.x * d.x; A.a01 -= d.x * d.y; A.a02 -= d.x * d.z;
      A.a11 += 1.f - d.y * d.y; A.a12 -= d.y * d.z; A.a22 += 1.f - d.z * d.z;
      rhs.x += c0 - d.x * dc; rhs.y += c1 - d.y * dc; rhs.z += c2 - d.z * dc;
    }
    X = solve_sym3(A, rhs);
    cur = evaluate(s_view, col, V, set, X);
    float lambda = 1e-3f;
#pragma unroll 1
    for (int it = 0; it < prm.iters; ++it) {
      Sym3 h = cur.h;
      h.a00 += lambda * h.a00; h.a11 += lambda * h.a11; h.a22 += lambda * h.a22;
      const Vec3 step = solve_sym3(h, cur.g);
      const Vec3 Xn = {X.x - step.x, X.y - step.y, X.z - step.z};
      const Normal nxt = evaluate(s_view, col, V, set, Xn);
      if (nxt.cost < cur.cost) {
        X = Xn;
        cur = nxt;
        lambda *= 0.1f;
      } else {
        lambda *= 10.f;
      }
    }
  }

  // ---- outputs
  float reproj = sqrtf(cur.cost / (float)nset);
  const ViewConst& rv = s_view[prm.ref_view];
  float z_ref = rv.r[6] * X.x + rv.r[7] * X.y + rv.r[8] * X.z + rv.t[2];
  float cosp = 2.f;
#pragma unroll 1
  for (int a = 0; a < V - 1; ++a) {
    if (!((set >> a) & 1u)) continue;
    const float a0 = s_view[a].c[0] - X.x, a1 = s_view[a].c[1] - X.y, a2 = s_view[a].c[2] - X.z;
    const float ia = 1.f / sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
#pragma unroll 1
    for (int b = a + 1; b < V; ++b) {
      if (!((set >> b) & 1u)) continue;
      const float b0 = s_view[b].c[0] - X.x, b1 = s_view[b].c[1] - X.y, b2 = s_view[b].c[2] - X.z;
      const float ib = 1.f / sqrtf(b0 * b0 + b1 * b1 + b2 * b2);
      const float d = (a0 * b0 + a1 * b1 + a2 * b2) * (ia * ib);
      cosp = d < cosp ? d : cosp;
    }
  }
  float pw0 = (float)((double)X.x + s_c0[0]), pw1 = (float)((double)X.y + s_c0[1]), pw2 = (float)((double)X.z + s_c0[2]);
  const bool fin = nset >= 2 && isfinite(X.x) && isfinite(X.y) && isfinite(X.z) && isfinite(pw0) && isfinite(pw1) && isfinite(pw2) &&
                   isfinite(z_ref) && isfinite(reproj) && isfinite(cur.minz) && cosp <= 1.5f;
  if (!fin) { pw0 = 0.f; pw1 = 0.f; pw2 = 0.f; z_ref = 0.f; reproj = 0.f; cosp = 0.f; set = 0; }
  const bool ok = fin && nset >= prm.min_views && cur.minz > 0.f && reproj <= prm.max_reproj && cosp <= prm.max_cos;
  const size_t n = (size_t)row * (size_t)prm.row_len + (size_t)col_i;
  if (points) { points[3 * n] = pw0; points[3 * n + 1] = pw1; points[3 * n + 2] = pw2; }
  if (depth) depth[n] = z_ref;
  if (reproj_out) reproj_out[n] = reproj;
  if (cos_out) cos_out[n] = cosp;
  if (views) views[n] = set;
  if (valid) valid[n] = ok ? 1 : 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_triangulate_nview(const float* const* obs, const float* to_px, const unsigned char* const* visible, long vis_row_stride,
                                      const double* K, const double* R, const double* t, int V, int rows, int row_len, long row_stride,
                                      long point_stride, float max_view_error, int iters, int min_views, int ref_view, float max_reproj,
                                      float max_cos_parallax, float* points, float* depth, float* reproj, float* cos_parallax,
                                      unsigned* views, unsigned char* valid, void* stream) {
  ROMA_REQUIRE(obs && K && R && t, ROMA_E_ARG, "roma_triangulate_nview: null pointer");
  ROMA_REQUIRE(points || depth || reproj || cos_parallax || views || valid, ROMA_E_ARG, "roma_triangulate_nview: every output is null");
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "roma_triangulate_nview: bad shape V=%d (2 to %d views)", V, MAX_VIEWS);
  ROMA_REQUIRE(rows >= 1 && rows <= 65535 && row_len >= 1 && (long)rows * row_len <= (1L << 28), ROMA_E_SHAPE,
               "roma_triangulate_nview: bad shape rows=%d row_len=%d (1 to 65535 rows, 1 to 2^28 points in all)", rows, row_len);
  ROMA_REQUIRE(row_stride >= 0 && point_stride >= 2 && row_stride % 2 == 0 && point_stride % 2 == 0, ROMA_E_SHAPE,
               "roma_triangulate_nview: bad strides row_stride=%ld point_stride=%ld (floats: even, not negative, point_stride >= 2)",
               row_stride, point_stride);
  ROMA_REQUIRE(!visible || vis_row_stride >= 0, ROMA_E_SHAPE, "roma_triangulate_nview: bad strides vis_row_stride=%ld (not negative)",
               vis_row_stride);
  ROMA_REQUIRE(iters >= 0 && iters <= 10, ROMA_E_ARG, "roma_triangulate_nview: iters must be in [0, 10], got %d", iters);
  ROMA_REQUIRE(min_views >= 2 && min_views <= V, ROMA_E_ARG, "roma_triangulate_nview: min_views must be in [2, V=%d], got %d", V, min_views);
  ROMA_REQUIRE(ref_view >= 0 && ref_view < V, ROMA_E_ARG, "roma_triangulate_nview: ref_view must be in [0, V=%d), got %d", V, ref_view);
  ROMA_REQUIRE(!(max_reproj != max_reproj) && !(max_cos_parallax != max_cos_parallax) && !(max_view_error != max_view_error), ROMA_E_ARG,
               "roma_triangulate_nview: max_view_error, max_reproj and max_cos_parallax must not be NaN");
  ROMA_REQUIRE(max_view_error > 0.f, ROMA_E_ARG, "roma_triangulate_nview: max_view_error must be positive (+inf = every observed view), got %g",
               (double)max_view_error);
  ObsTable tab;
  if (int rc = fill_obs_table("roma_triangulate_nview", obs, to_px, visible, V, tab)) return rc;
  NviewParams prm;
  prm.V = V; prm.row_len = row_len; prm.iters = iters; prm.min_views = min_views; prm.ref_view = ref_view;
  prm.robust = max_view_error < __builtin_inff() ? 1 : 0;
  prm.row_stride = row_stride; prm.point_stride = point_stride; prm.vis_row_stride = visible ? vis_row_stride : 0;
  prm.thr2 = max_view_error * max_view_error; prm.max_reproj = max_reproj; prm.max_cos = max_cos_parallax;
  // the slab is sized by V: up to 64 KiB of dynamic LDS beside the static constants, above the default limit of a launch
  static std::atomic<uint64_t> attr_done{0};
  if (int rc = ensure_dyn_smem(reinterpret_cast<const void*>(triangulate_nview_kernel), MAX_VIEWS * THREADS * (int)sizeof(float2), attr_done,
                               "roma_triangulate_nview"))
    return rc;
  const dim3 grid((unsigned)((row_len + THREADS - 1) / THREADS), (unsigned)rows);
  hipLaunchKernelGGL(triangulate_nview_kernel, grid, dim3(THREADS), (size_t)V * THREADS * sizeof(float2), static_cast<hipStream_t>(stream), tab,
                     prm, K, R, t, points, depth, reproj, cos_parallax, views, valid);
  ROMA_CHECK_LAUNCH();
}
