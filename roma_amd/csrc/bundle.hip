// Bundle adjustment of one reconstruction: V posed views (2 <= V <= 32) and N points refined TOGETHER by Levenberg-Marquardt on the
// truncated reprojection cost, the cameras through the Schur complement of the points.  DESIGN.md §3.4, "Bundle adjustment";
// tests/bundle_ref.py restates the definition in numpy with the FULL normal equations.
//
// Convention (find_absolute_pose, triangulate_nview): x_v ~ K_v (R_v X + t_v).  fp64 throughout, and everything relative to c0, the
// mean of the centres of the usable views summed in view order: X' = X - c0, t'_v = t_v + R_v c0 (triangulate_nview's frame).
//   observed (v, n): the pixel is finite, visible[v][n] is set, view v is usable (K upper triangular, fx fy != 0, K R t finite), X[n]
//     is finite;  weighted: observed, depth > 0, squared pixel error e < threshold^2;  cost = sum over observed (weighted ? e : thr^2)
//   parameters: a free view has 6, R' = exp([w]x) R, t' = exp([w]x) t + tau; a point has 3
//   held: the views of `fixed`, the views that are not usable, a free view without a weighted observation (for that step); a point
//     with fewer than 2 weighted observations or a pivot of its damped 3 x 3 block that is not positive (for that step)
//   damping A + lambda diag A on camera and point blocks; schedule of twoview_math.h's refinements: lambda_0 = 1e-3, / 10 on a kept
//     step (floor 1e-10), * 10 otherwise, kept when cost' < cost (1 - 1e-12)
//
// The launches of one call, all on one stream; the kernel boundary is the only synchronisation between phases:
//   init (1 block)        usable views, c0, the centred poses, the state record {lambda, cost, cost0, steps, finished, status, cur}
//   centre (N threads)    X' = X - c0
//   evaluate + decide     the cost of the input
//   `iters` rounds of
//     accumulate          one wave per chunk of CHUNK = 64 points, at most MAX_PARTIALS = 256 blocks (a block walks its chunks in
//                         order).  Phase A, a thread per point: the weighted views, V_n = sum Jp^T Jp, g_p, the damped inverse.  Phase
//                         B, the chunk's points ONE AFTER THE OTHER, the wave's lanes over the entries of the point's contribution:
//                         lane v adds U_v = Jc^T Jc, -g_c and Y_v g_p (Y_v = W_v V*^-1, W_v = Jc^T Jp) to view v's diagonal block and
//                         right-hand side and leaves W_v, Y_v in LDS; then the lanes share the 36 entries of every pair (a >= b) of
//                         the point's free views: S_ab -= Y_a W_b^T.  Every entry of the block's partial system is added to by one
//                         lane at a time, the points in their order: a fixed order of the sums, no floating-point atomics
//     reduce              entry e of the system = its partials added in block order
//     solve (1 block)     the damped reduced system, at most 192 x 192 (held views are identity rows), as a packed lower triangle in
//                         LDS (148 KB at V = 32): right-looking Cholesky, pivot rule of solve_step (p > 0 and finite), two
//                         substitutions.  A pivot that fails ends the call: finished, the input comes back
//     propose             a thread per point: the point's equations again (W is recomputed, never stored), delta_p = V*^-1 (-g_p -
//                         sum_v W_v^T delta_c,v); block 0 moves the views.  The candidate goes to the other of two state buffers
//     evaluate + decide   the candidate's cost by per-block partial sums added in order; one thread keeps or rejects: cur ^= 1
//   final                 R, t, X, mask, count, cost, steps, status; what never moved is copied from the input bit for bit
// Every launch after init reads `finished` first and returns at once when it is set.  No block waits for another block: no flags, no
// spin loops, no cooperative grid; every loop has a trip count fixed by (V, N) before it starts.  `count` is summed with an integer
// atomic (it commutes).  No host synchronisation: the call can be captured in a graph.
#include "multiview.h"

namespace roma {
namespace {

constexpr int CHUNK = 64, MAX_PARTIALS = 256, POINT_THREADS = 256, SOLVE_THREADS = 256, REGIONS = 11;
constexpr double LAMBDA0 = 1e-3, LAMBDA_MIN = 1e-10, ACCEPT_REL = 1e-12;
constexpr int STATUS_PIVOT = 1, STATUS_NO_FREE_VIEW = 2, STATUS_NOT_FINITE = 4;

struct State {
  double lambda, cost, cost0;
  int steps, finished, status, cur;
};

struct ViewK {                     // constant over the call
  double k[5];                     // fx, s, cx, fy, cy
  double ok, free_, pad;
};
struct ViewP {                     // one of two buffers
  double R[9], t[3];
  double moved, pad[3];
};
static_assert(sizeof(ViewK) == 64 && sizeof(ViewP) == 128, "view records");

struct Ws {
  State* st;
  ViewK* vk;
  double* c0;                      // 3
  double* delta;                   // 6 V, then V flags: the view took part in the solve
  ViewP* vp[2];
  double* X[2];
  unsigned char* moved[2];
  double* sys;                     // M
  double* part;                    // P x M
  double* cpart;                   // P
};

struct Prm {
  int V, N, P, M, n;               // n = 6 V, M = n (n + 1) / 2 + 2 n + V: lower triangle, b, diag U, weighted observations per view
  long point_stride;
  double thr2;
  unsigned fixed;
};

// q = R X + t, the pixel residual and its square
struct Proj {
  double q0, q1, q2, iz, a, b, ru, rv, e;
};
__device__ __forceinline__ Proj project(const double* k, const double* R, const double* t, const double* X, double px, double py) {
  Proj o;
  o.q0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  o.q1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  o.q2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  o.iz = 1.0 / o.q2;
  o.a = o.q0 * o.iz;
  o.b = o.q1 * o.iz;
  o.ru = k[0] * o.a + k[1] * o.b + k[2] - px;
  o.rv = k[3] * o.b + k[4] - py;
  o.e = o.ru * o.ru + o.rv * o.rv;
  return o;
}

// the residual's derivatives by (w, tau) and by X: d q = w x q + tau + R dX
__device__ __forceinline__ void jacobians(const double* k, const double* R, const Proj& p, double (&Jc)[2][6], double (&Jp)[2][3]) {
  const double u0 = k[0] * p.iz, u1 = k[1] * p.iz, u2 = -(k[0] * p.a + k[1] * p.b) * p.iz;
  const double v1 = k[3] * p.iz, v2 = -(k[3] * p.b) * p.iz;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    Jp[0][j] = u0 * R[j] + u1 * R[3 + j] + u2 * R[6 + j];
    Jp[1][j] = v1 * R[3 + j] + v2 * R[6 + j];
  }
  Jc[0][0] = u2 * p.q1 - u1 * p.q2; Jc[0][1] = u0 * p.q2 - u2 * p.q0; Jc[0][2] = u1 * p.q0 - u0 * p.q1;
  Jc[1][0] = v2 * p.q1 - v1 * p.q2; Jc[1][1] = -v2 * p.q0;            Jc[1][2] = v1 * p.q0;
  Jc[0][3] = u0; Jc[0][4] = u1; Jc[0][5] = u2;
  Jc[1][3] = 0.0; Jc[1][4] = v1; Jc[1][5] = v2;
}

// inverse of A + lambda diag A, A symmetric 3 x 3 as (a00, a01, a02, a11, a12, a22), by Cholesky; false on a pivot that is not
// positive (solve_step's rule)
__device__ __forceinline__ bool damped_inverse3(const double* a, double lambda, double* inv) {
  const double p0 = a[0] + lambda * a[0];
  bool ok = p0 > 0.0 && isfinite(p0);
  const double l00 = sqrt(p0), l10 = a[1] / l00, l20 = a[2] / l00;
  const double p1 = (a[3] + lambda * a[3]) - l10 * l10;
  ok = ok && p1 > 0.0 && isfinite(p1);
  const double l11 = sqrt(p1), l21 = (a[4] - l20 * l10) / l11;
  const double p2 = (a[5] + lambda * a[5]) - l20 * l20 - l21 * l21;
  ok = ok && p2 > 0.0 && isfinite(p2);
  const double l22 = sqrt(p2);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double m10 = -l10 * i00 * i11, m21 = -l21 * i11 * i22, m20 = -(l20 * i00 + l21 * m10) * i22;
  inv[0] = i00 * i00 + m10 * m10 + m20 * m20;
  inv[1] = m10 * i11 + m20 * m21;
  inv[2] = m20 * i22;
  inv[3] = i11 * i11 + m21 * m21;
  inv[4] = m21 * i22;
  inv[5] = i22 * i22;
  return ok;
}

// per-view constants and the current pose, 20 doubles in LDS: k (5), R (9), t (3), usable, takes part in the camera system
struct ViewL {
  double k[5], R[9], t[3], ok, active, pad;
};
__device__ __forceinline__ void load_view(ViewL& o, const ViewK& vk, const ViewP& vp) {
#pragma unroll
  for (int i = 0; i < 5; ++i) o.k[i] = vk.k[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) o.R[i] = vp.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) o.t[i] = vp.t[i];
  o.ok = vk.ok;
  o.active = (vk.ok != 0.0 && vk.free_ != 0.0) ? 1.0 : 0.0;
  o.pad = 0.0;
}

// One point against every view: the weighted views, V = sum Jp^T Jp, g_p = sum Jp^T r, its truncated cost; with `delta`, also
// wd = sum over the views of the camera system of Jp^T (Jc delta_v)
struct PointEq {
  double Vm[6], gp[3], wd[3], cost;
  unsigned weighted, observed;
};
__device__ __forceinline__ PointEq point_equations(const ObsTable& tab, const ViewL* view, int V, long n, long stride, const double* X, double thr2,
                                                   const double* delta, bool equations) {
  PointEq o;
#pragma unroll
  for (int i = 0; i < 6; ++i) o.Vm[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { o.gp[i] = 0.0; o.wd[i] = 0.0; }
  o.cost = 0.0;
  o.weighted = 0;
  o.observed = 0;
  const bool fin = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
#pragma unroll 1
  for (int v = 0; v < V; ++v) {
    const ViewL& c = view[v];
    float px, py;
    const bool seen = load_px(tab, v, n, stride, px, py);
    if (!(seen && fin && c.ok != 0.0)) continue;
    const Proj p = project(c.k, c.R, c.t, X, (double)px, (double)py);
    const bool w = p.q2 > 0.0 && p.e < thr2;
    o.observed |= 1u << v;
    o.cost += w ? p.e : thr2;
    if (!w) continue;
    o.weighted |= 1u << v;
    if (!equations) continue;
    double Jc[2][6], Jp[2][3];
    jacobians(c.k, c.R, p, Jc, Jp);
    o.Vm[0] += Jp[0][0] * Jp[0][0] + Jp[1][0] * Jp[1][0]; o.Vm[1] += Jp[0][0] * Jp[0][1] + Jp[1][0] * Jp[1][1];
    o.Vm[2] += Jp[0][0] * Jp[0][2] + Jp[1][0] * Jp[1][2]; o.Vm[3] += Jp[0][1] * Jp[0][1] + Jp[1][1] * Jp[1][1];
    o.Vm[4] += Jp[0][1] * Jp[0][2] + Jp[1][1] * Jp[1][2]; o.Vm[5] += Jp[0][2] * Jp[0][2] + Jp[1][2] * Jp[1][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) o.gp[j] += Jp[0][j] * p.ru + Jp[1][j] * p.rv;
    if (delta && c.active != 0.0) {
      double d0 = 0.0, d1 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) { d0 += Jc[0][j] * delta[6 * v + j]; d1 += Jc[1][j] * delta[6 * v + j]; }
#pragma unroll
      for (int j = 0; j < 3; ++j) o.wd[j] += Jp[0][j] * d0 + Jp[1][j] * d1;
    }
  }
  return o;
}

// t + R c0: the translation in the frame centred at c0
__device__ __forceinline__ double centred_t(const double* R, const double* t, const double* c0, int j) {
  return t[j] + (R[3 * j] * c0[0] + R[3 * j + 1] * c0[1] + R[3 * j + 2] * c0[2]);
}

// --------------------------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(CHUNK) void bundle_init_kernel(Ws ws, Prm prm, const double* __restrict__ K, const double* __restrict__ R,
                                                            const double* __restrict__ t, int iters, int* __restrict__ count) {
  __shared__ double s_centre[MAX_VIEWS][3];
  __shared__ int s_ok[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V;
  if (tid < V) {
    const double* Kv = K + 9 * tid;
    const double* Rv = R + 9 * tid;
    const double* tv = t + 3 * tid;
    double ki[5];
    bool ok = invert_k(Kv, ki) && upper_triangular(Kv);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(Rv[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && isfinite(tv[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) s_centre[tid][j] = -(Rv[j] * tv[0] + Rv[3 + j] * tv[1] + Rv[6 + j] * tv[2]);
    s_ok[tid] = ok ? 1 : 0;
  }
  __syncthreads();
  if (tid < V) {
    double c0[3] = {0.0, 0.0, 0.0};
    int m = 0, free_usable = 0;
    for (int u = 0; u < V; ++u) {
      if (!s_ok[u]) continue;
      c0[0] += s_centre[u][0]; c0[1] += s_centre[u][1]; c0[2] += s_centre[u][2];
      ++m;
      if (!((prm.fixed >> u) & 1u)) ++free_usable;
    }
    if (m > 0) { c0[0] /= m; c0[1] /= m; c0[2] /= m; }
    const double* Kv = K + 9 * tid;
    const double* Rv = R + 9 * tid;
    const double* tv = t + 3 * tid;
    ViewK& k = ws.vk[tid];
    k.k[0] = Kv[0]; k.k[1] = Kv[1]; k.k[2] = Kv[2]; k.k[3] = Kv[4]; k.k[4] = Kv[5];
    k.ok = s_ok[tid] ? 1.0 : 0.0;
    k.free_ = ((prm.fixed >> tid) & 1u) ? 0.0 : 1.0;
    k.pad = 0.0;
    ViewP& p = ws.vp[0][tid];
#pragma unroll
    for (int i = 0; i < 9; ++i) p.R[i] = Rv[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) { p.t[j] = centred_t(Rv, tv, c0, j); p.pad[j] = 0.0; }
    p.moved = 0.0;
    if (tid == 0) {
      ws.c0[0] = c0[0]; ws.c0[1] = c0[1]; ws.c0[2] = c0[2];
      State& s = *ws.st;
      s.lambda = LAMBDA0; s.cost = 0.0; s.cost0 = 0.0; s.steps = 0; s.cur = 0;
      s.status = free_usable > 0 ? 0 : STATUS_NO_FREE_VIEW;
      s.finished = (iters == 0 || free_usable == 0) ? 1 : 0;
      *count = 0;
    }
  }
}

__global__ __launch_bounds__(POINT_THREADS) void bundle_centre_kernel(Ws ws, Prm prm, const double* __restrict__ X) {
  const long n = (long)blockIdx.x * POINT_THREADS + threadIdx.x;
  if (n >= prm.N) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) ws.X[0][3 * n + j] = X[3 * n + j] - ws.c0[j];
  ws.moved[0][n] = 0;
}

// ----------------------------------------------------------------------------------------------------------------- evaluate
// the truncated cost of the current state (candidate = 0) or of the candidate: block p's chunks in order into cpart[p]
__global__ __launch_bounds__(CHUNK) void bundle_evaluate_kernel(ObsTable tab, Ws ws, Prm prm, int candidate) {
  const State& st = *ws.st;
  if (candidate && st.finished) return;
  __shared__ ViewL s_view[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V, buf = st.cur ^ candidate;
  if (tid < V) load_view(s_view[tid], ws.vk[tid], ws.vp[buf][tid]);
  __syncthreads();
  const int nchunks = (prm.N + CHUNK - 1) / CHUNK;
  double total = 0.0;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long n = (long)chunk * CHUNK + tid;
    double c = 0.0;
    if (n < prm.N) {
      const double X[3] = {ws.X[buf][3 * n], ws.X[buf][3 * n + 1], ws.X[buf][3 * n + 2]};
      c = point_equations(tab, s_view, V, n, prm.point_stride, X, prm.thr2, nullptr, false).cost;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    total += c;
  }
  if (tid == 0) ws.cpart[blockIdx.x] = total;
}

// one thread: the partial costs in block order, then the cost of the input (candidate = 0) or keep / reject
__global__ void bundle_decide_kernel(Ws ws, Prm prm, int candidate) {
  State& st = *ws.st;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (candidate && st.finished) return;
  double c = 0.0;
  for (int p = 0; p < prm.P; ++p) c += ws.cpart[p];
  if (!candidate) {
    st.cost = c;
    st.cost0 = c;
    if (!isfinite(c)) { st.finished = 1; st.status |= STATUS_NOT_FINITE; }
    return;
  }
  if (c < st.cost * (1.0 - ACCEPT_REL)) {
    st.cost = c;
    st.cur ^= 1;
    st.steps += 1;
    st.lambda = fmax(st.lambda / 10.0, LAMBDA_MIN);
  } else {
    st.lambda *= 10.0;
  }
}

// --------------------------------------------------------------------------------------------------------------- accumulate
__global__ __launch_bounds__(CHUNK) void bundle_accumulate_kernel(ObsTable tab, Ws ws, Prm prm) {
  const State& st = *ws.st;
  if (st.finished) return;
  __shared__ ViewL s_view[MAX_VIEWS];
  __shared__ double s_pt[CHUNK][12];                 // X (3), the damped inverse (6), g_p (3)
  __shared__ unsigned s_w[CHUNK];
  __shared__ int s_held[CHUNK];
  __shared__ double s_W[MAX_VIEWS][18], s_Y[MAX_VIEWS][18];
  __shared__ int s_list[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V, n6 = prm.n, cur = st.cur;
  const double lambda = st.lambda;
  const int boff = tri(n6), udoff = boff + n6, nwoff = udoff + n6;
  if (tid < V) load_view(s_view[tid], ws.vk[tid], ws.vp[cur][tid]);
  double* part = ws.part + (size_t)blockIdx.x * prm.M;
  for (int e = tid; e < prm.M; e += CHUNK) part[e] = 0.0;
  __syncthreads();
  unsigned active = 0;
  for (int v = 0; v < V; ++v) active |= (s_view[v].active != 0.0 ? 1u : 0u) << v;
  const int nchunks = (prm.N + CHUNK - 1) / CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    // ---- phase A: a thread per point
    const long n = (long)chunk * CHUNK + tid;
    unsigned w = 0;
    int held = 1;
    if (n < prm.N) {
      const double X[3] = {ws.X[cur][3 * n], ws.X[cur][3 * n + 1], ws.X[cur][3 * n + 2]};
      const PointEq q = point_equations(tab, s_view, V, n, prm.point_stride, X, prm.thr2, nullptr, true);
      double inv[6];
      const bool ok = damped_inverse3(q.Vm, lambda, inv);
      w = q.weighted;
      held = (__popc(w) < 2 || !ok) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) { s_pt[tid][j] = X[j]; s_pt[tid][9 + j] = q.gp[j]; }
#pragma unroll
      for (int j = 0; j < 6; ++j) s_pt[tid][3 + j] = inv[j];
    }
    s_w[tid] = w;
    s_held[tid] = held;
    __syncthreads();
    // ---- phase B: the chunk's points in order
    const int in_chunk = min(CHUNK, prm.N - chunk * CHUNK);
    for (int i = 0; i < in_chunk; ++i) {
      const unsigned act = s_w[i] & active;
      if (!act) continue;                                                     // the same for every lane
      const long ni = (long)chunk * CHUNK + i;
      const int held_i = s_held[i];
      if (tid < V && ((act >> tid) & 1u)) {
        const ViewL& c = s_view[tid];
        float px, py;
        load_px(tab, tid, ni, prm.point_stride, px, py);
        const Proj p = project(c.k, c.R, c.t, s_pt[i], (double)px, (double)py);
        double Jc[2][6], Jp[2][3];
        jacobians(c.k, c.R, p, Jc, Jp);
        const int r0 = 6 * tid;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int s = 0; s <= r; ++s) part[tri(r0 + r) + r0 + s] += Jc[0][r] * Jc[0][s] + Jc[1][r] * Jc[1][s];
          part[udoff + r0 + r] += Jc[0][r] * Jc[0][r] + Jc[1][r] * Jc[1][r];
          part[boff + r0 + r] += -(Jc[0][r] * p.ru + Jc[1][r] * p.rv);
        }
        part[nwoff + tid] += 1.0;
        double W[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            W[r][k] = Jc[0][r] * Jp[0][k] + Jc[1][r] * Jp[1][k];
            s_W[tid][3 * r + k] = W[r][k];
          }
        if (!held_i) {
          const double* inv = &s_pt[i][3];
          const double* gp = &s_pt[i][9];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double y[3];
            sym3_times(inv, W[r], y);
            s_Y[tid][3 * r] = y[0]; s_Y[tid][3 * r + 1] = y[1]; s_Y[tid][3 * r + 2] = y[2];
            part[boff + r0 + r] += y[0] * gp[0] + y[1] * gp[1] + y[2] * gp[2];
          }
        }
        s_list[__popc(act & ((1u << tid) - 1u))] = tid;
      }
      __syncthreads();
      if (!held_i) {
        const int ma = __popc(act), items = tri(ma) * 36;
        for (int item = tid; item < items; item += CHUNK) {
          const int pair = item / 36, e = item - 36 * pair, r = e / 6, s = e - 6 * r;
          int ja = 0;
          while (ja < MAX_VIEWS - 1 && tri(ja + 1) <= pair) ++ja;
          const int jb = pair - tri(ja);
          if (ja == jb && s > r) continue;
          const int a = s_list[ja], b = s_list[jb];                           // a >= b: the list ascends
          const double* y = &s_Y[a][3 * r];
          const double* wb = &s_W[b][3 * s];
          part[tri(6 * a + r) + 6 * b + s] -= y[0] * wb[0] + y[1] * wb[1] + y[2] * wb[2];
        }
      }
      __syncthreads();
    }
    __syncthreads();                                                          // phase A of the next chunk overwrites s_pt, s_w
  }
}

__global__ __launch_bounds__(POINT_THREADS) void bundle_reduce_kernel(Ws ws, Prm prm) {
  if (ws.st->finished) return;
  reduce_partials(ws.part, ws.sys, prm.M, prm.P, blockIdx.x * POINT_THREADS + threadIdx.x);
}

// -------------------------------------------------------------------------------------------------------------------- solve
__global__ __launch_bounds__(SOLVE_THREADS) void bundle_solve_kernel(Ws ws, Prm prm) {
  State& st = *ws.st;
  if (st.finished) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* L = reinterpret_cast<double*>(smem);       // packed lower triangle, row i at tri(i)
  __shared__ double s_rhs[6 * MAX_VIEWS];
  __shared__ int s_active[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V, n = prm.n;
  const int boff = tri(n), udoff = boff + n, nwoff = udoff + n;
  const double lambda = st.lambda;
  if (tid < V) s_active[tid] = (ws.vk[tid].ok != 0.0 && ws.vk[tid].free_ != 0.0 && ws.sys[nwoff + tid] > 0.0) ? 1 : 0;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int ai = s_active[i / 6];
    for (int j = tid; j <= i; j += SOLVE_THREADS) {
      double v = ws.sys[tri(i) + j];
      if (!(ai && s_active[j / 6])) v = i == j ? 1.0 : 0.0;
      else if (i == j) v += lambda * ws.sys[udoff + i];
      L[tri(i) + j] = v;
    }
  }
  if (tid < n) s_rhs[tid] = s_active[tid / 6] ? ws.sys[boff + tid] : 0.0;
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    const double p = L[tri(j) + j];
    if (!(p > 0.0 && isfinite(p))) { ok = false; break; }                     // the same for every thread
    const double d = sqrt(p);
    __syncthreads();
    const int i = j + tid;
    if (i == j) L[tri(j) + j] = d;
    else if (i < n) L[tri(i) + j] /= d;
    __syncthreads();
    if (i > j && i < n) {
      const double lij = L[tri(i) + j];
      for (int k = j + 1; k <= i; ++k) L[tri(i) + k] -= lij * L[tri(k) + j];
    }
  }
  if (!ok) {
    if (tid == 0) { st.finished = 1; st.status |= STATUS_PIVOT; }
    return;
  }
  for (int j = 0; j < n; ++j) {                                                // L y = b
    __syncthreads();
    const double y = s_rhs[j] / L[tri(j) + j];
    __syncthreads();
    const int i = j + tid;
    if (i == j) s_rhs[j] = y;
    else if (i < n) s_rhs[i] -= L[tri(i) + j] * y;
  }
  for (int j = n - 1; j >= 0; --j) {                                           // L^T x = y
    __syncthreads();
    const double x = s_rhs[j] / L[tri(j) + j];
    __syncthreads();
    if (tid == j) s_rhs[j] = x;
    else if (tid < j) s_rhs[tid] -= L[tri(j) + tid] * x;
  }
  __syncthreads();
  if (tid < n) ws.delta[tid] = s_rhs[tid];
  if (tid < V) ws.delta[n + tid] = s_active[tid] ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------ propose
__global__ __launch_bounds__(POINT_THREADS) void bundle_propose_kernel(ObsTable tab, Ws ws, Prm prm) {
  const State& st = *ws.st;
  if (st.finished) return;
  __shared__ ViewL s_view[MAX_VIEWS];
  __shared__ double s_delta[6 * MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V, cur = st.cur, nxt = cur ^ 1;
  if (tid < V) {
    load_view(s_view[tid], ws.vk[tid], ws.vp[cur][tid]);
    if (ws.delta[prm.n + tid] == 0.0) s_view[tid].active = 0.0;               // held for this step
  }
  if (tid < prm.n) s_delta[tid] = ws.delta[tid];
  __syncthreads();
  if (blockIdx.x == 0 && tid < V) {
    const ViewL& c = s_view[tid];
    ViewP& o = ws.vp[nxt][tid];
    if (c.active == 0.0) {
      o = ws.vp[cur][tid];
    } else {
      double w[3] = {s_delta[6 * tid], s_delta[6 * tid + 1], s_delta[6 * tid + 2]};
      double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
      if (th2 > 1.0) {
        const double sc = 1.0 / sqrt(th2);
        w[0] *= sc; w[1] *= sc; w[2] *= sc;
        th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
      }
      double A, B;
      so3_exp_series(th2, A, B, So3Literals());
      // E = I + A [w]x + B [w]x^2.  The step and the Gram-Schmidt are written out here: profiles/multiview_shared_code_micro.txt
      const double Kx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
      double E[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const double k2 = Kx[3 * r] * Kx[s] + Kx[3 * r + 1] * Kx[3 + s] + Kx[3 * r + 2] * Kx[6 + s];
          E[3 * r + s] = (r == s ? 1.0 : 0.0) + A * Kx[3 * r + s] + B * k2;
        }
      double M[9], tn[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int s = 0; s < 3; ++s) M[3 * r + s] = E[3 * r] * c.R[s] + E[3 * r + 1] * c.R[3 + s] + E[3 * r + 2] * c.R[6 + s];
        tn[r] = (E[3 * r] * c.t[0] + E[3 * r + 1] * c.t[1] + E[3 * r + 2] * c.t[2]) + s_delta[6 * tid + 3 + r];
      }
      // Gram-Schmidt on the rows: r0, r1 made orthogonal to r0, r2 = r0 x r1
      const double i0 = 1.0 / sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
      const double r0[3] = {M[0] * i0, M[1] * i0, M[2] * i0};
      const double d = r0[0] * M[3] + r0[1] * M[4] + r0[2] * M[5];
      double r1[3] = {M[3] - d * r0[0], M[4] - d * r0[1], M[5] - d * r0[2]};
      const double i1 = 1.0 / sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
      r1[0] *= i1; r1[1] *= i1; r1[2] *= i1;
      double r2[3];
      cross3(r0, r1, r2);
#pragma unroll
      for (int j = 0; j < 3; ++j) { o.R[j] = r0[j]; o.R[3 + j] = r1[j]; o.R[6 + j] = r2[j]; o.t[j] = tn[j]; o.pad[j] = 0.0; }
      o.moved = 1.0;
    }
  }
  const long n = (long)blockIdx.x * POINT_THREADS + tid;
  if (n >= prm.N) return;
  const double X[3] = {ws.X[cur][3 * n], ws.X[cur][3 * n + 1], ws.X[cur][3 * n + 2]};
  const PointEq q = point_equations(tab, s_view, V, n, prm.point_stride, X, prm.thr2, s_delta, true);
  double inv[6];
  const bool ok = damped_inverse3(q.Vm, st.lambda, inv);
  const bool held = __popc(q.weighted) < 2 || !ok;
  double step[3] = {0.0, 0.0, 0.0};
  if (!held) {
    const double rhs[3] = {-q.gp[0] - q.wd[0], -q.gp[1] - q.wd[1], -q.gp[2] - q.wd[2]};
    sym3_times(inv, rhs, step);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) ws.X[nxt][3 * n + j] = held ? X[j] : X[j] + step[j];
  ws.moved[nxt][n] = held ? ws.moved[cur][n] : 1;
}

// -------------------------------------------------------------------------------------------------------------------- final
__global__ __launch_bounds__(POINT_THREADS) void bundle_final_kernel(ObsTable tab, Ws ws, Prm prm, const double* __restrict__ R_in,
                                                                     const double* __restrict__ t_in, const double* __restrict__ X_in,
                                                                     double* __restrict__ R, double* __restrict__ t, double* __restrict__ X,
                                                                     unsigned char* __restrict__ mask, double* __restrict__ cost,
                                                                     int* __restrict__ count, int* __restrict__ steps, int* __restrict__ status) {
  const State& st = *ws.st;
  __shared__ ViewL s_view[MAX_VIEWS];
  __shared__ int s_count;
  const int tid = threadIdx.x, V = prm.V, cur = st.cur;
  const bool input = st.steps == 0 || (st.status & STATUS_PIVOT) != 0;         // the caller gets the input back
  const double c0[3] = {ws.c0[0], ws.c0[1], ws.c0[2]};
  if (tid == 0) s_count = 0;
  if (tid < V) {
    ViewP p = ws.vp[cur][tid];
    const bool same = input || p.moved == 0.0;
    if (same) {
#pragma unroll
      for (int i = 0; i < 9; ++i) p.R[i] = R_in[9 * tid + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) p.t[j] = centred_t(R_in + 9 * tid, t_in + 3 * tid, c0, j);
    }
    load_view(s_view[tid], ws.vk[tid], p);
    if (blockIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) R[9 * tid + i] = same ? R_in[9 * tid + i] : p.R[i];
#pragma unroll
      for (int j = 0; j < 3; ++j)
        t[3 * tid + j] = same ? t_in[3 * tid + j] : p.t[j] - (p.R[3 * j] * c0[0] + p.R[3 * j + 1] * c0[1] + p.R[3 * j + 2] * c0[2]);
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    cost[0] = st.cost0;
    cost[1] = input ? st.cost0 : st.cost;
    *steps = input ? 0 : st.steps;
    *status = st.status;
  }
  __syncthreads();
  const long n = (long)blockIdx.x * POINT_THREADS + tid;
  int mine = 0;
  if (n < prm.N) {
    const bool same = input || ws.moved[cur][n] == 0;
    double Xc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Xc[j] = same ? X_in[3 * n + j] - c0[j] : ws.X[cur][3 * n + j];
      X[3 * n + j] = same ? X_in[3 * n + j] : Xc[j] + c0[j];
    }
    const unsigned w = point_equations(tab, s_view, V, n, prm.point_stride, Xc, prm.thr2, nullptr, false).weighted;
    for (int v = 0; v < V; ++v) mask[(size_t)v * prm.N + n] = (w >> v) & 1u;
    mine = __popc(w);
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (tid == 0 && s_count) atomicAdd(count, s_count);
}

// bytes of the workspace and the offsets of its REGIONS regions, each 256-byte aligned
long layout(int V, int N, long* off) {
  const long n = 6L * V, M = n * (n + 1) / 2 + 2 * n + V;
  const long P = std::min<long>(((long)N + CHUNK - 1) / CHUNK, MAX_PARTIALS);
  const long bytes[REGIONS] = {(long)sizeof(State), (long)sizeof(ViewK) * MAX_VIEWS, 8L * (3 + 7 * MAX_VIEWS), (long)sizeof(ViewP) * MAX_VIEWS,
                               (long)sizeof(ViewP) * MAX_VIEWS, 24L * N, 24L * N, 2L * N, 8 * M, 8 * M * P, 8 * P};
  return layout_regions(bytes, REGIONS, off);
}

int check_shape(const char* fn, int V, int N) {
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "%s: bad shape V=%d (2 to %d views)", fn, V, MAX_VIEWS);
  ROMA_REQUIRE(N >= 1 && N <= (1 << 24), ROMA_E_SHAPE, "%s: bad shape N=%d (1 to 2^24 points)", fn, N);
  return 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_bundle_workspace(int V, int N, long* offsets) {
  if (int rc = check_shape("roma_bundle_workspace", V, N)) return rc;
  return layout(V, N, offsets);
}

extern "C" int roma_bundle_adjust(const float* const* obs, const float* to_px, const unsigned char* const* visible, long point_stride,
                                  const double* K, const double* R_in, const double* t_in, const double* X_in, int V, int N, unsigned fixed,
                                  double threshold, int iters, double* R, double* t, double* X, unsigned char* mask, double* cost, int* count,
                                  int* steps, int* status, void* workspace, long workspace_size, void* stream) {
  ROMA_REQUIRE(obs && K && R_in && t_in && X_in && R && t && X && mask && cost && count && steps && status && workspace, ROMA_E_ARG,
               "roma_bundle_adjust: null pointer");
  if (int rc = check_shape("roma_bundle_adjust", V, N)) return rc;
  ROMA_REQUIRE(point_stride >= 2 && point_stride % 2 == 0, ROMA_E_SHAPE,
               "roma_bundle_adjust: bad strides point_stride=%ld (floats: even, at least 2)", point_stride);
  ROMA_REQUIRE(threshold > 0.0 && threshold < 1e18, ROMA_E_ARG, "roma_bundle_adjust: threshold must be positive, got %g", threshold);
  ROMA_REQUIRE(iters >= 0 && iters <= 50, ROMA_E_ARG, "roma_bundle_adjust: iters must be in [0, 50], got %d", iters);
  const unsigned all = V == 32 ? 0xffffffffu : (1u << V) - 1u;
  ROMA_REQUIRE((fixed & ~all) == 0 && fixed != 0, ROMA_E_ARG, "roma_bundle_adjust: fixed=0x%x must name at least one of the V=%d views and no other",
               fixed, V);
  ROMA_REQUIRE(fixed != all, ROMA_E_ARG, "roma_bundle_adjust: fixed=0x%x holds every view: nothing to refine", fixed);
  long off[REGIONS];
  const long need = layout(V, N, off);
  ROMA_REQUIRE(workspace_size >= need, ROMA_E_ARG, "roma_bundle_adjust: workspace of %ld bytes, roma_bundle_workspace asks for %ld", workspace_size,
               need);
  ROMA_REQUIRE(aligned16(workspace) && aligned16(K) && aligned16(R_in) && aligned16(t_in) && aligned16(X_in) && aligned16(R) && aligned16(t) &&
                   aligned16(X) && aligned16(cost),
               ROMA_E_ALIGN, "roma_bundle_adjust: workspace, K, R_in, t_in, X_in, R, t, X and cost must be 16-byte aligned");
  ROMA_REQUIRE(aligned4(count) && aligned4(steps) && aligned4(status), ROMA_E_ALIGN,
               "roma_bundle_adjust: count, steps and status must be 4-byte aligned");
  ObsTable tab;
  if (int rc = fill_obs_table("roma_bundle_adjust", obs, to_px, visible, V, tab)) return rc;
  Prm prm;
  prm.V = V; prm.N = N; prm.n = 6 * V; prm.M = tri(prm.n) + 2 * prm.n + V;
  prm.P = std::min((N + CHUNK - 1) / CHUNK, MAX_PARTIALS);
  prm.point_stride = point_stride; prm.thr2 = threshold * threshold; prm.fixed = fixed;
  char* base = static_cast<char*>(workspace);
  Ws ws;
  ws.st = reinterpret_cast<State*>(base + off[0]);
  ws.vk = reinterpret_cast<ViewK*>(base + off[1]);
  ws.c0 = reinterpret_cast<double*>(base + off[2]);
  ws.delta = ws.c0 + 3;
  ws.vp[0] = reinterpret_cast<ViewP*>(base + off[3]);
  ws.vp[1] = reinterpret_cast<ViewP*>(base + off[4]);
  ws.X[0] = reinterpret_cast<double*>(base + off[5]);
  ws.X[1] = reinterpret_cast<double*>(base + off[6]);
  ws.moved[0] = reinterpret_cast<unsigned char*>(base + off[7]);
  ws.moved[1] = ws.moved[0] + N;
  ws.sys = reinterpret_cast<double*>(base + off[8]);
  ws.part = reinterpret_cast<double*>(base + off[9]);
  ws.cpart = reinterpret_cast<double*>(base + off[10]);

  const int solve_lds = tri(prm.n) * (int)sizeof(double);
  static std::atomic<uint64_t> attr_done{0};
  if (iters > 0)
    if (int rc = ensure_dyn_smem(reinterpret_cast<const void*>(bundle_solve_kernel), tri(6 * MAX_VIEWS) * (int)sizeof(double), attr_done,
                                 "roma_bundle_adjust"))
      return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 chunk_grid((unsigned)prm.P), chunk_block(CHUNK), point_grid((unsigned)((N + POINT_THREADS - 1) / POINT_THREADS)),
      point_block(POINT_THREADS), one(1);
  hipLaunchKernelGGL(bundle_init_kernel, one, chunk_block, 0, s, ws, prm, K, R_in, t_in, iters, count);
  hipLaunchKernelGGL(bundle_centre_kernel, point_grid, point_block, 0, s, ws, prm, X_in);
  hipLaunchKernelGGL(bundle_evaluate_kernel, chunk_grid, chunk_block, 0, s, tab, ws, prm, 0);
  hipLaunchKernelGGL(bundle_decide_kernel, one, chunk_block, 0, s, ws, prm, 0);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(bundle_accumulate_kernel, chunk_grid, chunk_block, 0, s, tab, ws, prm);
    hipLaunchKernelGGL(bundle_reduce_kernel, dim3((unsigned)((prm.M + POINT_THREADS - 1) / POINT_THREADS)), point_block, 0, s, ws, prm);
    hipLaunchKernelGGL(bundle_solve_kernel, one, dim3(SOLVE_THREADS), (size_t)solve_lds, s, ws, prm);
    hipLaunchKernelGGL(bundle_propose_kernel, point_grid, point_block, 0, s, tab, ws, prm);
    hipLaunchKernelGGL(bundle_evaluate_kernel, chunk_grid, chunk_block, 0, s, tab, ws, prm, 1);
    hipLaunchKernelGGL(bundle_decide_kernel, one, chunk_block, 0, s, ws, prm, 1);
  }
  hipLaunchKernelGGL(bundle_final_kernel, point_grid, point_block, 0, s, tab, ws, prm, R_in, t_in, X_in, R, t, X, mask, cost, count, steps, status);
  ROMA_CHECK_LAUNCH();
}
