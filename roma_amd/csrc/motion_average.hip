// Motion averaging: the V cameras of one reconstruction (V <= 32) from the pairwise poses of its pose graph and its tracks, the start that
// bundle.hip polishes.  DESIGN.md §3.4, "Motion averaging"; include/roma_hip.h has the definition and tests/motion_ref.py restates it.
//
// Conventions: a view is x_v ~ K_v (R_v X + t_v) (triangulate_nview, bundle); edge m, pairs[m] = (a, b), carries X_b = R_rel X_a + t_rel
// (estimate_pose).  fp64 throughout.
//
// roma_rotation_average — ONE launch of ONE workgroup (32 views x 4 slices of the edges): the maximum-weight spanning tree from the root,
// then `iters` rounds of re-weighted least squares on the Lie algebra: thread (v, s) walks the edges m = s, s + 4, ... that touch view v
// and adds them to its copy of row v of the weighted graph Laplacian (LDS), the four copies are added in order, the block factors the
// matrix (at most 31 x 31, three right-hand sides) by Cholesky and moves the views.
//
// roma_global_positions — the launches of one call, all on one stream; the kernel boundary is the only synchronisation:
//   init (1 block)        usable views, their constants, the edges' baseline directions, the state record
//   vote                  a thread per point: the round-0 weights as a bit per view (bearings and counters in LDS, the edges in order)
//   `rounds` rounds of
//     accumulate          one wave per chunk of CHUNK = 64 points, at most MAX_PARTIALS = 256 blocks (a block walks its chunks in order).
//                         The chunk's pixels are staged in LDS, then its points ONE AFTER THE OTHER, lane v = view v: the weight, Q_v =
//                         w P, A = sum Q_v in view order, solved or not, Y_v = Q_v A^-1; then the lanes share the 9 entries of every
//                         pair (a >= b) of the point's weighted views: S_ab -= Y_a Q_b.  The block's partial matrix (packed lower
//                         triangle, 3 V rows) lives in LDS; every entry is added to by one lane at a time, the points in their order
//     reduce              entry e of the matrix = its partials added in block order
//     solve (1 block)     the rows of the placed views without the root, at most 93 (padded to an even count), as a full matrix beside
//                         its eigenvectors in LDS (141 KB at V = 32): two-sided Jacobi in the round-robin order (n / 2 disjoint
//                         rotations at a time), until the off-diagonal part is below 1e-16 of the diagonal or SWEEPS sweeps
//     points              a thread per point: the weights again, X = A^-1 sum Q_v C_v, the block's sum of w depth
//     sign (1 block)      the partial sums in block order; C and (through the state record) X change sign when the sum is negative
//   final                 the weights after the last round: mask, count; points, centres, t, eigenvalues, status
// The weights are never stored: a weight is a function of the previous round's points and centres, evaluated by the same inlined code
// under `fp contract(off)` wherever it is needed, so every pass sees the same bits.  No floating-point atomics (count uses an integer
// one), no block waits for another, no host synchronisation: bitwise reproducible, and the call can be captured in a graph.
#include "twoview_math.h"

#pragma clang fp contract(off)

// after the pragma: the functions of multiview.h are this file's own code and must round as it does (no multiply fused with an add);
// before it they would be contracted, and the results are pinned to tests/motion_ref.py bit for bit
#include "multiview.h"

namespace roma {
namespace {

constexpr int MAX_EDGES = 4096, CHUNK = 64, MAX_PARTIALS = 256, POINT_THREADS = 256, MAX_POINT_BLOCKS = 1024, SOLVE_THREADS = 1024;
constexpr int ROT_SLICES = 4, ROT_THREADS = MAX_VIEWS * ROT_SLICES, ROT_LD = 36, SWEEPS = 16, REGIONS = 11;
constexpr int ROT_STATUS_PIVOT = 1;
constexpr int STATUS_EIGEN = 1, STATUS_UNPLACED = 2, STATUS_TOO_FEW = 4;

// ================================================================================================================= rotations
// r = log(Rb^T Rrel Ra) and its length
__device__ __forceinline__ double edge_residual(const double* Ra, const double* Rb, const double* Rrel, double* r) {
  double T[9], D[9];                                                           // T = Rrel Ra, D = Rb^T T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[3 * i + j] = Rrel[3 * i] * Ra[j] + Rrel[3 * i + 1] * Ra[3 + j] + Rrel[3 * i + 2] * Ra[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = Rb[i] * T[j] + Rb[3 + i] * T[3 + j] + Rb[6 + i] * T[6 + j];
  const double w[3] = {0.5 * (D[7] - D[5]), 0.5 * (D[2] - D[6]), 0.5 * (D[3] - D[1])};
  const double s = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double th = atan2(s, 0.5 * (D[0] + D[4] + D[8] - 1.0));
  const double f = s < 1e-12 ? 1.0 : th / s;
  r[0] = w[0] * f; r[1] = w[1] * f; r[2] = w[2] * f;
  return sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
}

// R <- rows of (R exp([w]x)) made orthonormal.  The step matrix and the Gram-Schmidt (twoview_math.h's orthonormalise_rows) are written
// out: here they must not be contracted, and the header is included before the pragma (profiles/multiview_shared_code_isa.txt)
__device__ __forceinline__ void rotate_right(double* R, const double* delta) {
  double w[3] = {delta[0], delta[1], delta[2]};
  double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 > 1.0) {
    const double sc = 1.0 / sqrt(th2);
    w[0] *= sc; w[1] *= sc; w[2] *= sc;
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  }
  double A, B;
  so3_exp_series(th2, A, B, So3Literals());
  const double Kx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9], M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const double k2 = Kx[3 * r] * Kx[s] + Kx[3 * r + 1] * Kx[3 + s] + Kx[3 * r + 2] * Kx[6 + s];
      E[3 * r + s] = (r == s ? 1.0 : 0.0) + A * Kx[3 * r + s] + B * k2;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) M[3 * r + s] = R[3 * r] * E[s] + R[3 * r + 1] * E[3 + s] + R[3 * r + 2] * E[6 + s];
  const double i0 = 1.0 / sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
  const double r0[3] = {M[0] * i0, M[1] * i0, M[2] * i0};
  const double d = r0[0] * M[3] + r0[1] * M[4] + r0[2] * M[5];
  double r1[3] = {M[3] - d * r0[0], M[4] - d * r0[1], M[5] - d * r0[2]};
  const double i1 = 1.0 / sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
  r1[0] *= i1; r1[1] *= i1; r1[2] *= i1;
  double r2[3];
  cross3(r0, r1, r2);
#pragma unroll
  for (int j = 0; j < 3; ++j) { R[j] = r0[j]; R[3 + j] = r1[j]; R[6 + j] = r2[j]; }
}

// `residual` doubles as the edge flags while the kernel runs: NaN = not usable, anything else = usable
__global__ __launch_bounds__(ROT_THREADS) void rotation_average_kernel(const double* __restrict__ R_rel, const int* __restrict__ pairs,
                                                                        const double* __restrict__ weights, int V, int M, int root,
                                                                        double sigma2, int iters, double* __restrict__ R_out,
                                                                        unsigned char* __restrict__ valid_out, double* residual,
                                                                        int* __restrict__ status_out) {
  __shared__ double s_R[MAX_VIEWS][9], s_R0[MAX_VIEWS][9];
  __shared__ double s_Lp[ROT_SLICES][MAX_VIEWS][ROT_LD];                        // row v: L[v][0 .. V), the right-hand sides at 32 .. 34
  __shared__ double s_L[MAX_VIEWS][MAX_VIEWS + 1], s_rhs[MAX_VIEWS][3];
  __shared__ double s_bw[ROT_THREADS];
  __shared__ int s_bm[ROT_THREADS];
  __shared__ int s_valid[MAX_VIEWS], s_unk[MAX_VIEWS], s_n, s_go, s_fail;
  const int tid = threadIdx.x, v = tid / ROT_SLICES, sl = tid % ROT_SLICES;
  const double nan = __builtin_nan("");
  for (int m = tid; m < M; m += ROT_THREADS) {
    const int a = pairs[2 * m], b = pairs[2 * m + 1];
    const double w = weights ? weights[m] : 1.0;
    bool ok = a != b && a >= 0 && a < V && b >= 0 && b < V && isfinite(w) && w > 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(R_rel[9 * (size_t)m + i]);
    residual[m] = ok ? 0.0 : nan;
  }
  if (tid < MAX_VIEWS) {
    s_valid[tid] = tid == root ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s_R[tid][i] = tid == root ? ((i & 3) == 0 ? 1.0 : 0.0) : nan;
  }
  __syncthreads();
  // ---- the spanning tree: at most V - 1 edges, each the heaviest usable edge that leaves the tree (lowest index on a tie)
  for (int step = 0; step < V - 1; ++step) {
    double bw = 0.0;
    int bm = -1;
    for (int m = tid; m < M; m += ROT_THREADS) {
      if (isnan(residual[m])) continue;
      const int a = pairs[2 * m], b = pairs[2 * m + 1];
      const double w = weights ? weights[m] : 1.0;
      if (s_valid[a] != s_valid[b] && (bm < 0 || w > bw)) { bw = w; bm = m; }
    }
    s_bw[tid] = bw;
    s_bm[tid] = bm;
    __syncthreads();
    if (tid == 0) {
      int best = -1;
      double w = 0.0;
      for (int i = 0; i < ROT_THREADS; ++i) {
        const int m = s_bm[i];
        if (m >= 0 && (best < 0 || s_bw[i] > w || (s_bw[i] == w && m < best))) { best = m; w = s_bw[i]; }
      }
      s_go = best;
      if (best >= 0) {
        const int a = pairs[2 * best], b = pairs[2 * best + 1];
        const double* Q = R_rel + 9 * (size_t)best;
        if (s_valid[a]) {
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) s_R[b][3 * i + j] = Q[3 * i] * s_R[a][j] + Q[3 * i + 1] * s_R[a][3 + j] + Q[3 * i + 2] * s_R[a][6 + j];
          s_valid[b] = 1;
        } else {
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) s_R[a][3 * i + j] = Q[i] * s_R[b][j] + Q[3 + i] * s_R[b][3 + j] + Q[6 + i] * s_R[b][6 + j];
          s_valid[a] = 1;
        }
      }
    }
    __syncthreads();
    if (s_go < 0) break;                                                        // the same for every thread
  }
  if (tid == 0) {
    int n = 0;
    for (int u = 0; u < V; ++u)
      if (s_valid[u] && u != root) s_unk[n++] = u;
    s_n = n;
    s_fail = 0;
  }
  if (tid < MAX_VIEWS)
#pragma unroll
    for (int i = 0; i < 9; ++i) s_R0[tid][i] = s_R[tid][i];
  __syncthreads();
  const int n = s_n;
  // ---- the rounds
  for (int it = 0; it < iters && n > 0; ++it) {
    double* row = s_Lp[sl][v];
    for (int i = 0; i < ROT_LD; ++i) row[i] = 0.0;
    if (v < V && s_valid[v]) {
      for (int m = sl; m < M; m += ROT_SLICES) {
        const int a = pairs[2 * m], b = pairs[2 * m + 1];
        if ((a != v && b != v) || isnan(residual[m]) || !s_valid[a] || !s_valid[b]) continue;
        double r[3];
        const double nr = edge_residual(s_R[a], s_R[b], R_rel + 9 * (size_t)m, r);
        const double w = weights ? weights[m] : 1.0;
        double om;
        if (it < iters / 2) {
          om = w / fmax(nr, 1e-3);
        } else {
          const double q = sigma2 / (sigma2 + nr * nr);
          om = w * (q * q);
        }
        const double sg = v == b ? 1.0 : -1.0;
        row[v] += om;
        row[v == b ? a : b] -= om;
        row[32] += sg * (om * r[0]); row[33] += sg * (om * r[1]); row[34] += sg * (om * r[2]);
      }
    }
    __syncthreads();
    for (int e = tid; e < n * (n + 3); e += ROT_THREADS) {                      // the unknowns' rows and columns, the slices in order
      const int i = e / (n + 3), j = e - i * (n + 3);
      const int c = j < n ? s_unk[j] : 32 + (j - n);
      double acc = s_Lp[0][s_unk[i]][c];
#pragma unroll
      for (int q = 1; q < ROT_SLICES; ++q) acc += s_Lp[q][s_unk[i]][c];
      if (j < n) s_L[i][j] = acc; else s_rhs[i][j - n] = acc;
    }
    // right-looking Cholesky, pivot rule of solve_step, then the two substitutions on the three right-hand sides
    for (int j = 0; j < n; ++j) {
      __syncthreads();
      const double p = s_L[j][j];
      if (!(p > 0.0 && isfinite(p))) { if (tid == 0) s_fail = 1; break; }       // the same for every thread
      const double d = sqrt(p);
      __syncthreads();
      const int i = j + tid;
      if (i == j) s_L[j][j] = d;
      else if (i < n) s_L[i][j] /= d;
      __syncthreads();
      if (i > j && i < n) {
        const double lij = s_L[i][j];
        for (int k = j + 1; k <= i; ++k) s_L[i][k] -= lij * s_L[k][j];
      }
    }
    __syncthreads();
    if (s_fail) break;
    if (tid < 3) {                                                              // one thread per right-hand side
      for (int j = 0; j < n; ++j) {
        const double y = s_rhs[j][tid] / s_L[j][j];
        s_rhs[j][tid] = y;
        for (int i = j + 1; i < n; ++i) s_rhs[i][tid] -= s_L[i][j] * y;
      }
      for (int j = n - 1; j >= 0; --j) {
        const double x = s_rhs[j][tid] / s_L[j][j];
        s_rhs[j][tid] = x;
        for (int i = 0; i < j; ++i) s_rhs[i][tid] -= s_L[j][i] * x;
      }
    }
    __syncthreads();
    if (tid < n) rotate_right(s_R[s_unk[tid]], s_rhs[tid]);
    __syncthreads();
  }
  __syncthreads();
  const bool fail = s_fail != 0;
  const double (*Rf)[9] = fail ? s_R0 : s_R;
  for (int m = tid; m < M; m += ROT_THREADS) {
    double out = nan;
    if (!isnan(residual[m])) {
      const int a = pairs[2 * m], b = pairs[2 * m + 1];
      double r[3];
      if (s_valid[a] && s_valid[b]) out = edge_residual(Rf[a], Rf[b], R_rel + 9 * (size_t)m, r);
    }
    residual[m] = out;
  }
  if (tid < V) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R_out[9 * tid + i] = Rf[tid][i];
    valid_out[tid] = s_valid[tid] ? 1 : 0;
  }
  if (tid == 0) *status_out = fail ? ROT_STATUS_PIVOT : 0;
}

// ================================================================================================================= positions
struct State {
  int finished, status, pad0, pad1;
  double sign[2];                  // of round r at r & 1
  double lam[2];
};

struct ViewC {                     // constant over the call: 16 doubles
  double R[9], ki[5], ang, ok;
};

struct EdgeRec {                   // a < 0: not usable
  double b[3], lim;                // the baseline direction in the world, 2 max(ang_a, ang_b)
  int a, b_, pad0, pad1;
};
static_assert(sizeof(ViewC) == 128 && sizeof(EdgeRec) == 48, "records");

struct Ws {
  State* st;
  ViewC* view;
  double* C[2];                    // centres of round r at r & 1, 3 MAX_VIEWS each
  int* placed;                     // MAX_VIEWS
  EdgeRec* edge;
  double* X[2];
  unsigned* vote;
  unsigned char* solved;
  double* sys;                     // Msys
  double* part;                    // P x Msys
  double* dpart;                   // MAX_POINT_BLOCKS
};

struct Prm {
  int V, N, M, P, PB, Msys, root, rounds;   // Msys = tri(3 V) + V: the lower triangle, then the weighted observations per view
  long point_stride;
};

// d = R^T h / |h|, h = K^-1 (x, y, 1); false when the pixel is not seen or the view not usable
__device__ __forceinline__ bool bearing(const ViewC& c, float2 px, double* d) {
  const double x = (double)px.x, y = (double)px.y;
  const double h0 = c.ki[0] * x + c.ki[1] * y + c.ki[2], h1 = c.ki[3] * y + c.ki[4];
  const double inv = 1.0 / sqrt(h0 * h0 + h1 * h1 + 1.0);
  const double u0 = h0 * inv, u1 = h1 * inv, u2 = inv;
  d[0] = c.R[0] * u0 + c.R[3] * u1 + c.R[6] * u2;
  d[1] = c.R[1] * u0 + c.R[4] * u1 + c.R[7] * u2;
  d[2] = c.R[2] * u0 + c.R[5] * u1 + c.R[8] * u2;
  return !isnan(px.x) && c.ok != 0.0;
}

// the weight that the round after `prev` gives a seen observation of a solved point: X and C of round prev (signs applied)
__device__ __forceinline__ double next_weight(const double* d, const double* C, const double* X, double ang_thr, int prev, int rounds) {
  const double rel[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]};
  const double depth = rel[0] * d[0] + rel[1] * d[1] + rel[2] * d[2];
  const double dist = sqrt(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]);
  const double p[3] = {rel[0] - d[0] * depth, rel[1] - d[1] * depth, rel[2] - d[2] * depth};
  const double ang = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) / dist;
  bool good = depth > 0.0 && dist > 1e-12;
  if (prev >= rounds - 2) good = good && ang < ang_thr;
  const int sh = rounds - 2 - prev;
  const double q = ang / (ang_thr * (double)(1 << (sh > 0 ? sh : 0)));
  return good ? 1.0 / (1.0 + q * q) : 0.0;
}

// the weight of (v, n) entering round r; d is valid when it returns a positive weight
__device__ __forceinline__ double weight_of(const ViewC& c, float2 px, double* d, int v, int r, int rounds, unsigned votes, bool solved_before,
                                            const double* Cprev, const double* Xprev) {
  if (!bearing(c, px, d)) return 0.0;
  if (r == 0) return ((votes >> v) & 1u) ? 1.0 : 0.0;
  if (!solved_before) return 0.0;
  return next_weight(d, Cprev, Xprev, c.ang, r - 1, rounds);
}

// A symmetric 3 x 3 as (a00, a01, a02, a11, a12, a22): solved = det > 1e-12 tr^3, the inverse by the adjugate
__device__ __forceinline__ bool inverse3(const double* a, double* inv) {
  const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[1] * a[5] - a[4] * a[2], c02 = a[1] * a[4] - a[3] * a[2];
  const double det = a[0] * c00 - a[1] * c01 + a[2] * c02;
  const double tr = a[0] + a[3] + a[5];
  const double id = 1.0 / det;
  inv[0] = c00 * id;
  inv[1] = -c01 * id;
  inv[2] = c02 * id;
  inv[3] = (a[0] * a[5] - a[2] * a[2]) * id;
  inv[4] = -(a[0] * a[4] - a[1] * a[2]) * id;
  inv[5] = (a[0] * a[3] - a[1] * a[1]) * id;
  return det > 1e-12 * tr * tr * tr;
}

// --------------------------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(POINT_THREADS) void positions_init_kernel(Ws ws, Prm prm, const double* __restrict__ K, const double* __restrict__ R,
                                                                       const int* __restrict__ pairs, const double* __restrict__ t_rel,
                                                                       double threshold, int* __restrict__ count) {
  __shared__ double s_ang[MAX_VIEWS];
  __shared__ int s_ok[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V;
  if (tid < MAX_VIEWS) {
    ViewC c;
    bool ok = false;
    if (tid < V) {
      const double* Kv = K + 9 * tid;
      const double* Rv = R + 9 * tid;
      // K^-1 as invert_k has it, written here so that it is not contracted: the bearings are what motion_ref.bearings computes, bit for
      // bit (a track of low parallax theta amplifies one ulp of its bearings by 1 / theta^2)
      const double fx = Kv[0], sk = Kv[1], cx = Kv[2], fy = Kv[4], cy = Kv[5], dk = fx * fy;
      c.ki[0] = 1.0 / fx; c.ki[1] = -sk / dk; c.ki[2] = (sk * cy - cx * fy) / dk; c.ki[3] = 1.0 / fy; c.ki[4] = -cy / fy;
      ok = isfinite(fx) && isfinite(sk) && isfinite(cx) && isfinite(fy) && isfinite(cy) && dk != 0.0 && isfinite(1.0 / dk);
      ok = ok && upper_triangular(Kv);
#pragma unroll
      for (int i = 0; i < 9; ++i) { ok = ok && isfinite(Rv[i]); c.R[i] = Rv[i]; }
      c.ang = threshold / sqrt(fabs(Kv[0] * Kv[4]));
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) c.R[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 5; ++i) c.ki[i] = 0.0;
      c.ang = 0.0;
    }
    c.ok = ok ? 1.0 : 0.0;
    ws.view[tid] = c;
    s_ang[tid] = c.ang;
    s_ok[tid] = ok ? 1 : 0;
    ws.placed[tid] = 0;
  }
  if (tid < 3 * MAX_VIEWS) { ws.C[0][tid] = 0.0; ws.C[1][tid] = 0.0; }
  if (tid == 0) {
    State& s = *ws.st;
    s.finished = 0; s.status = 0; s.pad0 = 0; s.pad1 = 0;
    s.sign[0] = 1.0; s.sign[1] = 1.0;
    s.lam[0] = 0.0; s.lam[1] = 0.0;
    *count = 0;
  }
  __syncthreads();
  for (int m = tid; m < prm.M; m += POINT_THREADS) {
    const int a = pairs[2 * m], b = pairs[2 * m + 1];
    const double t[3] = {t_rel[3 * m], t_rel[3 * m + 1], t_rel[3 * m + 2]};
    const double n2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
    bool ok = a != b && a >= 0 && a < V && b >= 0 && b < V && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]) && n2 > 0.0;
    ok = ok && s_ok[a] && s_ok[b];
    EdgeRec e;
    e.a = ok ? a : -1; e.b_ = ok ? b : -1; e.pad0 = 0; e.pad1 = 0;
    e.b[0] = e.b[1] = e.b[2] = 0.0; e.lim = 0.0;
    if (ok) {
      const double* Rb = R + 9 * b;
      const double inv = 1.0 / sqrt(n2);
      const double u[3] = {t[0] * inv, t[1] * inv, t[2] * inv};
#pragma unroll
      for (int j = 0; j < 3; ++j) e.b[j] = -(Rb[j] * u[0] + Rb[3 + j] * u[1] + Rb[6 + j] * u[2]);
      e.lim = 2.0 * fmax(s_ang[a], s_ang[b]);
    }
    ws.edge[m] = e;
  }
}

// --------------------------------------------------------------------------------------------------------------------- vote
__global__ __launch_bounds__(CHUNK) void positions_vote_kernel(ObsTable tab, Ws ws, Prm prm) {
  __shared__ double s_d[MAX_VIEWS][3][CHUNK];
  __shared__ unsigned short s_cnt[MAX_VIEWS][CHUNK], s_vote[MAX_VIEWS][CHUNK];
  __shared__ ViewC s_view[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V;
  if (tid < MAX_VIEWS) s_view[tid] = ws.view[tid];
  __syncthreads();
  const long n = (long)blockIdx.x * CHUNK + tid;
  if (n >= prm.N) return;                                                       // no barrier below
  unsigned seen = 0;
  for (int v = 0; v < V; ++v) {
    double d[3];
    const bool see = bearing(s_view[v], load_px(tab, v, n, prm.point_stride), d);
    seen |= (see ? 1u : 0u) << v;
    s_d[v][0][tid] = d[0]; s_d[v][1][tid] = d[1]; s_d[v][2][tid] = d[2];
    s_cnt[v][tid] = 0;
    s_vote[v][tid] = 0;
  }
  for (int m = 0; m < prm.M; ++m) {
    const EdgeRec& e = ws.edge[m];
    const int a = e.a, b = e.b_;
    if (a < 0) continue;                                                        // the same for every lane
    if (!((seen >> a) & (seen >> b) & 1u)) continue;
    const double da[3] = {s_d[a][0][tid], s_d[a][1][tid], s_d[a][2][tid]}, db[3] = {s_d[b][0][tid], s_d[b][1][tid], s_d[b][2][tid]};
    double c[3];
    cross3(da, db, c);
    const bool agree = fabs(c[0] * e.b[0] + c[1] * e.b[1] + c[2] * e.b[2]) < e.lim;
    s_cnt[a][tid] += 1; s_cnt[b][tid] += 1;
    if (agree) { s_vote[a][tid] += 1; s_vote[b][tid] += 1; }
  }
  unsigned w = 0;
  for (int v = 0; v < V; ++v) {
    const int vt = s_vote[v][tid], cn = s_cnt[v][tid];
    if (((seen >> v) & 1u) && vt >= 1 && 2 * vt >= cn) w |= 1u << v;
  }
  ws.vote[n] = w;
  ws.solved[n] = 1;
}

// --------------------------------------------------------------------------------------------------------------- accumulate
__global__ __launch_bounds__(CHUNK) void positions_accumulate_kernel(ObsTable tab, Ws ws, Prm prm, int r) {
  const State& st = *ws.st;
  if (st.finished) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* part = reinterpret_cast<double*>(smem);                               // Msys
  __shared__ ViewC s_view[MAX_VIEWS];
  __shared__ double s_C[MAX_VIEWS][3];
  __shared__ float2 s_px[MAX_VIEWS][CHUNK];
  __shared__ double s_Q[MAX_VIEWS][6], s_Y[MAX_VIEWS][9];
  __shared__ unsigned short s_pair[MAX_VIEWS * (MAX_VIEWS + 1) / 2];
  __shared__ int s_list[MAX_VIEWS];
  const int tid = threadIdx.x, V = prm.V, cntoff = tri(3 * V);
  const int prev = (r + 1) & 1;                                                 // (r - 1) & 1
  const double sign = r > 0 ? st.sign[prev] : 1.0;
  if (tid < MAX_VIEWS) {
    s_view[tid] = ws.view[tid];
#pragma unroll
    for (int j = 0; j < 3; ++j) s_C[tid][j] = ws.C[prev][3 * tid + j];
  }
  for (int e = tid; e < prm.Msys; e += CHUNK) part[e] = 0.0;
  for (int e = tid; e < tri(MAX_VIEWS); e += CHUNK) {
    int ja = 0;
    while (tri(ja + 1) <= e) ++ja;
    s_pair[e] = (unsigned short)((ja << 8) | (e - tri(ja)));
  }
  __syncthreads();
  const int nchunks = (prm.N + CHUNK - 1) / CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long n0 = (long)chunk * CHUNK;
    const int in_chunk = min(CHUNK, prm.N - chunk * CHUNK);
    if (tid < in_chunk)
      for (int v = 0; v < V; ++v) s_px[v][tid] = load_px(tab, v, n0 + tid, prm.point_stride);
    __syncthreads();
    for (int i = 0; i < in_chunk; ++i) {
      const long n = n0 + i;
      const bool before = ws.solved[n] != 0;
      double w = 0.0, Q[6];
      if (tid < V) {
        double d[3], X[3] = {0.0, 0.0, 0.0};
        if (r > 0) { X[0] = sign * ws.X[prev][3 * n]; X[1] = sign * ws.X[prev][3 * n + 1]; X[2] = sign * ws.X[prev][3 * n + 2]; }
        w = weight_of(s_view[tid], s_px[tid][i], d, tid, r, prm.rounds, ws.vote[n], before, s_C[tid], X);
        if (!(w > 0.0)) { w = 0.0; d[0] = d[1] = d[2] = 0.0; }
        Q[0] = w * (1.0 - d[0] * d[0]); Q[1] = w * (-(d[0] * d[1])); Q[2] = w * (-(d[0] * d[2]));
        Q[3] = w * (1.0 - d[1] * d[1]); Q[4] = w * (-(d[1] * d[2])); Q[5] = w * (1.0 - d[2] * d[2]);
#pragma unroll
        for (int j = 0; j < 6; ++j) s_Q[tid][j] = Q[j];
      }
      const unsigned act = (unsigned)__ballot(w > 0.0);
      if (tid < V && w > 0.0) s_list[__popc(act & ((1u << tid) - 1u))] = tid;
      __syncthreads();
      double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, inv[6];
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int j = 0; j < 6; ++j) A[j] += s_Q[v][j];
      const bool solved = inverse3(A, inv) && __popc(act) >= 2 && before;       // the same for every lane
      if (tid == 0) ws.solved[n] = solved ? 1 : 0;
      if (solved) {
        if (tid < V && w > 0.0) {
          const int r0 = 3 * tid;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const double row[3] = {Q[a == 0 ? 0 : a], Q[a == 0 ? 1 : (a == 1 ? 3 : 4)], Q[a == 0 ? 2 : (a == 1 ? 4 : 5)]};
            double y[3];
            sym3_times(inv, row, y);                                            // row a of Q A^-1 (both symmetric)
            s_Y[tid][3 * a] = y[0]; s_Y[tid][3 * a + 1] = y[1]; s_Y[tid][3 * a + 2] = y[2];
          }
          part[tri(r0) + r0] += Q[0];
          part[tri(r0 + 1) + r0] += Q[1]; part[tri(r0 + 1) + r0 + 1] += Q[3];
          part[tri(r0 + 2) + r0] += Q[2]; part[tri(r0 + 2) + r0 + 1] += Q[4]; part[tri(r0 + 2) + r0 + 2] += Q[5];
          part[cntoff + tid] += 1.0;
        }
        __syncthreads();
        const int items = tri(__popc(act)) * 9;
        for (int item = tid; item < items; item += CHUNK) {
          const int pair = item / 9, e = item - 9 * pair, ra = e / 3, sb = e - 3 * ra;
          const int ja = s_pair[pair] >> 8, jb = s_pair[pair] & 255;
          if (ja == jb && sb > ra) continue;
          const int a = s_list[ja], b = s_list[jb];                             // a >= b: the list ascends
          const double* y = &s_Y[a][3 * ra];
          const double* q = s_Q[b];
          const double q0 = q[sb], q1 = q[sb == 0 ? 1 : (sb == 1 ? 3 : 4)], q2 = q[sb == 0 ? 2 : (sb == 1 ? 4 : 5)];   // column sb of Q_b
          part[tri(3 * a + ra) + 3 * b + sb] -= y[0] * q0 + y[1] * q1 + y[2] * q2;
        }
      }
      __syncthreads();
    }
  }
  double* out = ws.part + (size_t)blockIdx.x * prm.Msys;
  for (int e = tid; e < prm.Msys; e += CHUNK) out[e] = part[e];
}

__global__ __launch_bounds__(POINT_THREADS) void positions_reduce_kernel(Ws ws, Prm prm) {
  if (ws.st->finished) return;
  reduce_partials(ws.part, ws.sys, prm.Msys, prm.P, blockIdx.x * POINT_THREADS + threadIdx.x);
}

// -------------------------------------------------------------------------------------------------------------------- solve
__global__ __launch_bounds__(SOLVE_THREADS) void positions_solve_kernel(Ws ws, Prm prm, int r) {
  State& st = *ws.st;
  if (st.finished) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double s_c[3 * MAX_VIEWS / 2], s_s[3 * MAX_VIEWS / 2];
  __shared__ int s_p[3 * MAX_VIEWS / 2], s_q[3 * MAX_VIEWS / 2];
  __shared__ double s_red[SOLVE_THREADS / 64][2];
  __shared__ int s_keep[MAX_VIEWS], s_nk, s_status, s_j[2];
  const int tid = threadIdx.x, V = prm.V, cntoff = tri(3 * V);
  if (tid == 0) {
    int nk = 0, np = 0, status = 0;
    for (int v = 0; v < MAX_VIEWS; ++v) {
      const int placed = v < V && ws.sys[cntoff + v] > 0.0 ? 1 : 0;
      ws.placed[v] = placed;
      np += placed;
      if (v < V && !placed) status |= STATUS_UNPLACED;
      if (placed && v != prm.root) s_keep[nk++] = v;
    }
    if (np < 2 || !(ws.sys[cntoff + prm.root] > 0.0)) status |= STATUS_TOO_FEW;
    s_nk = nk;
    s_status = status;
  }
  __syncthreads();
  if (s_status & STATUS_TOO_FEW) {
    if (tid == 0) { st.status = s_status; st.finished = 1; }
    return;
  }
  const int n = 3 * s_nk, n2 = n + (n & 1), half = n2 / 2;
  double* A = reinterpret_cast<double*>(smem);                                  // n2 x n2
  double* Q = A + n2 * n2;                                                      // the eigenvectors in its columns
  double trace = 0.0;
  for (int i = 0; i < n; ++i) {
    const int gi = 3 * s_keep[i / 3] + i % 3;
    trace += fabs(ws.sys[tri(gi) + gi]);
  }
  for (int e = tid; e < n2 * n2; e += SOLVE_THREADS) {
    const int i = e / n2, j = e - i * n2;
    double a;
    if (i < n && j < n) {
      const int gi = 3 * s_keep[i / 3] + i % 3, gj = 3 * s_keep[j / 3] + j % 3;
      a = gi >= gj ? ws.sys[tri(gi) + gj] : ws.sys[tri(gj) + gi];
    } else {
      a = i == j ? 2.0 * trace + 1.0 : 0.0;                                     // the padding row: above every eigenvalue, coupled to nothing
    }
    A[e] = a;
    Q[e] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sw = 0; sw < SWEEPS; ++sw) {
    double s[2] = {0.0, 0.0};
    for (int e = tid; e < n2 * n2; e += SOLVE_THREADS) {
      const int i = e / n2, j = e - i * n2;
      const double a = A[e];
      s[i == j ? 1 : 0] += a * a;
    }
    block_sum<2, SOLVE_THREADS / 64>(s, s_red);
    if (!(s[0] > 1e-32 * s[1])) break;                                          // the same for every thread
    for (int step = 0; step < n2 - 1; ++step) {
      if (tid < half) {                                                         // the round-robin order: n2 - 1 is fixed, the others rotate
        const int m1 = n2 - 1;
        int p = tid == 0 ? m1 : (step + tid) % m1, q = tid == 0 ? step : (step - tid + m1) % m1;
        if (p > q) { const int t = p; p = q; q = t; }
        const double app = A[p * n2 + p], aqq = A[q * n2 + q], apq = A[p * n2 + q];
        double c = 1.0, sn = 0.0;
        if (apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          sn = t * c;
        }
        s_c[tid] = c; s_s[tid] = sn; s_p[tid] = p; s_q[tid] = q;
      }
      __syncthreads();
      for (int e = tid; e < n2 * half; e += SOLVE_THREADS) {                    // columns p, q of A and of Q
        const int i = e / half, k = e - i * half, p = s_p[k], q = s_q[k];
        const double c = s_c[k], sn = s_s[k];
        const double ap = A[i * n2 + p], aq = A[i * n2 + q], vp = Q[i * n2 + p], vq = Q[i * n2 + q];
        A[i * n2 + p] = c * ap - sn * aq; A[i * n2 + q] = sn * ap + c * aq;
        Q[i * n2 + p] = c * vp - sn * vq; Q[i * n2 + q] = sn * vp + c * vq;
      }
      __syncthreads();
      for (int e = tid; e < n2 * half; e += SOLVE_THREADS) {                    // rows p, q of A
        const int k = e / n2, j = e - k * n2, p = s_p[k], q = s_q[k];
        const double c = s_c[k], sn = s_s[k];
        const double ap = A[p * n2 + j], aq = A[q * n2 + j];
        A[p * n2 + j] = j == q ? 0.0 : c * ap - sn * aq;                        // the rotated pair is exactly 0
        A[q * n2 + j] = j == p ? 0.0 : sn * ap + c * aq;
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    int j1 = 0;
    for (int i = 1; i < n; ++i)
      if (A[i * n2 + i] < A[j1 * n2 + j1]) j1 = i;
    int j2 = j1 == 0 ? 1 : 0;
    for (int i = 0; i < n; ++i)
      if (i != j1 && A[i * n2 + i] < A[j2 * n2 + j2]) j2 = i;
    s_j[0] = j1; s_j[1] = j2;
    const double l1 = A[j1 * n2 + j1], l2 = A[j2 * n2 + j2];
    st.lam[0] = l1; st.lam[1] = l2;
    int status = s_status;
    if (!(l2 > 0.0 && isfinite(l2) && isfinite(l1))) { status |= STATUS_EIGEN; st.finished = 1; }
    st.status = status;
  }
  __syncthreads();
  const int j1 = s_j[0];
  const double nan = __builtin_nan("");
  if (tid < 3 * MAX_VIEWS) ws.C[r & 1][tid] = tid / 3 == prm.root ? 0.0 : nan;
  __syncthreads();
  if (tid < n) ws.C[r & 1][3 * s_keep[tid / 3] + tid % 3] = Q[tid * n2 + j1];
}

// ------------------------------------------------------------------------------------------------------------------- points
__global__ __launch_bounds__(POINT_THREADS) void positions_points_kernel(ObsTable tab, Ws ws, Prm prm, int r) {
  const State& st = *ws.st;
  if (st.finished) return;
  __shared__ ViewC s_view[MAX_VIEWS];
  __shared__ double s_C[2][MAX_VIEWS][3];                                       // of the round before (signed) and of this round
  __shared__ double s_red[POINT_THREADS / 64][1];
  const int tid = threadIdx.x, V = prm.V, cur = r & 1, prev = cur ^ 1;
  const double sign = r > 0 ? st.sign[prev] : 1.0;
  if (tid < MAX_VIEWS) {
    s_view[tid] = ws.view[tid];
#pragma unroll
    for (int j = 0; j < 3; ++j) { s_C[0][tid][j] = ws.C[prev][3 * tid + j]; s_C[1][tid][j] = ws.C[cur][3 * tid + j]; }
  }
  __syncthreads();
  const double nan = __builtin_nan("");
  double total[1] = {0.0};
  const long nchunks = ((long)prm.N + POINT_THREADS - 1) / POINT_THREADS;
  for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long n = chunk * POINT_THREADS + tid;
    if (n >= prm.N) continue;
    const bool solved = ws.solved[n] != 0;
    double X[3] = {nan, nan, nan};
    if (solved) {
      double Xp[3] = {0.0, 0.0, 0.0};
      if (r > 0) { Xp[0] = sign * ws.X[prev][3 * n]; Xp[1] = sign * ws.X[prev][3 * n + 1]; Xp[2] = sign * ws.X[prev][3 * n + 2]; }
      const unsigned votes = ws.vote[n];
      double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, wd[3] = {0.0, 0.0, 0.0}, wcd = 0.0;
#pragma unroll 1
      for (int v = 0; v < V; ++v) {
        double d[3];
        const double w = weight_of(s_view[v], load_px(tab, v, n, prm.point_stride), d, v, r, prm.rounds, votes, true, s_C[0][v], Xp);
        if (!(w > 0.0)) continue;
        const double Q[6] = {w * (1.0 - d[0] * d[0]), w * (-(d[0] * d[1])), w * (-(d[0] * d[2])),
                             w * (1.0 - d[1] * d[1]), w * (-(d[1] * d[2])), w * (1.0 - d[2] * d[2])};
        const double* C = s_C[1][v];
        double qc[3];
        sym3_times(Q, C, qc);
#pragma unroll
        for (int j = 0; j < 6; ++j) A[j] += Q[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) { g[j] += qc[j]; wd[j] += w * d[j]; }
        wcd += w * (C[0] * d[0] + C[1] * d[1] + C[2] * d[2]);
      }
      double inv[6];
      inverse3(A, inv);
      sym3_times(inv, g, X);
      total[0] += (X[0] * wd[0] + X[1] * wd[1] + X[2] * wd[2]) - wcd;           // sum of w (X - C_v) . d_v
    }
    ws.X[cur][3 * n] = X[0]; ws.X[cur][3 * n + 1] = X[1]; ws.X[cur][3 * n + 2] = X[2];
  }
  block_sum<1, POINT_THREADS / 64>(total, s_red);
  if (tid == 0) ws.dpart[blockIdx.x] = total[0];
}

__global__ __launch_bounds__(3 * MAX_VIEWS) void positions_sign_kernel(Ws ws, Prm prm, int r) {
  State& st = *ws.st;
  if (st.finished) return;
  __shared__ double s_sign;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int p = 0; p < prm.PB; ++p) s += ws.dpart[p];
    s_sign = s < 0.0 ? -1.0 : 1.0;
    st.sign[r & 1] = s_sign;
  }
  __syncthreads();
  ws.C[r & 1][threadIdx.x] *= s_sign;
}

// -------------------------------------------------------------------------------------------------------------------- final
__global__ __launch_bounds__(POINT_THREADS) void positions_final_kernel(ObsTable tab, Ws ws, Prm prm, const double* __restrict__ R,
                                                                        double* __restrict__ t, double* __restrict__ centres,
                                                                        double* __restrict__ points, unsigned char* __restrict__ mask,
                                                                        int* __restrict__ count, double* __restrict__ eigenvalues,
                                                                        int* __restrict__ status) {
  const State& st = *ws.st;
  __shared__ ViewC s_view[MAX_VIEWS];
  __shared__ double s_C[MAX_VIEWS][3];
  __shared__ int s_count;
  const int tid = threadIdx.x, V = prm.V, last = (prm.rounds - 1) & 1;
  const bool failed = st.finished != 0;
  const double nan = __builtin_nan(""), sign = st.sign[last];
  if (tid == 0) s_count = 0;
  if (tid < MAX_VIEWS) {
    s_view[tid] = ws.view[tid];
    const bool placed = !failed && ws.placed[tid] != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) s_C[tid][j] = placed ? ws.C[last][3 * tid + j] : nan;
    if (blockIdx.x == 0 && tid < V) {
      const double* Rv = R + 9 * tid;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        centres[3 * tid + j] = s_C[tid][j];
        t[3 * tid + j] = -(Rv[3 * j] * s_C[tid][0] + Rv[3 * j + 1] * s_C[tid][1] + Rv[3 * j + 2] * s_C[tid][2]);
      }
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    eigenvalues[0] = failed ? nan : st.lam[0];
    eigenvalues[1] = failed ? nan : st.lam[1];
    *status = st.status;
  }
  __syncthreads();
  const long n = (long)blockIdx.x * POINT_THREADS + tid;
  int mine = 0;
  if (n < prm.N) {
    const bool solved = !failed && ws.solved[n] != 0;
    double X[3] = {nan, nan, nan};
    if (solved) { X[0] = sign * ws.X[last][3 * n]; X[1] = sign * ws.X[last][3 * n + 1]; X[2] = sign * ws.X[last][3 * n + 2]; }
    points[3 * n] = X[0]; points[3 * n + 1] = X[1]; points[3 * n + 2] = X[2];
    for (int v = 0; v < V; ++v) {
      double d[3], w = 0.0;
      if (solved) w = weight_of(s_view[v], load_px(tab, v, n, prm.point_stride), d, v, prm.rounds, prm.rounds, 0u, true, s_C[v], X);
      const bool in = w > 0.0;
      mask[(size_t)v * prm.N + n] = in ? 1 : 0;
      mine += in ? 1 : 0;
    }
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (tid == 0 && s_count) atomicAdd(count, s_count);
}

// bytes of the workspace and the offsets of its REGIONS regions, each 256-byte aligned
long layout(int V, int N, int M, long* off) {
  const long Msys = tri(3 * V) + V;
  const long P = std::min<long>(((long)N + CHUNK - 1) / CHUNK, MAX_PARTIALS);
  const long bytes[REGIONS] = {(long)sizeof(State), (long)sizeof(ViewC) * MAX_VIEWS, 8L * 6 * MAX_VIEWS + 4L * MAX_VIEWS, (long)sizeof(EdgeRec) * M,
                               24L * N, 24L * N, 4L * N, 1L * N, 8 * Msys, 8 * Msys * P, 8L * MAX_POINT_BLOCKS};
  return layout_regions(bytes, REGIONS, off);
}

int check_shape(const char* fn, int V, int N, int M) {
  ROMA_REQUIRE(V >= 3 && V <= MAX_VIEWS, ROMA_E_SHAPE, "%s: bad shape V=%d (3 to %d views)", fn, V, MAX_VIEWS);
  ROMA_REQUIRE(N >= 1 && N <= (1 << 24), ROMA_E_SHAPE, "%s: bad shape N=%d (1 to 2^24 points)", fn, N);
  ROMA_REQUIRE(M >= 1 && M <= MAX_EDGES, ROMA_E_SHAPE, "%s: bad shape M=%d (1 to %d edges)", fn, M, MAX_EDGES);
  return 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_rotation_average(const double* R_rel, const int* pairs, const double* weights, int V, int M, int root, double sigma_deg,
                                     int iters, double* R, unsigned char* valid, double* residual, int* status, void* stream) {
  ROMA_REQUIRE(R_rel && pairs && R && valid && residual && status, ROMA_E_ARG, "roma_rotation_average: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "roma_rotation_average: bad shape V=%d (2 to %d views)", V, MAX_VIEWS);
  ROMA_REQUIRE(M >= 1 && M <= MAX_EDGES, ROMA_E_SHAPE, "roma_rotation_average: bad shape M=%d (1 to %d edges)", M, MAX_EDGES);
  ROMA_REQUIRE(root >= 0 && root < V, ROMA_E_ARG, "roma_rotation_average: root=%d is not one of the V=%d views", root, V);
  ROMA_REQUIRE(sigma_deg > 0.0 && sigma_deg < 1e18, ROMA_E_ARG, "roma_rotation_average: sigma_deg must be positive, got %g", sigma_deg);
  ROMA_REQUIRE(iters >= 0 && iters <= 50, ROMA_E_ARG, "roma_rotation_average: iters must be in [0, 50], got %d", iters);
  ROMA_REQUIRE(aligned16(R_rel) && aligned16(R) && aligned8(residual) && (weights == nullptr || aligned8(weights)), ROMA_E_ALIGN,
               "roma_rotation_average: R_rel and R must be 16-byte aligned, weights and residual 8-byte aligned");
  ROMA_REQUIRE(aligned4(pairs) && aligned4(status), ROMA_E_ALIGN,
               "roma_rotation_average: pairs and status must be 4-byte aligned");
  const double sigma = sigma_deg * 3.14159265358979323846 / 180.0;
  hipLaunchKernelGGL(rotation_average_kernel, dim3(1), dim3(ROT_THREADS), 0, static_cast<hipStream_t>(stream), R_rel, pairs, weights, V, M, root,
                     sigma * sigma, iters, R, valid, residual, status);
  ROMA_CHECK_LAUNCH();
}

extern "C" long roma_positions_workspace(int V, int N, int M, long* offsets) {
  if (int rc = check_shape("roma_positions_workspace", V, N, M)) return rc;
  return layout(V, N, M, offsets);
}

extern "C" int roma_global_positions(const float* const* obs, const float* to_px, const unsigned char* const* visible, long point_stride,
                                     const double* K, const double* R, const int* pairs, const double* t_rel, int V, int N, int M, int root,
                                     double threshold, int rounds, double* t, double* centres, double* points, unsigned char* mask, int* count,
                                     double* eigenvalues, int* status, void* workspace, long workspace_size, void* stream) {
  ROMA_REQUIRE(obs && K && R && pairs && t_rel && t && centres && points && mask && count && eigenvalues && status && workspace, ROMA_E_ARG,
               "roma_global_positions: null pointer");
  if (int rc = check_shape("roma_global_positions", V, N, M)) return rc;
  ROMA_REQUIRE(point_stride >= 2 && point_stride % 2 == 0, ROMA_E_SHAPE,
               "roma_global_positions: bad strides point_stride=%ld (floats: even, at least 2)", point_stride);
  ROMA_REQUIRE(root >= 0 && root < V, ROMA_E_ARG, "roma_global_positions: root=%d is not one of the V=%d views", root, V);
  ROMA_REQUIRE(threshold > 0.0 && threshold < 1e18, ROMA_E_ARG, "roma_global_positions: threshold must be positive, got %g", threshold);
  ROMA_REQUIRE(rounds >= 2 && rounds <= 8, ROMA_E_ARG, "roma_global_positions: rounds must be in [2, 8], got %d", rounds);
  long off[REGIONS];
  const long need = layout(V, N, M, off);
  ROMA_REQUIRE(workspace_size >= need, ROMA_E_ARG, "roma_global_positions: workspace of %ld bytes, roma_positions_workspace asks for %ld",
               workspace_size, need);
  ROMA_REQUIRE(aligned16(workspace) && aligned16(K) && aligned16(R) && aligned16(t_rel) && aligned16(t) && aligned16(centres) && aligned16(points) &&
                   aligned16(eigenvalues),
               ROMA_E_ALIGN, "roma_global_positions: workspace, K, R, t_rel, t, centres, points and eigenvalues must be 16-byte aligned");
  ROMA_REQUIRE(aligned4(count) && aligned4(status) && aligned4(pairs), ROMA_E_ALIGN,
               "roma_global_positions: pairs, count and status must be 4-byte aligned");
  ObsTable tab;
  if (int rc = fill_obs_table("roma_global_positions", obs, to_px, visible, V, tab)) return rc;
  Prm prm;
  prm.V = V; prm.N = N; prm.M = M; prm.root = root; prm.rounds = rounds;
  prm.Msys = tri(3 * V) + V;
  prm.P = std::min((N + CHUNK - 1) / CHUNK, MAX_PARTIALS);
  prm.PB = std::min((N + POINT_THREADS - 1) / POINT_THREADS, MAX_POINT_BLOCKS);
  prm.point_stride = point_stride;
  char* base = static_cast<char*>(workspace);
  Ws ws;
  ws.st = reinterpret_cast<State*>(base + off[0]);
  ws.view = reinterpret_cast<ViewC*>(base + off[1]);
  ws.C[0] = reinterpret_cast<double*>(base + off[2]);
  ws.C[1] = ws.C[0] + 3 * MAX_VIEWS;
  ws.placed = reinterpret_cast<int*>(ws.C[1] + 3 * MAX_VIEWS);
  ws.edge = reinterpret_cast<EdgeRec*>(base + off[3]);
  ws.X[0] = reinterpret_cast<double*>(base + off[4]);
  ws.X[1] = reinterpret_cast<double*>(base + off[5]);
  ws.vote = reinterpret_cast<unsigned*>(base + off[6]);
  ws.solved = reinterpret_cast<unsigned char*>(base + off[7]);
  ws.sys = reinterpret_cast<double*>(base + off[8]);
  ws.part = reinterpret_cast<double*>(base + off[9]);
  ws.dpart = reinterpret_cast<double*>(base + off[10]);

  constexpr int N2_MAX = 3 * (MAX_VIEWS - 1) + 1;                               // 93 unknowns padded to 94
  static std::atomic<uint64_t> attr_done{0};
  if (int rc = ensure_dyn_smem(reinterpret_cast<const void*>(positions_solve_kernel), 2 * N2_MAX * N2_MAX * (int)sizeof(double), attr_done,
                               "roma_global_positions"))
    return rc;
  const int n2 = 3 * (V - 1) + ((3 * (V - 1)) & 1);
  const size_t solve_lds = (size_t)2 * n2 * n2 * sizeof(double), part_lds = (size_t)prm.Msys * sizeof(double);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 one(1), chunk_block(CHUNK), point_block(POINT_THREADS), chunk_grid((unsigned)prm.P), walk_grid((unsigned)prm.PB),
      point_grid((unsigned)((N + POINT_THREADS - 1) / POINT_THREADS)), vote_grid((unsigned)((N + CHUNK - 1) / CHUNK));
  hipLaunchKernelGGL(positions_init_kernel, one, point_block, 0, s, ws, prm, K, R, pairs, t_rel, threshold, count);
  hipLaunchKernelGGL(positions_vote_kernel, vote_grid, chunk_block, 0, s, tab, ws, prm);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(positions_accumulate_kernel, chunk_grid, chunk_block, part_lds, s, tab, ws, prm, r);
    hipLaunchKernelGGL(positions_reduce_kernel, dim3((unsigned)((prm.Msys + POINT_THREADS - 1) / POINT_THREADS)), point_block, 0, s, ws, prm);
    hipLaunchKernelGGL(positions_solve_kernel, one, dim3(SOLVE_THREADS), solve_lds, s, ws, prm, r);
    hipLaunchKernelGGL(positions_points_kernel, walk_grid, point_block, 0, s, tab, ws, prm, r);
    hipLaunchKernelGGL(positions_sign_kernel, one, dim3(3 * MAX_VIEWS), 0, s, ws, prm, r);
  }
  hipLaunchKernelGGL(positions_final_kernel, point_grid, point_block, 0, s, tab, ws, prm, R, t, centres, points, mask, count, eigenvalues, status);
  ROMA_CHECK_LAUNCH();
}
