// Two-view triangulation of matches under a known relative pose: what follows match -> sample -> estimate_pose when the caller
// wants 3-D — a point cloud of the sampled matches, or a depth map per image from all rows of the dense warp.  DESIGN.md §3.4.
//
// Convention (recover_pose / estimate_pose): x_B ~ K_B (R X_A + t).  Points come out in camera A's frame, in units of |t| — with
// the unit t of recover_pose, depths are in baselines.
//
// One launch, grid (blocks of MATCHES_PER_BLOCK matches, pair): the pair is a grid dimension, so everything per pair is uniform
// over the workgroup.  Thread 0 computes the pair's constants in fp64 — the pixel-space F = K_B^-T [t]x R K_A^-1 scaled to unit
// Frobenius norm (zero when [t]x R vanishes), the two inverse intrinsics — and leaves them, with K, R and t, as fp32 in LDS.  That is
// the fp64 / fp32 boundary: everything per match is fp32 with IEEE operations (no fast-math; the compiler may fuse a multiply with
// an add), one thread per match and ITEMS matches per thread one after the other, one 16-byte load per match.
//
//   method 0, optimal: Lindstrom, "Triangulation made easy" (CVPR 2010), the closed-form two-step correction (niter2) in pixel space
//     with F: (x_A, x_B) moves by the smallest |d_A|^2 + |d_B|^2 onto x_B^T F x_A = 0, to first order twice.  The corrected rays
//     a = K_A^-1 x_A', b = K_B^-1 x_B' meet; lambda_A, lambda_B of lambda_B b = lambda_A R a + t are the least-squares closed form
//     recover_pose_kernel votes with (essential.hip; fp64 there, fp32 here, so the expression is repeated and not shared: see
//     DESIGN).  X_A = lambda_A a, depths (lambda_A, lambda_B), reproj = sqrt(|d_A|^2 + |d_B|^2) in pixels.
//   method 1, midpoint: the same closed form on the uncorrected rays; X is the midpoint of the two closest points, the depths are
//     its z in either camera, reproj the root of the sum over both images of the squared pixel distance between its projection and
//     the match.
//   cos_parallax = (Ra . b) / (|Ra| |b|) of the rays the method used.
//
// valid = input finite && mask_in && solution finite (b^2 - ac >= 0 and non-zero denominators in the correction included) && both
// depths > 0 && reproj <= max_reproj && cos_parallax <= max_cos_parallax.  A match whose input or solution is not finite gets exact
// zeros in every output; any other match gets its values whether valid or not; no output ever holds NaN or inf.  No atomics, no
// workspace, nothing depends on the other pairs of the batch; tests/triangulate_ref.py restates it in numpy.
#include "twoview_math.h"

namespace roma {
namespace {

constexpr int THREADS = 256, ITEMS = 4, MATCHES_PER_BLOCK = THREADS * ITEMS;
constexpr int METHOD_OPTIMAL = 0, METHOD_MIDPOINT = 1;

// pixel = s * c + o per coordinate, (sx_A, ox_A, sy_A, oy_A, sx_B, ox_B, sy_B, oy_B): a kernel argument by value
struct ToPx {
  float v[8];
};

// fp32 per-pair constants, in this order in LDS
struct PairConst {
  float f[9];              // F, row major, x_B^T F x_A = 0 in pixels, unit Frobenius norm
  float ia[5], ib[5];      // invert_k's five entries of K_A^-1, K_B^-1
  float ka[5], kb[5];      // fx, s, cx, fy, cy
  float r[9], t[3];
};
constexpr int NCONST = sizeof(PairConst) / sizeof(float);

// thread 0: fp64 -> fp32.  A K that is not invertible, or a pose that is not finite, poisons F with NaN: every match of the pair
// then fails the finiteness test and gets zeros.
__device__ void pair_constants(const double* Ka, const double* Kb, const double* R, const double* t, PairConst& c) {
  double ia[5], ib[5];
  const bool ka_ok = invert_k(Ka, ia), kb_ok = invert_k(Kb, ib);
  // E = [t]x R
  double e[9], g[9], f[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    e[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    e[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    e[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
  // g = E K_A^-1, K^-1 = [i0 i1 i2; 0 i3 i4; 0 0 1]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = e[3 * r] * ia[0];
    g[3 * r + 1] = e[3 * r] * ia[1] + e[3 * r + 1] * ia[3];
    g[3 * r + 2] = e[3 * r] * ia[2] + e[3 * r + 1] * ia[4] + e[3 * r + 2];
  }
  // f = K_B^-T g
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    f[j] = ib[0] * g[j];
    f[3 + j] = ib[1] * g[j] + ib[3] * g[3 + j];
    f[6 + j] = ib[2] * g[j] + ib[4] * g[3 + j] + g[6 + j];
  }
  unit_frobenius(f);                                             // zero stays zero (t = 0); NaN stays NaN
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    c.f[i] = (ka_ok && kb_ok) ? (float)f[i] : nan;
    c.r[i] = (float)R[i];
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    c.ia[i] = (float)ia[i];
    c.ib[i] = (float)ib[i];
  }
  c.ka[0] = (float)Ka[0]; c.ka[1] = (float)Ka[1]; c.ka[2] = (float)Ka[2]; c.ka[3] = (float)Ka[4]; c.ka[4] = (float)Ka[5];
  c.kb[0] = (float)Kb[0]; c.kb[1] = (float)Kb[1]; c.kb[2] = (float)Kb[2]; c.kb[3] = (float)Kb[4]; c.kb[4] = (float)Kb[5];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.t[i] = (float)t[i];
}

template <int METHOD>
__global__ __launch_bounds__(THREADS) void triangulate_kernel(const float4* __restrict__ m, ToPx px, const double* __restrict__ Ka,
                                                              const double* __restrict__ Kb, const double* __restrict__ R,
                                                              const double* __restrict__ t, const unsigned char* __restrict__ mask_in,
                                                              int N, float max_reproj, float max_cos, float* __restrict__ points,
                                                              float* __restrict__ depth_a, float* __restrict__ depth_b,
                                                              float* __restrict__ reproj_out, float* __restrict__ cos_out,
                                                              unsigned char* __restrict__ valid) {
  __shared__ PairConst s_c;
  const int p = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) pair_constants(Ka + (size_t)p * 9, Kb + (size_t)p * 9, R + (size_t)p * 9, t + (size_t)p * 3, s_c);
  __syncthreads();
  PairConst c;
  {
    const float* src = reinterpret_cast<const float*>(&s_c);
    float* dst = reinterpret_cast<float*>(&c);
#pragma unroll
    for (int i = 0; i < NCONST; ++i) dst[i] = src[i];
  }
  const float* f = c.f;
  const float* r = c.r;
  const size_t row0 = (size_t)p * (size_t)N;                     // 64-bit: P * N may pass 2^31
  const int n0 = blockIdx.x * MATCHES_PER_BLOCK + tid;
#pragma unroll 1
  for (int it = 0; it < ITEMS; ++it) {
    const int n = n0 + it * THREADS;
    if (n >= N) break;
    const size_t i = row0 + (size_t)n;
    const float4 q = m[i];
    const float xa = q.x * px.v[0] + px.v[1], ya = q.y * px.v[2] + px.v[3];
    const float xb = q.z * px.v[4] + px.v[5], yb = q.w * px.v[6] + px.v[7];
    bool fin = isfinite(xa) && isfinite(ya) && isfinite(xb) && isfinite(yb);
    float ua = xa, va = ya, ub = xb, vb = yb, reproj = 0.f;
    if (METHOD == METHOD_OPTIMAL) {
      float nb0 = f[0] * xa + f[1] * ya + f[2], nb1 = f[3] * xa + f[4] * ya + f[5];          // (F x_A)[:2]
      const float l2 = f[6] * xa + f[7] * ya + f[8];
      float na0 = f[0] * xb + f[3] * yb + f[6], na1 = f[1] * xb + f[4] * yb + f[7];          // (F^T x_B)[:2]
      const float cc = xb * nb0 + yb * nb1 + l2;
      const float a = nb0 * (f[0] * na0 + f[1] * na1) + nb1 * (f[3] * na0 + f[4] * na1);
      const float b = (nb0 * nb0 + nb1 * nb1 + na0 * na0 + na1 * na1) * 0.5f;
      const float disc = b * b - a * cc;
      const float d = sqrtf(disc);
      const float den1 = b + d;
      float lam = cc / den1;
      float da0 = lam * na0, da1 = lam * na1, db0 = lam * nb0, db1 = lam * nb1;
      nb0 -= f[0] * da0 + f[1] * da1;
      nb1 -= f[3] * da0 + f[4] * da1;
      na0 -= f[0] * db0 + f[3] * db1;
      na1 -= f[1] * db0 + f[4] * db1;
      const float den2 = nb0 * nb0 + nb1 * nb1 + na0 * na0 + na1 * na1;
      lam = lam * ((d + d) / den2);
      da0 = lam * na0; da1 = lam * na1; db0 = lam * nb0; db1 = lam * nb1;
      fin = fin && disc >= 0.f && den1 != 0.f && den2 != 0.f;
      ua = xa - da0; va = ya - da1; ub = xb - db0; vb = yb - db1;
      reproj = sqrtf(da0 * da0 + da1 * da1 + db0 * db0 + db1 * db1);
    }
    const float a0 = c.ia[0] * ua + c.ia[1] * va + c.ia[2], a1 = c.ia[3] * va + c.ia[4];     // a = K_A^-1 x_A, a_z = 1
    const float b0 = c.ib[0] * ub + c.ib[1] * vb + c.ib[2], b1 = c.ib[3] * vb + c.ib[4];
    const float q0 = r[0] * a0 + r[1] * a1 + r[2], q1 = r[3] * a0 + r[4] * a1 + r[5], q2 = r[6] * a0 + r[7] * a1 + r[8];   // R a
    const float aa = q0 * q0 + q1 * q1 + q2 * q2, bb = b0 * b0 + b1 * b1 + 1.f, ab = q0 * b0 + q1 * b1 + q2;
    const float at = q0 * c.t[0] + q1 * c.t[1] + q2 * c.t[2], bt = b0 * c.t[0] + b1 * c.t[1] + c.t[2];
    const float det = aa * bb - ab * ab;
    const float la = (ab * bt - bb * at) / det, lb = (aa * bt - ab * at) / det;
    float cosp = ab / sqrtf(aa * bb);
    float X, Y, Z, zb;
    if (METHOD == METHOD_OPTIMAL) {
      X = la * a0; Y = la * a1; Z = la;
      zb = lb;
    } else {
      // the midpoint in B's frame, then back into A's: X_A = R^T (X_B - t)
      const float m0 = 0.5f * (la * q0 + c.t[0] + lb * b0), m1 = 0.5f * (la * q1 + c.t[1] + lb * b1), m2 = 0.5f * (la * q2 + c.t[2] + lb);
      const float e0 = m0 - c.t[0], e1 = m1 - c.t[1], e2 = m2 - c.t[2];
      X = r[0] * e0 + r[3] * e1 + r[6] * e2; Y = r[1] * e0 + r[4] * e1 + r[7] * e2; Z = r[2] * e0 + r[5] * e1 + r[8] * e2;
      zb = m2;
      const float pa0 = (c.ka[0] * X + c.ka[1] * Y) / Z + c.ka[2] - xa, pa1 = c.ka[3] * Y / Z + c.ka[4] - ya;
      const float pb0 = (c.kb[0] * m0 + c.kb[1] * m1) / m2 + c.kb[2] - xb, pb1 = c.kb[3] * m1 / m2 + c.kb[4] - yb;
      reproj = sqrtf(pa0 * pa0 + pa1 * pa1 + pb0 * pb0 + pb1 * pb1);
    }
    fin = fin && isfinite(X) && isfinite(Y) && isfinite(Z) && isfinite(zb) && isfinite(reproj) && isfinite(cosp);
    if (!fin) { X = 0.f; Y = 0.f; Z = 0.f; zb = 0.f; reproj = 0.f; cosp = 0.f; }
    bool ok = fin && Z > 0.f && zb > 0.f && reproj <= max_reproj && cosp <= max_cos;
    if (mask_in) ok = ok && mask_in[i] != 0;
    if (points) { points[3 * i] = X; points[3 * i + 1] = Y; points[3 * i + 2] = Z; }
    if (depth_a) depth_a[i] = Z;
    if (depth_b) depth_b[i] = zb;
    if (reproj_out) reproj_out[i] = reproj;
    if (cos_out) cos_out[i] = cosp;
    if (valid) valid[i] = ok ? 1 : 0;
  }
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_triangulate(const float* m, const float* to_px, const double* Ka, const double* Kb, const double* R, const double* t,
                                const unsigned char* mask_in, int P, int N, int method, float max_reproj, float max_cos_parallax,
                                float* points, float* depth_a, float* depth_b, float* reproj, float* cos_parallax, unsigned char* valid,
                                void* stream) {
  ROMA_REQUIRE(m && Ka && Kb && R && t, ROMA_E_ARG, "roma_triangulate: null pointer");
  ROMA_REQUIRE(points || depth_a || depth_b || reproj || cos_parallax || valid, ROMA_E_ARG, "roma_triangulate: every output is null");
  ROMA_REQUIRE(P >= 1 && P <= 65535, ROMA_E_SHAPE, "roma_triangulate: bad shape P=%d (1 to 65535 pairs)", P);
  ROMA_REQUIRE(N >= 1 && N <= (1 << 28), ROMA_E_SHAPE, "roma_triangulate: bad shape N=%d (1 to 2^28 matches per pair)", N);
  ROMA_REQUIRE(method == METHOD_OPTIMAL || method == METHOD_MIDPOINT, ROMA_E_ARG,
               "roma_triangulate: unknown method %d (0 = optimal, 1 = midpoint)", method);
  ROMA_REQUIRE(!(max_reproj != max_reproj) && !(max_cos_parallax != max_cos_parallax), ROMA_E_ARG,
               "roma_triangulate: max_reproj and max_cos_parallax must not be NaN");
  ROMA_REQUIRE(aligned16(m), ROMA_E_ALIGN, "roma_triangulate: m must be 16-byte aligned");
  ToPx px;
  for (int i = 0; i < 8; ++i) px.v[i] = to_px ? to_px[i] : ((i & 1) ? 0.f : 1.f);
  const dim3 grid((unsigned)((N + MATCHES_PER_BLOCK - 1) / MATCHES_PER_BLOCK), (unsigned)P);
  auto kernel = method == METHOD_OPTIMAL ? triangulate_kernel<METHOD_OPTIMAL> : triangulate_kernel<METHOD_MIDPOINT>;
  hipLaunchKernelGGL(kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(m), px, Ka, Kb, R,
                     t, mask_in, N, max_reproj, max_cos_parallax, points, depth_a, depth_b, reproj, cos_parallax, valid);
  ROMA_CHECK_LAUNCH();
}
