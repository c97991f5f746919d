// One whole ConvRefiner block at MID widths (32 < C <= 160: the D = 144 refiner of scale 2) in one launch — reference:
// romatch/models/matcher.py:77-103 (create_block: depthwise 5x5 conv -> BatchNorm(eval) -> ReLU -> 1x1 conv), 9x per refiner:
//   t[m][k]   = relu(scale[k] * sum_{dy,dx} w25[dy*5+dx][k] * x[m + (dy-2, dx-2)][k] + shift[k])      rounded to 16 bits
//   out[m][n] = bias[n] + sum_k t[m][k] * wt[n][k]
// The plain join of the two kernels that win at this width when run one after the other (dwconv5x5_lds_kernel, pointwise_mfma_kernel):
// t goes from the first to the second through LDS instead of HBM, which halves the bytes of a block (2 instead of 4 passes over the
// activation; measurements: profiles/refiner_mid_block.md).  Persistent 512-thread workgroups, one per CU.  A tile is S consecutive strips of the linear (b, y, strip) order
// (8 pixels each, S = 28 at C = 144: 504 of the 512 threads own one strip x one 16-byte channel packet); it may wrap from one image
// row or image into the next, which the per-pixel 1x1 does not care about.
//   phase A  mid::dw_strip, global -> registers with no halo in LDS, the packed packet to t[pixel][packet] (row stride 21 packets)
//   barrier
//   phase B  mid::pw_row_groups: every wave takes up to two groups of 16 rows of t as its A fragments (one weight fragment read from
//            LDS serves both), stages the results over its own, consumed, rows of t and stores them as 16-byte packets; strips past
//            the right edge and past the last strip are computed and not stored
//   barrier
// Both phases are the code of the two kernels, so the output has the bits of roma_pointwise_mfma(roma_dwconv5x5_bn_relu(x)).
#include "common.h"
#include "refiner_mid_device.h"

namespace roma {
namespace {

constexpr int MID_NT = 512;                                      // threads: 8 waves, 2 per SIMD
constexpr int MID_KP = 5, MID_KPAD = 32 * MID_KP;                // the 1x1 is padded to 160 x 160 (roma_pointwise_mfma's kpad 160)
constexpr int MID_RS = MID_KPAD / 8 + 1;                         // row stride of t and of the weights in packets: odd
constexpr int MID_SMAX = 28, MID_ROWS = MID_SMAX * mid::kStrip;  // strips / pixel rows of a tile at most: 14 groups of 16 rows
constexpr int MID_SMEM = (MID_ROWS * MID_RS + MID_KPAD * MID_RS) * 16 + 25 * MID_KPAD * 4 + MID_KPAD * 4 + MID_ROWS * 4 + 16 * (MID_KPAD / 8) * 4;
static_assert(MID_SMEM <= 160 * 1024, "LDS budget: t 75.3 KB + weights 53.8 KB + taps 16 KB + bias + the two index tables");
static_assert(MID_ROWS % 16 == 0 && MID_ROWS / 16 <= 16, "a wave takes row groups wv and wv + 8");

struct MidParams {
  const void* x;
  void* y;
  const float* w25;   // (25, C) fp32 tap-major
  const float* scale; // (C)
  const float* shift; // (C)
  const void* wt;     // (160, 160) T: wt[n][k], zero-padded
  const float* bias;  // (160)
  int B, H, W, C, x_pitch, y_pitch;
  int S;              // strips per tile
  unsigned nstrip, ntile, band;
};

template <typename T>
__global__ __launch_bounds__(MID_NT) void refiner_mid_kernel(MidParams p) {
  constexpr int RS = MID_RS, OS = MID_KPAD + 8;
  static_assert(OS == RS * 8, "a staged output row is one row of t");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* s_t = reinterpret_cast<u32x4*>(smem);                         // [MID_ROWS][RS]  t, then the staged outputs
  u32x4* s_pw = s_t + MID_ROWS * RS;                                   // [160][RS]       1x1 weights, row = output channel
  float* s_w = reinterpret_cast<float*>(s_pw + MID_KPAD * RS);         // [25][C]         depthwise taps
  float* s_b = s_w + 25 * MID_KPAD;                                    // [160]
  int* s_pix = reinterpret_cast<int*>(s_b + MID_KPAD);                 // [MID_ROWS]      linear pixel of a row of t, -1: not stored
  int* s_item = s_pix + MID_ROWS;                                      // [320]           store item i of a row group: row << 8 | packet, -1 from 16 PK on
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = p.C, H = p.H, W = p.W, PK = C / 8, S = p.S;

  // ---- once per workgroup: weights, bias, taps ----
  for (int i = tid; i < MID_KPAD * (MID_KPAD / 8); i += MID_NT) {
    const int n = i / (MID_KPAD / 8), k = i % (MID_KPAD / 8);
    s_pw[n * RS + k] = reinterpret_cast<const u32x4*>(p.wt)[i];
  }
  for (int i = tid; i < 25 * C / 4; i += MID_NT) reinterpret_cast<float4_t*>(s_w)[i] = reinterpret_cast<const float4_t*>(p.w25)[i];
  for (int i = tid; i < MID_KPAD; i += MID_NT) s_b[i] = p.bias[i];
  for (int i = tid; i < MID_ROWS; i += MID_NT) s_pix[i] = -1;          // rows past 8 S stay -1
  // (a table: as divisions in the store loop, hipcc hoisted them out of the tile loop, 20 registers more than phase A leaves)
  for (int i = tid; i < 16 * (MID_KPAD / 8); i += MID_NT) s_item[i] = i < 16 * PK ? (i / PK) << 8 | (i % PK) : -1;
  __syncthreads();

  const T* x = static_cast<const T*>(p.x);
  T* y = static_cast<T*>(p.y);
  const unsigned WS = (unsigned)(W + mid::kStrip - 1) / mid::kStrip;
  const int sl = tid / PK, k = tid - sl * PK;                          // this thread's strip of the tile and channel packet
  const int ngrp = (S * mid::kStrip + 15) / 16;
  // tile order: XCD x (workgroup b runs on XCD b % 8) owns the contiguous eighth `band` of the tile sequence and its gridDim / 8
  // workgroups walk it side by side, as dwconv5x5_lds_kernel deals its items: the halo rows of a step are the L2-resident rows of
  // the step before
  const unsigned nx = gridDim.x >> 3;
  const unsigned beg = (blockIdx.x & 7u) * p.band;
  const unsigned end = min(beg + p.band, p.ntile);
  for (unsigned tile = beg + (blockIdx.x >> 3); tile < end; tile += nx) {
    // ---- phase A: depthwise + BN + ReLU of strip (tile, sl), packet k -> t ----
    if (sl < S) {
      const unsigned strip = tile * (unsigned)S + (unsigned)sl;
      if (strip < p.nstrip) {
        unsigned r = strip;
        const int xs = (int)(r % WS) * mid::kStrip;
        r /= WS;
        const int ys = (int)(r % (unsigned)H), b = (int)(r / (unsigned)H);
        u32x4* trow = s_t + sl * mid::kStrip * RS + k;
        mid::dw_strip<T>(x, s_w, p.scale, p.shift, b, ys, xs, k * 8, C, H, W, p.x_pitch, mid::kStrip,
                         [&](int o, const u32x4& v) { trow[o * RS] = v; });
        if (k == 0) {
          const int pix0 = (b * H + ys) * W + xs;
#pragma unroll
          for (int o = 0; o < mid::kStrip; ++o) s_pix[sl * mid::kStrip + o] = xs + o < W ? pix0 + o : -1;
        }
      } else if (k == 0) {
#pragma unroll
        for (int o = 0; o < mid::kStrip; ++o) s_pix[sl * mid::kStrip + o] = -1;
      }
    }
    __syncthreads();
    // ---- phase B: 1x1 of row groups wv and wv + 8 on the matrix cores, staged over the same rows of t, stored ----
    // (the lane index is made opaque per tile: phase A has no register to spare for phase B's addresses, which hipcc otherwise computes
    // once in front of the loop and keeps in scratch)
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));
    const int m = lane & 15, kq = lane >> 4;
    auto fragments = [&](int g, u32x4 (&a)[MID_KP]) {
#pragma unroll
      for (int ks = 0; ks < MID_KP; ++ks) {
        const int pk = 4 * ks + kq;
        u32x4 v = s_t[(g * 16 + m) * RS + (pk < PK ? pk : 0)];
        if (pk >= PK) v = u32x4{0, 0, 0, 0};
        a[ks] = v;
      }
    };
    // the 16 PK packets of a row group leave as 16-byte stores, 64 consecutive packets per wave instruction; unrolled over the items
    // of all G groups so that the index reads, the packet reads and the stores each go out back to back
    auto store_groups = [&](const int (&g)[2], auto ng) {
      constexpr int G = decltype(ng)::value, NIT = 16 * (MID_KPAD / 8) / 64;
      int item[NIT], pix[G][NIT];
#pragma unroll
      for (int j = 0; j < NIT; ++j) item[j] = s_item[lane + 64 * j];
#pragma unroll
      for (int q = 0; q < G; ++q)
#pragma unroll
        for (int j = 0; j < NIT; ++j) pix[q][j] = item[j] >= 0 ? s_pix[g[q] * 16 + (item[j] >> 8)] : -1;
#pragma unroll
      for (int q = 0; q < G; ++q) {
        const T* so = reinterpret_cast<const T*>(s_t + g[q] * 16 * RS);
#pragma unroll
        for (int j = 0; j < NIT; ++j)
          if (pix[q][j] >= 0)
            *reinterpret_cast<u32x4*>(y + (size_t)pix[q][j] * p.y_pitch + (item[j] & 255) * 8) =
                *reinterpret_cast<const u32x4*>(so + (item[j] >> 8) * OS + (item[j] & 255) * 8);
      }
    };
    if (wv + 8 < ngrp) {
      u32x4 a[2][MID_KP];
      fragments(wv, a[0]);
      fragments(wv + 8, a[1]);
      T* const stage[2] = {reinterpret_cast<T*>(s_t + wv * 16 * RS), reinterpret_cast<T*>(s_t + (wv + 8) * 16 * RS)};
      mid::pw_row_groups<T, MID_KP, 2>(a, s_pw, s_b, stage, m, kq);
      store_groups({wv, wv + 8}, std::integral_constant<int, 2>{});
    } else if (wv < ngrp) {
      u32x4 a[1][MID_KP];
      fragments(wv, a[0]);
      T* const stage[1] = {reinterpret_cast<T*>(s_t + wv * 16 * RS)};
      mid::pw_row_groups<T, MID_KP, 1>(a, s_pw, s_b, stage, m, kq);
      store_groups({wv, wv}, std::integral_constant<int, 1>{});
    }
    __syncthreads();                                                   // t and the pixel index are free for the next tile
  }
}

template <typename T>
int launch_mid(MidParams p, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  if (int rc = ensure_dyn_smem(reinterpret_cast<const void*>(refiner_mid_kernel<T>), MID_SMEM, attr_done, "roma_refiner_block_mid")) return rc;
  const int cus = num_cus() & ~7;                                     // 8 XCD bands: a multiple of 8 workgroups
  ROMA_REQUIRE(cus >= 8, ROMA_E_UNSUPPORTED, "roma_refiner_block_mid: needs a device with at least 8 compute units");
  const unsigned want = (p.ntile + 7u) & ~7u;
  const int grid = want < (unsigned)cus ? (int)want : cus;
  hipLaunchKernelGGL((refiner_mid_kernel<T>), dim3(grid), dim3(MID_NT), MID_SMEM, s, p);
  ROMA_CHECK_LAUNCH();
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" int roma_refiner_block_mid(const void* x, const float* w25, const float* scale, const float* shift, const void* wt,
                                      const float* bias, void* y, int B, int C, int H, int W, int dtype, int x_pitch, int y_pitch,
                                      void* stream) {
  ROMA_REQUIRE(x && w25 && scale && shift && wt && bias && y, ROMA_E_ARG, "roma_refiner_block_mid: null pointer");
  ROMA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && x_pitch >= C && y_pitch >= C, ROMA_E_SHAPE, "roma_refiner_block_mid: bad shape");
  ROMA_REQUIRE(dtype == ROMA_F16 || dtype == ROMA_BF16, ROMA_E_DTYPE, "roma_refiner_block_mid: fp16 / bf16 only");
  ROMA_REQUIRE(C > 32 && C <= MID_KPAD && C % 8 == 0, ROMA_E_UNSUPPORTED,
               "roma_refiner_block_mid: C=%d (a multiple of 8, 32 < C <= 160)", C);
  ROMA_REQUIRE(x_pitch % 8 == 0 && y_pitch % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(w25) && aligned16(scale) &&
                   aligned16(shift) && aligned16(wt),
               ROMA_E_ALIGN, "roma_refiner_block_mid: pitches must be multiples of 8 and bases 16-byte aligned");
  const size_t npix = (size_t)B * H * W;
  ROMA_REQUIRE(npix * x_pitch * 2 < (1ull << 32) && npix * y_pitch * 2 < (1ull << 32), ROMA_E_SHAPE,
               "roma_refiner_block_mid: a map of 4 GB or more in one launch");
  const char *xb = static_cast<const char*>(x), *yb = static_cast<const char*>(y);
  ROMA_REQUIRE(yb + npix * y_pitch * 2 <= xb || xb + npix * x_pitch * 2 <= yb, ROMA_E_ARG, "roma_refiner_block_mid: x and y overlap");
  MidParams p{x, y, w25, scale, shift, wt, bias, B, H, W, C, x_pitch, y_pitch, 0, 0, 0, 0};
  const int S0 = MID_NT / (C / 8);
  p.S = S0 < MID_SMAX ? S0 : MID_SMAX;                               // t holds 8 S rows; every strip of a tile has its PK threads
  p.nstrip = (unsigned)((size_t)B * H * ((W + mid::kStrip - 1) / mid::kStrip));
  p.ntile = (p.nstrip + p.S - 1) / p.S;
  p.band = (p.ntile + 7) / 8;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == ROMA_F16 ? launch_mid<half_t>(p, s) : launch_mid<bf16_t>(p, s);
}
