// local_correlation for gfx950 — reference: romatch/utils/local_correlation.py:4-48 (called at matcher.py:121-125).
//
// Formulation ("shared bilinear fraction"): the (2r+1)^2 window offsets are whole pixels, so every tap of
// one pixel shares one bilinear fraction (ax, ay).  With (x0,y0) = floor of the un-normalised flow target,
//     D[j][i] = <f0[:,y,x], f1[:, y0-r+j, x0-r+i]>      (0 <= i,j <= 2r+1, zero outside the image)
//     corr[k=(iy,ix)] = C^-1/2 * ((1-ay)(1-ax) D[iy][ix] + (1-ay)ax D[iy][ix+1] + ay(1-ax) D[iy+1][ix] + ay ax D[iy+1][ix+1])
// which never materialises the reference's (C,h,w,K) window tensor and needs (2r+2)^2 instead of 4(2r+1)^2 dot products.
//
// Mapping: one 256-thread workgroup owns a TW x TH tile of query pixels.  It computes the tile's bounding box of
// target positions, stages that box of f1 (a CC-channel chunk at a time, channels-last rows) and the tile's f0 rows in
// LDS, and every thread (pixel p, position group g) accumulates its NPOS dot products from LDS with packed dot2
// (fp16/bf16) or fma (fp32), fp32 accumulation.  D is exchanged through LDS for the 4-tap blend and written out
// coalesced.  Tiles whose bounding box does not fit in LDS (incoherent flow) read f1 rows straight from L2/HBM.
//
// This file: the dispatch of roma_local_corr and three kernels,
//   local_corr_kernel       any layout and dtype                      geometry and LDS layout: LCGeom<R>
//   local_corr_nhwc_kernel  fp32 channels-last, LDS-DMA staging                                LCFast<R>
//   local_corr_mfma_kernel  16-bit channels-last on the matrix cores, 8x4 / 4x4 tiles          LCM<R>
// The steps they have in common are defined once, ahead of the kernels: block id -> tile (tile_of_block), a pixel's target
// and clipped window (pixel_target, on lc::flow_target), the blend-and-store epilogue (blend_store), the ds_read_b128
// lane groups (lane_group) and the count of DMA rounds (dma_rounds).  Each geometry struct states its kernel's LDS layout
// once, as byte offsets and a total; the kernel carves the buffer up from the offsets and the launcher passes the total.
// Written out twice on purpose: the per-pixel-patch path ("mode B") of the fp32 kernel (the MA = false instantiation of its
// lambda) and of the MFMA kernel, the same algorithm with another swizzle, f0 row map and number of DMA rounds.  One
// routine templated on the row map left the MFMA kernel within its registers but not local_corr_nhwc_kernel<float, R>:
// r = 1 went from 68 to 80 VGPRs (7 -> 6 waves per SIMD), and the scratch of r = 2, 4, 7 from 32, 60, 152 to 44, 84, 160
// bytes per lane (gfx950, hipcc -O3; profiles/local_corr_shared_code.txt).
#include <type_traits>
#include <cstdlib>
#include "common.h"
#include "lc_variants.h"
#include "lc_device.h"

namespace roma {
namespace {

// what a kernel reads (the kernel choice and the LDS sizes are the launchers' business)
struct LCParams {
  const void* f0;
  const void* f1;
  const float* flow;
  void* out;
  int B, C, H, W;
  int f0_pitch, f1_pitch, out_pitch;
  int in_nhwc, out_nhwc;
  int tiles_x, tiles_y;
  int f1_shift;  // f1 batch item paired with f0's item b is (b + f1_shift) % B (forward_symmetric: B/2)
  float scale;   // C^-1/2
};

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------------------------
// Steps the three kernels of this file share.  Each is written once and inlined; the kernels keep what differs between
// them: the reduction of the pixel windows to a box, the staging and the dot products.
// ------------------------------------------------------------------------------------------------------------------

// element address of (b, c, y, x) in a feature map
__device__ __forceinline__ size_t feat_off(int nhwc, int b, int c, int y, int x, int pitch, int H, int W) {
  return nhwc ? (((size_t)b * H + y) * W + x) * pitch + c : (((size_t)b * pitch + c) * H + y) * W + x;
}

// block id -> batch item b and origin (ty0, tx0) of its TW x TH tile
struct LCTile { int b, ty0, tx0; };
template <int TW, int TH>
__device__ __forceinline__ LCTile tile_of_block(int tiles_x, int tiles_y) {
  const int ntile = tiles_x * tiles_y;
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = wid / ntile;
  const int t = wid - b * ntile;
  return {b, (t / tiles_x) * TH, (t % tiles_x) * TW};
}

// Target of image pixel (b, y, x): floor (x0, y0) and bilinear fraction (ax, ay) of the flow (identity grid without
// one) in pixels, and its window [x0-R, x0+R+1] x [y0-R, y0+R+1] clipped to the map; `hit` is false when the window
// misses the map (then lo > hi on some axis).
struct LCTarget { int x0, y0; float ax, ay; int lox, loy, hix, hiy; bool hit; };
template <int R>
__device__ __forceinline__ LCTarget pixel_target(const float* flow, int b, int y, int x, int H, int W) {
  LCTarget t;
  float fx, fy;
  if (flow) {
    fx = flow[((size_t)(b * 2 + 0) * H + y) * W + x];
    fy = flow[((size_t)(b * 2 + 1) * H + y) * W + x];
  } else {
    fx = -1.f + (2.f * x + 1.f) / W;
    fy = -1.f + (2.f * y + 1.f) / H;
  }
  lc::flow_target(fx, fy, H, W, t.x0, t.y0, t.ax, t.ay);
  t.lox = max(t.x0 - R, 0), t.hix = min(t.x0 + R + 1, W - 1);
  t.loy = max(t.y0 - R, 0), t.hiy = min(t.y0 + R + 1, H - 1);
  t.hit = t.lox <= t.hix && t.loy <= t.hiy;
  return t;
}

// Epilogue: 4-tap blend of the integer-grid products s_D[pix][(2R+2)^2 (+1 pad)] with each pixel's fraction.  Output
// element e of the tile's TP x (2R+1)^2 is (pixel, k) channels-last (consecutive threads = consecutive k of one pixel)
// or (k, pixel) planar (consecutive pixels of one k).
template <typename T, int R, int TP, int TW>
__device__ __forceinline__ void blend_store_at(int e, T* out, int out_nhwc, int out_pitch, int b, int ty0, int tx0, int H, int W,
                                               const float* s_D, const float* s_ax, const float* s_ay) {
  constexpr int N1 = 2 * R + 1, N2 = 2 * R + 2, Q = N2 * N2, K = N1 * N1;
  int pix, k;
  if (out_nhwc) { pix = e / K; k = e - pix * K; } else { k = e / TP; pix = e - k * TP; }
  const int y = ty0 + pix / TW, x = tx0 + pix % TW;
  if (y >= H || x >= W) return;
  const int iy = k / N1, ix = k - iy * N1;
  const float ax = s_ax[pix], ay = s_ay[pix];
  const float* d = s_D + pix * (Q + 1) + iy * N2 + ix;
  const float top = d[0] + ax * (d[1] - d[0]);
  const float bot = d[N2] + ax * (d[N2 + 1] - d[N2]);
  out[feat_off(out_nhwc, b, k, y, x, out_pitch, H, W)] = from_f32<T>(top + ay * (bot - top));
}
// The whole epilogue of one thread.  local_corr_nhwc_kernel writes this loop out instead: with the loop inlined from here
// its fp32 r = 4..7 instantiations, which sit at 128 VGPRs, spill 4 to 12 bytes more per lane (64/168/28/164 against 60/160/24/152
// bytes of scratch), while the MFMA kernel at r = 6 takes 136 instead of 116 VGPRs with the loop written out
// (profiles/local_corr_shared_code.txt).
template <typename T, int R, int TP, int TW>
__device__ __forceinline__ void blend_store(int tid, T* out, int out_nhwc, int out_pitch, int b, int ty0, int tx0, int H, int W,
                                            const float* s_D, const float* s_ax, const float* s_ay) {
  for (int e = tid; e < TP * (2 * R + 1) * (2 * R + 1); e += kThreads)
    blend_store_at<T, R, TP, TW>(e, out, out_nhwc, out_pitch, b, ty0, tx0, H, W, s_D, s_ax, s_ay);
}

// ds_read_b128 serves a wavefront in four fixed 16-lane groups: lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, and the
// same +32.  g16 = this thread's group among the workgroup's 16, idx = its place in the group.
struct LaneGroup { int g16, idx; };
__device__ __forceinline__ LaneGroup lane_group(int lane, int wave) {
  const int l5 = lane & 31;
  int hg, idx;
  if (l5 < 4) { hg = 0; idx = l5; }
  else if (l5 < 12) { hg = 1; idx = l5 - 4; }
  else if (l5 < 16) { hg = 0; idx = l5 - 8; }
  else if (l5 < 20) { hg = 1; idx = l5 - 8; }
  else if (l5 < 28) { hg = 0; idx = l5 - 12; }
  else { hg = 1; idx = l5 - 16; }
  return {wave * 4 + (lane >> 5) * 2 + hg, idx};
}

// LDS-DMA rounds (one round = 256 threads x 16 bytes = 64 rows of 64 bytes) that cover `rows` staged rows, 16 at a time
__host__ __device__ constexpr int dma_rounds(int rows) { return (((rows + 15) & ~15) * 4 + kThreads - 1) / kThreads; }

constexpr int pow2_floor(int v) { return v >= 16 ? 16 : v >= 8 ? 8 : v >= 4 ? 4 : v >= 2 ? 2 : 1; }

// LDS of the two LDS-DMA kernels (fp32 channels-last, 16-bit matrix cores), stated once for kernel and launcher: the
// DMA'd rows (TP f0 rows + up to MAXR staged rows, in whole rounds), 16 all-zero rows (never a DMA target), the products
// D[TP][Q+1], META words of boxes, then x0, y0, ax, ay per pixel.  Offsets in bytes.
template <int TP, int MAXR, int Q, int META> struct LCStagedLds {
  static constexpr int NL = dma_rounds(TP + MAXR);                  // DMA rounds of a full buffer
  static constexpr int ZROW = NL * (kThreads / 4);                  // first zero row
  static constexpr int ROWS_B = (NL * kThreads + 16 * 4) * 16, D_B = TP * (Q + 1) * 4, META_B = META * 4, PIX_B = TP * 4;
  static constexpr int OFF_D = ROWS_B, OFF_META = OFF_D + D_B;
  static constexpr int OFF_X0 = OFF_META + META_B, OFF_Y0 = OFF_X0 + PIX_B, OFF_AX = OFF_Y0 + PIX_B, OFF_AY = OFF_AX + PIX_B;
  static constexpr int BYTES = ROWS_B + D_B + META_B + 4 * PIX_B;
  static_assert(BYTES == OFF_AY + PIX_B, "LDS total != end of the last region");
};

// ------------------------------------------------------------------------------------------------------------------
// Any layout and dtype.  TP pixels x PG position groups = 256 threads; NPOS = ceil((2R+2)^2 / PG) positions per thread.
// LDS (bytes): 8 meta words, x0, y0, ax, ay per pixel, TP f0 rows, MAXROWS + 1 f1 rows (the last all zero); D[TP][Q+1]
// aliases the f1 rows after the channel loop.  A row is one position's channel chunk plus a 16-byte pad (odd stride in
// packets: no bank conflicts): 128 bytes of channels for small windows, 64 for r >= 4 (more rows fit).
// ------------------------------------------------------------------------------------------------------------------
template <int R> struct LCGeom {
  static constexpr int TW = R <= 5 ? 8 : 4, TH = R <= 3 ? 8 : 4, TP = TW * TH, PG = kThreads / TP;
  static constexpr int Q = (2 * R + 2) * (2 * R + 2);
  static constexpr int CHUNK_B = R >= 4 ? 64 : 128, ROW_B = CHUNK_B + 16;
  static constexpr int PIX_B = TP * 4;
  static constexpr int OFF_X0 = 8 * 4, OFF_Y0 = OFF_X0 + PIX_B, OFF_AX = OFF_Y0 + PIX_B, OFF_AY = OFF_AX + PIX_B;
  static constexpr int OFF_F0 = OFF_AY + PIX_B, OFF_F1 = OFF_F0 + TP * ROW_B;
  // about 60 KiB per workgroup so that two workgroups share a CU
  static constexpr int MAXROWS = (60 * 1024 - OFF_F1) / ROW_B - 1;  // capacity in f1 rows (excluding the zero row)
  static constexpr int F1_B = (MAXROWS + 1) * ROW_B, D_B = TP * (Q + 1) * 4;
  static constexpr int BYTES = 8 * 4 + 4 * PIX_B + TP * ROW_B + (F1_B > D_B ? F1_B : D_B);
  static_assert(BYTES == OFF_F1 + (F1_B > D_B ? F1_B : D_B), "LDS total != end of the last region");
};

template <typename T, int R, int CC>
__global__ __launch_bounds__(kThreads) void local_corr_kernel(LCParams p) {
  using G = LCGeom<R>;
  constexpr int TW = G::TW, TH = G::TH, TP = G::TP, PG = G::PG;
  constexpr int N2 = 2 * R + 2, Q = G::Q;
  constexpr int NPOS = (Q + PG - 1) / PG;
  constexpr int E16 = ElemTraits<T>::kPer16B;     // elements per 16-byte packet
  constexpr int PK = CC / E16;                    // packets per LDS row
  constexpr int ROW16 = G::ROW_B / 16;            // row stride in packets
  static_assert(CC * sizeof(T) == G::CHUNK_B && ROW16 == PK + 1, "chunk");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* s_meta = reinterpret_cast<int*>(smem);                 // [0..3] bbox
  int* s_x0 = reinterpret_cast<int*>(smem + G::OFF_X0);
  int* s_y0 = reinterpret_cast<int*>(smem + G::OFF_Y0);
  float* s_ax = reinterpret_cast<float*>(smem + G::OFF_AX);
  float* s_ay = reinterpret_cast<float*>(smem + G::OFF_AY);
  u32x4* s_f0 = reinterpret_cast<u32x4*>(smem + G::OFF_F0);   // TP rows
  u32x4* s_f1 = reinterpret_cast<u32x4*>(smem + G::OFF_F1);   // MAXROWS + 1 rows (last = zeros)
  float* s_D = reinterpret_cast<float*>(s_f1);                // aliased after the channel loop: [TP][Q+1]

  const int tid = threadIdx.x;
  const LCTile tile = tile_of_block<TW, TH>(p.tiles_x, p.tiles_y);
  const int b = tile.b, ty0 = tile.ty0, tx0 = tile.tx0;
  const int H = p.H, W = p.W;

  if (tid < 4) s_meta[tid] = (tid < 2) ? 0x7fffffff : -0x7fffffff;
  __syncthreads();
  if (tid < TP) {
    const int y = ty0 + tid / TW, x = tx0 + tid % TW;
    LCTarget t{};
    if (y < H && x < W) {
      t = pixel_target<R>(p.flow, b, y, x, H, W);
      if (t.hit) {
        atomicMin(&s_meta[0], t.lox);
        atomicMin(&s_meta[1], t.loy);
        atomicMax(&s_meta[2], t.hix);
        atomicMax(&s_meta[3], t.hiy);
      }
    }
    s_x0[tid] = t.x0;
    s_y0[tid] = t.y0;
    s_ax[tid] = t.ax;
    s_ay[tid] = t.ay;
  }
  __syncthreads();
  const int bx0 = s_meta[0], by0 = s_meta[1];
  const bool empty = s_meta[2] < bx0 || s_meta[3] < by0;       // every window of the tile is outside the image
  const int bw = empty ? 0 : s_meta[2] - bx0 + 1, bh = empty ? 0 : s_meta[3] - by0 + 1;
  const int nrows = bw * bh;
  const bool staged = nrows <= G::MAXROWS;                   // else: read f1 rows from global memory directly
  const int zero_row = staged ? nrows : 0;

  // per-thread work list: pixel pp, positions q = g*NPOS .. g*NPOS+NPOS-1
  const int pp = tid % TP, g = tid / TP;
  const int my_x0 = s_x0[pp], my_y0 = s_y0[pp];
  const int py_img = ty0 + pp / TW, px_img = tx0 + pp % TW;
  const bool pvalid = (py_img < H) && (px_img < W);
  int rowoff[NPOS];      // staged: LDS row index; direct: pixel index y*W+x (or -1)
#pragma unroll
  for (int i = 0; i < NPOS; ++i) {
    const int q = g * NPOS + i;
    const int yy = my_y0 - R + q / N2, xx = my_x0 - R + q % N2;
    const bool ok = pvalid && (q < Q) && (yy >= 0) && (yy < H) && (xx >= 0) && (xx < W);
    rowoff[i] = staged ? (ok ? (yy - by0) * bw + (xx - bx0) : zero_row) : (ok ? yy * W + xx : -1);
  }
  float acc[NPOS];
#pragma unroll
  for (int i = 0; i < NPOS; ++i) acc[i] = 0.f;

  const T* f0 = static_cast<const T*>(p.f0);
  const T* f1 = static_cast<const T*>(p.f1);
  const int b1 = (b + p.f1_shift) % p.B;
  if (staged) {                                                // zero row
    for (int i = tid; i < ROW16; i += kThreads) s_f1[zero_row * ROW16 + i] = u32x4{0, 0, 0, 0};
  }

  for (int c0 = 0; c0 < p.C; c0 += CC) {
    // ---- stage f0 tile rows and the f1 bounding box (channels c0..c0+CC) ----
    if (p.in_nhwc) {
      for (int i = tid; i < TP * PK; i += kThreads) {
        const int row = i / PK, k = i - row * PK;
        const int y = ty0 + row / TW, x = tx0 + row % TW;
        u32x4 v{0, 0, 0, 0};
        if (y < H && x < W && c0 + k * E16 < p.C)
          v = *reinterpret_cast<const u32x4*>(f0 + feat_off(1, b, c0 + k * E16, y, x, p.f0_pitch, H, W));
        s_f0[row * ROW16 + k] = v;
      }
      if (staged) {
        for (int i = tid; i < nrows * PK; i += kThreads) {
          const int row = i / PK, k = i - row * PK;
          const int y = by0 + row / bw, x = bx0 + row % bw;
          u32x4 v{0, 0, 0, 0};
          if (c0 + k * E16 < p.C)
            v = *reinterpret_cast<const u32x4*>(f1 + feat_off(1, b1, c0 + k * E16, y, x, p.f1_pitch, H, W));
          s_f1[row * ROW16 + k] = v;
        }
      }
    } else {
      // planar input: lanes run along x (contiguous), LDS write transposes to channels-last rows
      T* s0 = reinterpret_cast<T*>(s_f0);
      for (int i = tid; i < TP * CC; i += kThreads) {
        const int c = i / TP, row = i - c * TP;
        const int y = ty0 + row / TW, x = tx0 + row % TW;
        T v = from_f32<T>(0.f);
        if (y < H && x < W && c0 + c < p.C) v = f0[feat_off(0, b, c0 + c, y, x, p.f0_pitch, H, W)];
        s0[row * ROW16 * E16 + c] = v;
      }
      if (staged) {
        T* s1 = reinterpret_cast<T*>(s_f1);
        for (int i = tid; i < nrows * CC; i += kThreads) {
          const int c = i / nrows, row = i - c * nrows;
          const int y = by0 + row / bw, x = bx0 + row % bw;
          T v = from_f32<T>(0.f);
          if (c0 + c < p.C) v = f1[feat_off(0, b1, c0 + c, y, x, p.f1_pitch, H, W)];
          s1[row * ROW16 * E16 + c] = v;
        }
      }
    }
    __syncthreads();
    // ---- dot products ----
    u32x4 a[PK];
#pragma unroll
    for (int k = 0; k < PK; ++k) a[k] = s_f0[pp * ROW16 + k];
    if (staged) {
#pragma unroll
      for (int i = 0; i < NPOS; ++i) {
        const u32x4* row = s_f1 + rowoff[i] * ROW16;
        float s = acc[i];
#pragma unroll
        for (int k = 0; k < PK; ++k) s = dot16<T>(a[k], row[k], s);
        acc[i] = s;
      }
    } else {
      // incoherent tile: f1 rows come straight from L2/HBM (correct for any flow, not the fast path)
      const T* a_el = reinterpret_cast<const T*>(s_f0 + pp * ROW16);
#pragma unroll
      for (int i = 0; i < NPOS; ++i) {
        if (rowoff[i] >= 0) {
          const int yy = rowoff[i] / W, xx = rowoff[i] - yy * W;
          float s = acc[i];
          if (p.in_nhwc) {
            const T* src = f1 + feat_off(1, b1, c0, yy, xx, p.f1_pitch, H, W);
#pragma unroll 1
            for (int k = 0; k < PK; ++k)
              if (c0 + k * E16 < p.C)
                s = dot16<T>(s_f0[pp * ROW16 + k], *reinterpret_cast<const u32x4*>(src + k * E16), s);
          } else {
#pragma unroll 1
            for (int c = 0; c < CC && c0 + c < p.C; ++c)
              s = __builtin_fmaf(to_f32(a_el[c]), to_f32(f1[feat_off(0, b1, c0 + c, yy, xx, p.f1_pitch, H, W)]), s);
          }
          acc[i] = s;
        }
      }
    }
    __syncthreads();
  }

  // ---- exchange D through LDS, blend, write ----
#pragma unroll
  for (int i = 0; i < NPOS; ++i) {
    const int q = g * NPOS + i;
    if (q < Q) s_D[pp * (Q + 1) + q] = acc[i] * p.scale;
  }
  __syncthreads();
  blend_store<T, R, TP, TW>(tid, static_cast<T*>(p.out), p.out_nhwc, p.out_pitch, b, ty0, tx0, H, W, s_D, s_ax, s_ay);
}


// ------------------------------------------------------------------------------------------------------------------
// Channels-last fast path.
//  * The tile's box of f1 rows is staged 64 bytes of channels at a time by LDS-DMA (global_load_lds_dwordx4: no VGPR
//    round trip, no ds_write), with a per-thread source-address plan computed once; every DMA is unconditional.
//  * LDS rows are 64 bytes, unpadded (an LDS-DMA wave-instruction writes 1 KiB linearly), with the packet index
//    XOR-swizzled by (row >> 2) & 3: any 16 rows with distinct (row mod 16) then occupy 16 distinct 16-byte slots.
//  * LDS reads are bank-conflict free BY CONSTRUCTION, for any flow: ds_read_b128 serves a wavefront in four fixed
//    16-lane groups; each group works on ONE pixel at a time, its 16 lanes take 16 consecutive window positions
//    q = 16 t + idx (runs of 2r+2 consecutive target columns over consecutive target rows), and the staged box uses a
//    row pitch congruent to (2r+2) mod 16, so the runs tile the 16 residues.  The pixel's f0 row is a broadcast read.
//    (A thread-per-pixel mapping measured 56 % of all LDS cycles as bank conflicts, profiles/r01_local_corr_pmc.md.)
//  * 32-pixel tiles (16 for r >= 6) and <= 30 KiB of LDS per workgroup: 5 workgroups per CU hide the DMA latency of
//    one another (single LDS buffer, two barriers per chunk).
// ------------------------------------------------------------------------------------------------------------------
template <int R> struct LCFast {
  static constexpr int TP = R <= 5 ? 32 : 16;                       // pixels per tile
  static constexpr int TW = R <= 5 ? 8 : 4, TH = TP / TW;
  static constexpr int MAXR = R <= 3 ? 384 : (R <= 5 ? 512 : 640);  // LDS capacity in staged rows (multiple of 16)
  using Lds = LCStagedLds<TP, MAXR, (2 * R + 2) * (2 * R + 2), 8>;  // meta: [0..3] tile box
};

__device__ __forceinline__ int swz(int row, int k) { return row * 4 + (k ^ ((row >> 2) & 3)); }

// one LDS-DMA wave-instruction: lane i of the wavefront copies 16 bytes from its own global address to
// lds_wave_base + 16*i (the LDS side is wave-uniform base + lane*16 by hardware definition)
__device__ __forceinline__ void dma16(const void* gsrc, unsigned char* lds_wave_base) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
#endif
}

template <typename T, int R>
__global__ __launch_bounds__(kThreads, 4) void local_corr_nhwc_kernel(LCParams p) {   // <= 128 VGPRs: 4 workgroups / CU
  using G = LCFast<R>;
  using L = typename G::Lds;
  constexpr int TW = G::TW, TH = G::TH, TP = G::TP;
  constexpr int N2 = 2 * R + 2, Q = N2 * N2;
  constexpr int NPIX = TP / 16;                 // pixels handled (one after the other) by each 16-lane group
  constexpr int NIT = (Q + 15) / 16;            // window positions per lane and pixel
  constexpr int QP = NIT * 16;                  // rows of one per-pixel patch (mode B)
  constexpr int E16 = ElemTraits<T>::kPer16B;
  constexpr int PK = 4, CC = PK * E16;
  constexpr int MAXR = G::MAXR;
  constexpr int SB = pow2_floor(MAXR / QP);     // pixels whose private patches fit in LDS together (mode B)
  constexpr int NL = L::NL, ZROW = L::ZROW;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* s_rows = reinterpret_cast<u32x4*>(smem);             // row r, packet k at s_rows[swz(r, k)]
  float* s_D = reinterpret_cast<float*>(smem + L::OFF_D);     // [TP][Q+1] integer-grid dot products
  int* s_meta = reinterpret_cast<int*>(smem + L::OFF_META);
  int* s_x0 = reinterpret_cast<int*>(smem + L::OFF_X0);
  int* s_y0 = reinterpret_cast<int*>(smem + L::OFF_Y0);
  float* s_ax = reinterpret_cast<float*>(smem + L::OFF_AX);
  float* s_ay = reinterpret_cast<float*>(smem + L::OFF_AY);

  const int tid = threadIdx.x;
  const LCTile tile = tile_of_block<TW, TH>(p.tiles_x, p.tiles_y);
  const int b = tile.b, ty0 = tile.ty0, tx0 = tile.tx0;
  const int H = p.H, W = p.W;

  if (tid < 4) s_meta[tid] = (tid < 2) ? 0x7fffffff : -0x7fffffff;
  for (int i = tid; i < 16 * PK; i += kThreads) s_rows[ZROW * PK + i] = u32x4{0, 0, 0, 0};
  __syncthreads();
  if (tid < TP) {
    const int y = ty0 + tid / TW, x = tx0 + tid % TW;
    LCTarget t{};
    if (y < H && x < W) {
      t = pixel_target<R>(p.flow, b, y, x, H, W);
      if (t.hit) {
        atomicMin(&s_meta[0], t.lox);
        atomicMin(&s_meta[1], t.loy);
        atomicMax(&s_meta[2], t.hix);
        atomicMax(&s_meta[3], t.hiy);
      }
    }
    s_x0[tid] = t.x0;
    s_y0[tid] = t.y0;
    s_ax[tid] = t.ax;
    s_ay[tid] = t.ay;
  }
  __syncthreads();
  const int bx0 = s_meta[0], by0 = s_meta[1];
  const bool empty = s_meta[2] < bx0 || s_meta[3] < by0;
  const int bw = empty ? 0 : s_meta[2] - bx0 + 1, bh = empty ? 0 : s_meta[3] - by0 + 1;
  // LDS row pitch of the box: smallest value >= bw congruent to (2r+2) mod 16 (a full 16-wide window needs none)
  const int bwp = (empty || N2 == 16) ? bw : bw + ((N2 - bw) & 15);
  // mode A: the whole tile shares one staged box (coherent flow).  mode B: the box is too large (incoherent flow):
  // SB pixels at a time get a private (2r+2)^2 patch each (16-row aligned), several passes.
  const bool modeA = bwp * bh <= MAXR;

  const LaneGroup lg = lane_group(tid & 63, tid >> 6);
  const int g16 = lg.g16, idx = lg.idx;
  const T* f0 = static_cast<const T*>(p.f0) + (size_t)b * H * W * p.f0_pitch;
  const T* f1 = static_cast<const T*>(p.f1) + (size_t)((b + p.f1_shift) % p.B) * H * W * p.f1_pitch;

  // The two modes are separate instantiations of one lambda so that each keeps its own (small) register set.
  // A work item = 16 consecutive window positions (one "iteration" it) of one pixel, reduced by one 16-lane group.
  //   mode A: group g16 owns pixels a*16+g16 and all NIT iterations of each               -> NPIX*NIT items
  //   mode B: the SB*NIT items of the pass are dealt round-robin to the 16 groups           -> UB items
  auto run = [&](auto mode_tag) {
    constexpr bool MA = decltype(mode_tag)::value;
    constexpr int UB = (SB * NIT + 15) / 16;
    constexpr int WN = MA ? NPIX * NIT : UB;
    const int npasses = MA ? 1 : (TP + SB - 1) / SB;
    for (int pass = 0; pass < npasses; ++pass) {
      int pixw[WN], qw[WN], rowidx[WN];
      float acc[WN];
#pragma unroll
      for (int w = 0; w < WN; ++w) {
        int pix, it, slot = 0;
        if (MA) {
          pix = (w / NIT) * 16 + g16;
          it = w % NIT;
        } else {
          const int u = g16 + 16 * w;
          slot = u / NIT;
          it = u - slot * NIT;
          pix = (u < SB * NIT) ? pass * SB + slot : TP;
        }
        const bool pact = pix < TP;
        pix = pact ? pix : 0;
        const bool pvalid = pact && (ty0 + pix / TW < H) && (tx0 + pix % TW < W);
        const int q = it * 16 + idx;
        const int yy = s_y0[pix] - R + q / N2, xx = s_x0[pix] - R + q % N2;
        const bool ok = pvalid && (q < Q) && (yy >= 0) && (yy < H) && (xx >= 0) && (xx < W);
        const int row = MA ? TP + (yy - by0) * bwp + (xx - bx0) : TP + slot * QP + q;
        pixw[w] = pvalid ? pix : -1;
        qw[w] = q;
        rowidx[w] = ok ? row : ZROW;
        acc[w] = 0.f;
      }
      // ---- DMA plan: LDS packet slot s = l*256 + tid holds (row = s/4, k = (s%4) ^ ((row>>2)&3)); its global source
      // is fixed for the whole channel loop.  Slots that hold nothing read a valid dummy address, never consumed. ----
      const T* src[NL];
      const int used_rows = TP + (MA ? bwp * bh : SB * QP);
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const int slot = l * kThreads + tid;
        const int row = slot >> 2;
        const int k = (slot & 3) ^ ((row >> 2) & 3);
        int y = ty0, x = tx0, pitch = p.f0_pitch;
        const T* base = f0;
        if (row < TP) {
          y = min(ty0 + row / TW, H - 1);
          x = min(tx0 + row % TW, W - 1);
        } else if (row < used_rows) {
          const int rr = row - TP;
          if (MA) {
            const int ry = rr / bwp, rx = rr - ry * bwp;
            if (rx < bw) {
              y = by0 + ry;
              x = bx0 + rx;
              base = f1;
              pitch = p.f1_pitch;
            }
          } else {
            const int sl = rr / QP, q = rr - sl * QP;
            const int pix = pass * SB + sl;
            if (pix < TP && q < Q) {
              y = min(max(s_y0[pix] - R + q / N2, 0), H - 1);
              x = min(max(s_x0[pix] - R + q % N2, 0), W - 1);
              base = f1;
              pitch = p.f1_pitch;
            }
          }
        }
        src[l] = base + ((size_t)y * W + x) * pitch + k * E16;
      }
      const int nl_used = dma_rounds(used_rows);                // DMA rounds that carry data
      for (int c0 = 0; c0 < p.C; c0 += CC) {
#pragma unroll
        for (int l = 0; l < NL; ++l)
          if (l < nl_used) dma16(src[l] + c0, smem + (size_t)(l * kThreads + (tid & ~63)) * 16);
        __syncthreads();                                        // vmcnt(0) + barrier: the chunk has landed
        u32x4 fa[PK];
#pragma unroll
        for (int w = 0; w < WN; ++w) {
          if (!MA || w % NIT == 0) {                            // the pixel's own f0 row: broadcast within the group
            const int prow = pixw[w] < 0 ? 0 : pixw[w];
#pragma unroll
            for (int k = 0; k < PK; ++k) fa[k] = s_rows[swz(prow, k)];
          }
          const int r0 = rowidx[w];
          const int sw = (r0 >> 2) & 3;
          float sacc = acc[w];
#pragma unroll
          for (int k = 0; k < PK; ++k) sacc = dot16<T>(fa[k], s_rows[r0 * 4 + (k ^ sw)], sacc);
          acc[w] = sacc;
        }
        __syncthreads();                                        // everyone is done reading before the next DMA lands
      }
#pragma unroll
      for (int w = 0; w < WN; ++w)
        if (qw[w] < Q && pixw[w] >= 0) s_D[pixw[w] * (Q + 1) + qw[w]] = acc[w] * p.scale;
    }
  };
  if (modeA) run(std::true_type{}); else run(std::false_type{});
  __syncthreads();
  T* out = static_cast<T*>(p.out);
  for (int e = tid; e < TP * (2 * R + 1) * (2 * R + 1); e += kThreads)     // blend_store's loop, written out: see its comment
    blend_store_at<T, R, TP, TW>(e, out, p.out_nhwc, p.out_pitch, b, ty0, tx0, H, W, s_D, s_ax, s_ay);
}

template <typename T, int R>
int launch_lc_nhwc(LCParams p, hipStream_t stream) {
  using G = LCFast<R>;
  p.tiles_x = (p.W + G::TW - 1) / G::TW;
  p.tiles_y = (p.H + G::TH - 1) / G::TH;
  const int grid = p.B * p.tiles_x * p.tiles_y;
  hipLaunchKernelGGL((local_corr_nhwc_kernel<T, R>), dim3(grid), dim3(kThreads), G::Lds::BYTES, stream, p);
  ROMA_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------------
// fp16 / bf16 channels-last path on the matrix cores.
// PMC showed the VALU version issue-bound (2.7x more VALU instructions than the minimum dot2 count), not HBM-bound, so
// the dot products move to v_mfma_f32_16x16x32_{f16,bf16}: M = the 16 pixels of a 4x4 group, N = 16 horizontally
// consecutive target positions of one row of the group's union window, K = 32 channels = one 64-byte LDS row chunk.
// A fragment (the group's f0 rows) is read once per chunk and reused for every block; each B fragment is one
// ds_read_b128 of 16 consecutive staged rows.  Rows are XOR-swizzled by (row>>2)&1 and the four K-slices are assigned to
// the lane quarters in the order (0,2,1,3): with the fixed ds_read_b128 lane groups this is bank-conflict free for any
// row base (exhaustive search, tools/scratch).  Each lane scatters the products that fall in its pixels' own windows
// straight into the per-pixel (2r+2)^2 images the 4-tap blend reads.  Only 1/4-1/3 of the computed products are used (every pixel needs (2r+2)^2 of the union's positions),
// which the 16x MFMA rate absorbs.  Tiles whose groups are not compact (incoherent flow) use per-pixel patches on the
// VALU (mode B of the kernel above, same staging).
// ------------------------------------------------------------------------------------------------------------------
template <int R> struct LCM {
  static constexpr int NG = R <= 3 ? 2 : 1;                  // 4x4-pixel groups per tile (16x4 tiles for r <= 2: +5 % coherent, -10 % incoherent)
  static constexpr int TP = 16 * NG, TW = 4 * NG, TH = 4;
  static constexpr int WPG = 4 / NG;                         // wavefronts per group
  static constexpr int N2 = 2 * R + 2;
  static constexpr int NRUN = N2 <= 10 ? 1 : 2;              // 16-position runs per union row
  static constexpr int WC = 16 * NRUN;                       // union columns a group may span
  static constexpr int GHMAX = N2 + 10;                      // union rows a group may span
  static constexpr int NB = (GHMAX * NRUN + WPG - 1) / WPG;  // accumulator blocks per wavefront
  static constexpr int MAXR = R <= 3 ? 384 : 704;            // staged rows
  using Lds = LCStagedLds<TP, MAXR, N2 * N2, 8 + 4 * NG>;    // meta: [0..3] tile box, [8+4g ..] group boxes
};

template <typename T, int R>
__global__ __launch_bounds__(kThreads, 2) void local_corr_mfma_kernel(LCParams p) {
  using M = LCM<R>;
  constexpr int NG = M::NG, TP = M::TP, TW = M::TW, TH = M::TH, WPG = M::WPG, NRUN = M::NRUN, WC = M::WC;
  constexpr int GHMAX = M::GHMAX, NB = M::NB, MAXR = M::MAXR;
  constexpr int N2 = 2 * R + 2, Q = N2 * N2;
  constexpr int NIT = (Q + 15) / 16, QP = NIT * 16;
  constexpr int E16 = 8, PK = 4, CC = PK * E16;
  constexpr int SB = pow2_floor(MAXR / QP);
  using L = typename M::Lds;
  constexpr int NL = L::NL, ZROW = L::ZROW;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* s_rows = reinterpret_cast<u32x4*>(smem);             // staged rows, packet k of row r at s_rows[lc::swzr(r, k)]
  float* s_D = reinterpret_cast<float*>(smem + L::OFF_D);     // [TP][Q+1] per-pixel window images
  int* s_meta = reinterpret_cast<int*>(smem + L::OFF_META);   // [0..3] tile box, [8+4g ..] group boxes
  int* s_x0 = reinterpret_cast<int*>(smem + L::OFF_X0);
  int* s_y0 = reinterpret_cast<int*>(smem + L::OFF_Y0);
  float* s_ax = reinterpret_cast<float*>(smem + L::OFF_AX);
  float* s_ay = reinterpret_cast<float*>(smem + L::OFF_AY);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LCTile tile = tile_of_block<TW, TH>(p.tiles_x, p.tiles_y);
  const int b = tile.b, ty0 = tile.ty0, tx0 = tile.tx0;
  const int H = p.H, W = p.W;

  for (int i = tid; i < 16 * PK; i += kThreads) s_rows[ZROW * PK + i] = u32x4{0, 0, 0, 0};
  for (int i = tid; i < TP * (Q + 1); i += kThreads) s_D[i] = 0.f;
  // ---- per-pixel targets and the tile / group boxes: the TP pixel threads are the low lanes of wavefront 0, so the
  // boxes are wavefront shuffles (the first version used 8 LDS atomics per pixel + two more barriers: 21 % of the
  // kernel in the ablation of DESIGN.md §3.1) ----
  if (wave == 0) {
    const int y = ty0 + tid / TW, x = tx0 + tid % TW;
    LCTarget t{};
    int lox = 0x3fffffff, loy = 0x3fffffff, hix = -0x3fffffff, hiy = -0x3fffffff;
    if (tid < TP && y < H && x < W) {
      t = pixel_target<R>(p.flow, b, y, x, H, W);
      if (t.hit) { lox = t.lox; hix = t.hix; loy = t.loy; hiy = t.hiy; }
    }
    if (tid < TP) {
      s_x0[tid] = t.x0;
      s_y0[tid] = t.y0;
      s_ax[tid] = t.ax;
      s_ay[tid] = t.ay;
    }
    // pixel tid = (ty, tx) = (tid / TW, tid % TW); its 4x4 group is tx >> 2.  Reduce over every lane bit except the
    // group bit(s) first (group boxes), then over those (tile box).  Lanes >= TP carry neutral values.
    constexpr int GMASK = (TW - 1) & ~3;                     // lane bits that select the group: 4 for TW = 8, 0 for TW = 4
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
      if (!(o & GMASK)) {
        lox = min(lox, __shfl_xor(lox, o, 64)); loy = min(loy, __shfl_xor(loy, o, 64));
        hix = max(hix, __shfl_xor(hix, o, 64)); hiy = max(hiy, __shfl_xor(hiy, o, 64));
      }
    // lane 4g holds group g's box (tx = 4g, ty = 0)
    if ((tid & ~GMASK) == 0 && tid < TW) {
      int* gm = s_meta + 8 + 4 * (tid >> 2);
      gm[0] = lox; gm[1] = loy; gm[2] = hix; gm[3] = hiy;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
      if (o & GMASK) {
        lox = min(lox, __shfl_xor(lox, o, 64)); loy = min(loy, __shfl_xor(loy, o, 64));
        hix = max(hix, __shfl_xor(hix, o, 64)); hiy = max(hiy, __shfl_xor(hiy, o, 64));
      }
    if (tid == 0) { s_meta[0] = lox; s_meta[1] = loy; s_meta[2] = hix; s_meta[3] = hiy; }
  }
  __syncthreads();
  const int bx0 = s_meta[0], by0 = s_meta[1];
  const bool empty = s_meta[2] < bx0 || s_meta[3] < by0;
  const int bw = empty ? 0 : s_meta[2] - bx0 + 1, bh = empty ? 0 : s_meta[3] - by0 + 1;
  bool eligible = bw * bh <= MAXR;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int* gm = s_meta + 8 + 4 * g;
    if (gm[2] >= gm[0] && gm[3] >= gm[1]) eligible = eligible && (gm[2] - gm[0] + 1 <= WC) && (gm[3] - gm[1] + 1 <= GHMAX);
  }
  const T* f0 = static_cast<const T*>(p.f0) + (size_t)b * H * W * p.f0_pitch;
  const T* f1 = static_cast<const T*>(p.f1) + (size_t)((b + p.f1_shift) % p.B) * H * W * p.f1_pitch;
  T* out = static_cast<T*>(p.out);
  // LDS row of pixel (ty,tx)'s f0: group-major so that a group's 16 rows are consecutive (A fragment = one b128 each)
  auto frow = [&](int pix) { const int ty = pix / TW, tx = pix % TW; return (tx >> 2) * 16 + ty * 4 + (tx & 3); };
  auto fpix = [&](int row, int& y, int& x) { const int g = row >> 4, m = row & 15; y = ty0 + (m >> 2); x = tx0 + 4 * g + (m & 3); };

  if (eligible) {
    // =========================== matrix-core path ===========================
    const float inv_bw = 1.0f / (float)bw;
    const T* src[NL];
    const int used_rows = TP + bw * bh;
    const int nl_used = dma_rounds(used_rows);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (l >= nl_used) { src[l] = f0; continue; }            // never issued
      const int slot = l * kThreads + tid;
      const int row = slot >> 2;
      const int k = (slot & 3) ^ ((row >> 2) & 1);
      int y = ty0, x = tx0, pitch = p.f0_pitch;
      const T* base = f0;
      if (row < TP) {
        fpix(row, y, x);
        y = min(y, H - 1);
        x = min(x, W - 1);
      } else if (row < used_rows) {
        const int rr = row - TP;
        const int ry = min((int)(((float)rr + 0.5f) * inv_bw), bh - 1);   // rr / bw, exact for these small integers
        y = by0 + ry;
        x = bx0 + rr - ry * bw;
        base = f1;
        pitch = p.f1_pitch;
      }
      src[l] = base + ((size_t)y * W + x) * pitch + k * E16;
    }
    const int gi = wave / WPG, sub = wave % WPG;
    const int* gm = s_meta + 8 + 4 * gi;
    const bool gempty = gm[2] < gm[0] || gm[3] < gm[1];
    const int gx0 = gm[0], gy0 = gm[1];
    const int gh = gempty ? 0 : gm[3] - gy0 + 1, gw = gempty ? 0 : gm[2] - gx0 + 1;
    const int n = lane & 15, kg = lane >> 4;
    const int ks = (kg == 1) ? 2 : (kg == 2 ? 1 : kg);          // K-slice of this lane quarter: (0,2,1,3)
    int bidx[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int blk = sub + WPG * j;
      const int ry = blk / NRUN, run = blk - ry * NRUN;
      const int row = (blk < gh * NRUN ? TP + (gy0 - by0 + ry) * bw + (gx0 - bx0 + 16 * run) : ZROW) + n;
      bidx[j] = lc::swzr(row, ks);
    }
    const int aidx = lc::swzr(gi * 16 + n, ks);
    float4_t acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < p.C; c0 += CC) {
#pragma unroll
      for (int l = 0; l < NL; ++l)
        if (l < nl_used) dma16(src[l] + c0, smem + (size_t)(l * kThreads + (tid & ~63)) * 16);
      __syncthreads();
      const u32x4 a = s_rows[aidx];
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = lc::mfma16r(a, s_rows[bidx[j]], acc[j], T{});
      __syncthreads();
    }
    // accumulators -> the per-pixel window images s_D[pix][dy*N2+dx] directly: lane (n, kg) of block (ry, run) holds the
    // products of pixels m = 4kg..4kg+3 of the group with union position (gy0+ry, gx0+16run+n); each pixel keeps the
    // (2r+2)^2 of them that fall in its own window (positions outside the image are never written: s_D starts at 0)
    {
      int wx[4], wy[4], pixs[4];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int m = 4 * kg + r4;
        pixs[r4] = (m >> 2) * TW + 4 * gi + (m & 3);
        wx[r4] = s_x0[pixs[r4]] - R;
        wy[r4] = s_y0[pixs[r4]] - R;
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int blk = sub + WPG * j;
        const int ry = blk / NRUN, run = blk - ry * NRUN;
        if (blk < gh * NRUN && 16 * run + n < gw) {             // inside the group's (image-clamped) box: the rest of a
          const int ya = gy0 + ry, xa = gx0 + 16 * run + n;     // 16-wide run wraps into other rows / unstaged LDS
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int dy = ya - wy[r4], dx = xa - wx[r4];
            if (dy >= 0 && dy < N2 && dx >= 0 && dx < N2) s_D[pixs[r4] * (Q + 1) + dy * N2 + dx] = acc[j][r4] * p.scale;
          }
        }
      }
    }
    __syncthreads();
    blend_store<T, R, TP, TW>(tid, out, p.out_nhwc, p.out_pitch, b, ty0, tx0, H, W, s_D, s_ax, s_ay);
    return;
  }

  // =========================== incoherent tile: per-pixel patches on the VALU (mode B) ===========================
  const LaneGroup lg = lane_group(lane, wave);
  const int g16 = lg.g16, idx = lg.idx;
  constexpr int UB = (SB * NIT + 15) / 16;
  for (int pass = 0; pass < (TP + SB - 1) / SB; ++pass) {
    int pixw[UB], qw[UB], rowidx[UB];
    float acc[UB];
#pragma unroll
    for (int w = 0; w < UB; ++w) {
      const int u = g16 + 16 * w;
      const int slot = u / NIT, it = u - slot * NIT;
      int pix = (u < SB * NIT) ? pass * SB + slot : TP;
      const bool pact = pix < TP;
      pix = pact ? pix : 0;
      const bool pvalid = pact && (ty0 + pix / TW < H) && (tx0 + pix % TW < W);
      const int q = it * 16 + idx;
      const int yy = s_y0[pix] - R + q / N2, xx = s_x0[pix] - R + q % N2;
      const bool ok = pvalid && (q < Q) && (yy >= 0) && (yy < H) && (xx >= 0) && (xx < W);
      pixw[w] = pvalid ? pix : -1;
      qw[w] = q;
      rowidx[w] = ok ? TP + slot * QP + q : ZROW;
      acc[w] = 0.f;
    }
    const T* src[NL];
    const int used_rows = TP + SB * QP;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int slot = l * kThreads + tid;
      const int row = slot >> 2;
      const int k = (slot & 3) ^ ((row >> 2) & 1);
      int y = ty0, x = tx0, pitch = p.f0_pitch;
      const T* base = f0;
      if (row < TP) {
        fpix(row, y, x);
        y = min(y, H - 1);
        x = min(x, W - 1);
      } else if (row < used_rows) {
        const int rr = row - TP;
        const int sl = rr / QP, q = rr - sl * QP;
        const int pix = pass * SB + sl;
        if (pix < TP && q < Q) {
          y = min(max(s_y0[pix] - R + q / N2, 0), H - 1);
          x = min(max(s_x0[pix] - R + q % N2, 0), W - 1);
          base = f1;
          pitch = p.f1_pitch;
        }
      }
      src[l] = base + ((size_t)y * W + x) * pitch + k * E16;
    }
    const int nl_used = dma_rounds(used_rows);
    for (int c0 = 0; c0 < p.C; c0 += CC) {
#pragma unroll
      for (int l = 0; l < NL; ++l)
        if (l < nl_used) dma16(src[l] + c0, smem + (size_t)(l * kThreads + (tid & ~63)) * 16);
      __syncthreads();
#pragma unroll
      for (int w = 0; w < UB; ++w) {
        const int prow = frow(pixw[w] < 0 ? 0 : pixw[w]);
        const int r0 = rowidx[w];
        float sacc = acc[w];
#pragma unroll
        for (int k = 0; k < PK; ++k) sacc = dot16<T>(s_rows[lc::swzr(prow, k)], s_rows[lc::swzr(r0, k)], sacc);
        acc[w] = sacc;
      }
      __syncthreads();
    }
#pragma unroll
    for (int w = 0; w < UB; ++w)
      if (qw[w] < Q && pixw[w] >= 0) s_D[pixw[w] * (Q + 1) + qw[w]] = acc[w] * p.scale;
  }
  __syncthreads();
  blend_store<T, R, TP, TW>(tid, out, p.out_nhwc, p.out_pitch, b, ty0, tx0, H, W, s_D, s_ax, s_ay);
}

template <typename T, int R>
int launch_lc_mfma(LCParams p, hipStream_t stream) {
  using M = LCM<R>;
  p.tiles_x = (p.W + M::TW - 1) / M::TW;
  p.tiles_y = (p.H + M::TH - 1) / M::TH;
  constexpr int smem = M::Lds::BYTES;
  static std::atomic<uint64_t> attr_done{0};
  if (int rc = ensure_dyn_smem(reinterpret_cast<const void*>(local_corr_mfma_kernel<T, R>), smem, attr_done, "roma_local_corr")) return rc;
  const int grid = p.B * p.tiles_x * p.tiles_y;
  hipLaunchKernelGGL((local_corr_mfma_kernel<T, R>), dim3(grid), dim3(kThreads), smem, stream, p);
  ROMA_CHECK_LAUNCH();
}

template <typename T, int R>
int launch_lc(LCParams p, hipStream_t stream) {
  using G = LCGeom<R>;
  constexpr int CC = G::CHUNK_B / (int)sizeof(T);               // channels per LDS row
  p.tiles_x = (p.W + G::TW - 1) / G::TW;
  p.tiles_y = (p.H + G::TH - 1) / G::TH;
  const int grid = p.B * p.tiles_x * p.tiles_y;
  hipLaunchKernelGGL((local_corr_kernel<T, R, CC>), dim3(grid), dim3(kThreads), G::BYTES, stream, p);
  ROMA_CHECK_LAUNCH();
}

template <typename T, int R>
int launch_any(const LCParams& p, int variant, hipStream_t s) {
  constexpr int CC = 4 * ElemTraits<T>::kPer16B;                // the fast paths stream whole 64-byte channel chunks
  if (!(p.in_nhwc && p.C % CC == 0)) return launch_lc<T, R>(p, s);
  if constexpr (sizeof(T) == 2) {
    // Kernels for this case; `variant` (roma_hip.h) picks one, AUTO:
    //   row streaming (local_corr_rows.hip, 8x8 tiles, C = 256 / 512; r <= 3, or r = 7 on maps up to 47 wide): whole 512-byte
    //     pixel rows through an LDS ring, f0 in registers — AUTO wherever it applies (coherent flow, the regime of a trained matcher:
    //     26.6 vs 20.9 % of 8 TB/s at one pair per launch, 42.4 vs 35.2 % at 16 pairs; on fully incoherent flow its r <= 3 patch path
    //     runs at 3 workgroups per CU, ~20 % behind the 8x4-tile kernel's: gpurun_out/r3_lcb5*.txt);
    //   8x4 tiles, 32-channel chunks (below): 4-5 workgroups per CU hide the per-tile fixed latencies;
    //   8x8 tiles, 32-channel chunks (local_corr_t8.hip, r <= 3): half the fixed cost per pixel, register epilogue.
    const int nt8 = p.B * ((p.H + 7) / 8) * ((p.W + 7) / 8);
    // the tile kernels address one feature map with 32-bit byte offsets
    const bool t8_ok = R <= 3 && p.C % 32 == 0 && (size_t)p.H * p.W * (size_t)(p.f0_pitch > p.f1_pitch ? p.f0_pitch : p.f1_pitch) * 2 < (1ull << 32);
    const bool rows_ok = local_corr_rows_supports(p.C, R, p.H, p.W) && nt8 < (1 << 21) &&
                         (size_t)p.H * p.W * (size_t)(p.f0_pitch > p.f1_pitch ? p.f0_pitch : p.f1_pitch) * 2 < (1ull << 32);
    int v = variant;
    if (v == ROMA_LC_AUTO) v = rows_ok ? ROMA_LC_ROWS8 : (t8_ok && nt8 >= 2048) ? ROMA_LC_TILE8X8 : ROMA_LC_TILE8X4;
    if (v == ROMA_LC_ROWS8 && !rows_ok) v = ROMA_LC_TILE8X8;
    if (v == ROMA_LC_TILE8X8 && !t8_ok) v = ROMA_LC_TILE8X4;
    if (v != ROMA_LC_TILE8X4) {
      LCTileParams q{};
      q.f0 = p.f0; q.f1 = p.f1; q.flow = p.flow; q.out = p.out;
      q.B = p.B; q.C = p.C; q.H = p.H; q.W = p.W;
      q.f0_pitch = p.f0_pitch; q.f1_pitch = p.f1_pitch; q.out_pitch = p.out_pitch;
      q.out_nhwc = p.out_nhwc; q.f1_shift = p.f1_shift; q.scale = p.scale;
      const int dt = std::is_same<T, half_t>::value ? ROMA_F16 : ROMA_BF16;
      if (v == ROMA_LC_TILE8X8) return local_corr_t8(q, R, dt, s);
      return local_corr_rows(q, R, dt, s);
    }
    return launch_lc_mfma<T, R>(p, s);
  } else {
    return launch_lc_nhwc<T, R>(p, s);
  }
}

template <typename T>
int dispatch_r(const LCParams& p, int r, int variant, hipStream_t s) {
  switch (r) {
    case 1: return launch_any<T, 1>(p, variant, s);
    case 2: return launch_any<T, 2>(p, variant, s);
    case 3: return launch_any<T, 3>(p, variant, s);
    case 4: return launch_any<T, 4>(p, variant, s);
    case 5: return launch_any<T, 5>(p, variant, s);
    case 6: return launch_any<T, 6>(p, variant, s);
    case 7: return launch_any<T, 7>(p, variant, s);
  }
  set_error("roma_local_corr: radius %d outside 1..7", r);
  return ROMA_E_UNSUPPORTED;
}

}  // namespace
}  // namespace roma

extern "C" int roma_local_corr(const void* f0, const void* f1, const float* flow, void* out, int B, int C, int H, int W,
                               int r, int dtype, int layout, int f0_pitch, int f1_pitch, int out_layout, int out_pitch,
                               int f1_batch_shift, int variant, void* stream) {
  using namespace roma;
  ROMA_REQUIRE(f0 && f1 && out, ROMA_E_ARG, "roma_local_corr: null pointer");
  ROMA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, ROMA_E_SHAPE, "roma_local_corr: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  ROMA_REQUIRE(r >= 1 && r <= 7, ROMA_E_UNSUPPORTED, "roma_local_corr: radius %d outside 1..7", r);
  ROMA_REQUIRE(f1_batch_shift >= 0 && f1_batch_shift < B, ROMA_E_ARG, "roma_local_corr: f1_batch_shift %d outside [0, B)", f1_batch_shift);
  ROMA_REQUIRE(variant >= ROMA_LC_AUTO && variant <= ROMA_LC_ROWS8, ROMA_E_ARG, "roma_local_corr: unknown kernel variant %d", variant);
  ROMA_REQUIRE(layout == ROMA_NCHW || layout == ROMA_NHWC, ROMA_E_ARG, "roma_local_corr: bad layout %d", layout);
  ROMA_REQUIRE(out_layout == ROMA_NCHW || out_layout == ROMA_NHWC, ROMA_E_ARG, "roma_local_corr: bad out_layout %d", out_layout);
  const int K = (2 * r + 1) * (2 * r + 1);
  ROMA_REQUIRE(f0_pitch >= C && f1_pitch >= C && out_pitch >= K, ROMA_E_SHAPE, "roma_local_corr: pitch smaller than channel count");
  const int esz = dtype == ROMA_F32 ? 4 : 2;
  if (layout == ROMA_NHWC) {
    const int e16 = 16 / esz;
    ROMA_REQUIRE(C % e16 == 0 && f0_pitch % e16 == 0 && f1_pitch % e16 == 0 && aligned16(f0) && aligned16(f1), ROMA_E_ALIGN,
                 "roma_local_corr: channels-last inputs need C and pitches multiples of %d and 16-byte aligned bases", e16);
  }
  ROMA_REQUIRE((size_t)B * H * W * (size_t)(f0_pitch > out_pitch ? f0_pitch : out_pitch) < (1ull << 40), ROMA_E_SHAPE, "roma_local_corr: tensor too large");
  LCParams p{};
  p.f0 = f0; p.f1 = f1; p.flow = flow; p.out = out;
  p.B = B; p.C = C; p.H = H; p.W = W;
  p.f0_pitch = f0_pitch; p.f1_pitch = f1_pitch; p.out_pitch = out_pitch;
  p.in_nhwc = layout == ROMA_NHWC; p.out_nhwc = out_layout == ROMA_NHWC;
  p.scale = 1.0f / sqrtf((float)C);
  p.f1_shift = f1_batch_shift;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case ROMA_F32: return dispatch_r<float>(p, r, variant, s);
    case ROMA_F16: return dispatch_r<half_t>(p, r, variant, s);
    case ROMA_BF16: return dispatch_r<bf16_t>(p, r, variant, s);
  }
  set_error("roma_local_corr: unknown dtype %d", dtype);
  return ROMA_E_DTYPE;
}
