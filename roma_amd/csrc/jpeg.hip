// Device half of JPEG decoding for RegressionMatcher.match() on file paths — reference: romatch/models/matcher.py:606-637, 667-676
// (`Image.open(path).convert("RGB")`, i.e. PIL -> libjpeg(-turbo) with its defaults: JDCT_ISLOW, fancy up-sampling).
// SURVEY §8(f) rank 3 asks for the pre-processing on the device.  The entropy-coded segment is a serial bit stream, so the split is
// the usual one: Huffman decoding on the host (jpeg_host.cpp: roma_jpeg_info, roma_jpeg_entropy_decode), everything after it on the GPU
// (roma_jpeg_reconstruct): de-quantisation + the 8x8 inverse DCT, chroma up-sampling, YCbCr -> RGB, one uint8 (H, W, 3) image in HBM
// that roma_resample_u8 / roma_normalize_u8 consume — the decoded photograph never crosses PCIe, only its quantised coefficients do.
// The arithmetic is libjpeg's, restated from its published description (the "islow" integer IDCT of Loeffler / Ligtenberg / Moschytz with
// 13-bit constants and a 2-bit first-pass scale; the h2v2 "triangle" up-sampler, 3/4 near + 1/4 far in each direction with its 8 / 7
// rounding biases and replicated edges; the 16-bit fixed-point colour tables), so the result is BIT-IDENTICAL to PIL's
// (tests/test_jpeg.py: the four bundled photographs, one of them 618 pixels wide, and synthetic 4:4:4 / grey / restart-interval streams).
#include "common.h"

namespace roma {
namespace {

// one thread per 8x8 block: de-quantise, inverse DCT (two passes of the 8-point butterfly, 13-bit constants), level shift, clamp
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift, bool first) {
  constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * F0_541;
  const int t2 = z1 + z3 * (-F1_847), t3 = z1 + z2 * F0_765;
  z2 = in[0];
  z3 = in[4];
  const int t0 = (z2 + z3) << 13, t1 = (z2 - z3) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  z1 = o0 + o3;
  z2 = o1 + o2;
  z3 = o0 + o2;
  int z4 = o1 + o3;
  const int z5 = (z3 + z4) * F1_175;
  o0 *= F0_298; o1 *= F2_053; o2 *= F3_072; o3 *= F1_501;
  z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
  z3 += z5;
  z4 += z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const int r = 1 << (shift - 1);
  (void)first;
  out[0] = (t10 + o3 + r) >> shift; out[7] = (t10 - o3 + r) >> shift;
  out[1] = (t11 + o2 + r) >> shift; out[6] = (t11 - o2 + r) >> shift;
  out[2] = (t12 + o1 + r) >> shift; out[5] = (t12 - o1 + r) >> shift;
  out[3] = (t13 + o0 + r) >> shift; out[4] = (t13 - o0 + r) >> shift;
}

__global__ __launch_bounds__(64) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, uint8_t* __restrict__ plane,
                                                       int blocks_w, int nblocks, int pitch) {
  const int bi = blockIdx.x * 64 + threadIdx.x;
  if (bi >= nblocks) return;
  const int16_t* c = coef + (size_t)bi * 64;
  int ws[8][8];
#pragma unroll
  for (int col = 0; col < 8; ++col) {                            // pass 1: columns, results scaled by 2^2
    int in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = (int)c[r * 8 + col] * (int)qt[r * 8 + col];
    idct8(in, out, 13 - 2, true);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r][col] = out[r];
  }
  const int by = bi / blocks_w, bx = bi - by * blocks_w;
  uint8_t* dst = plane + (size_t)by * 8 * pitch + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {                                  // pass 2: rows, remove the 2^2 and the 8 of the 2-D transform, + 128
    int out[8];
    idct8(ws[r], out, 13 + 2 + 3, false);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)min(max(out[k] + 128, 0), 255) << (8 * k);
      hi |= (uint32_t)min(max(out[4 + k] + 128, 0), 255) << (8 * k);
    }
    *reinterpret_cast<uint2*>(dst + (size_t)r * pitch) = uint2{lo, hi};
  }
}

// Y (full resolution) + Cb, Cr (same, or half in both directions: "fancy" triangle up-sampling) -> RGB, one thread per pixel
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cbp, const uint8_t* __restrict__ crp,
                                                       uint8_t* __restrict__ rgb, int W, int H, int ypitch, int cpitch, int cw, int ch, int sub) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const int Y = yp[(size_t)y * ypitch + x];
  int cb, cr;
  if (sub == 0) {
    cb = cbp[(size_t)y * cpitch + x];
    cr = crp[(size_t)y * cpitch + x];
  } else if (sub < 0) {
    cb = cr = 128;
  } else if (cw <= 2) {                                          // libjpeg picks the triangle filter only for more than two chroma columns
    const int yc = sub == 2 ? y : y >> 1;
    cb = cbp[(size_t)yc * cpitch + (x >> 1)];
    cr = crp[(size_t)yc * cpitch + (x >> 1)];
  } else if (sub == 2) {
    // 4:2:2, horizontal triangle filter only: column 2 j = (3 c[j] + c[j - 1] + 1) >> 2, column 2 j + 1 = (3 c[j] + c[j + 1] + 2) >> 2,
    // the first and the last output column are the first / last sample themselves
    const int j = x >> 1;
    const uint8_t *r0 = cbp + (size_t)y * cpitch, *r1 = crp + (size_t)y * cpitch;
    if ((x & 1) == 0) {
      cb = j == 0 ? r0[0] : (3 * r0[j] + r0[j - 1] + 1) >> 2;
      cr = j == 0 ? r1[0] : (3 * r1[j] + r1[j - 1] + 1) >> 2;
    } else {
      cb = j == cw - 1 ? r0[j] : (3 * r0[j] + r0[j + 1] + 2) >> 2;
      cr = j == cw - 1 ? r1[j] : (3 * r1[j] + r1[j + 1] + 2) >> 2;
    }
  } else {
    // output row 2 r + v takes 3/4 of chroma row r and 1/4 of row r - 1 (v = 0) or r + 1 (v = 1), edges replicated; output column
    // 2 j takes 3/4 of column j and 1/4 of column j - 1 with bias 8, column 2 j + 1 takes 1/4 of column j + 1 with bias 7; at the first
    // / last column the missing neighbour is the column itself
    const int r = y >> 1, j = x >> 1;
    const int rf = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
    const int jn = (x & 1) ? min(j + 1, cw - 1) : max(j - 1, 0);
    const int bias = (x & 1) ? 7 : 8;
    const uint8_t *n0 = cbp + (size_t)r * cpitch, *f0 = cbp + (size_t)rf * cpitch, *n1 = crp + (size_t)r * cpitch, *f1 = crp + (size_t)rf * cpitch;
    cb = (3 * (3 * n0[j] + f0[j]) + (3 * n0[jn] + f0[jn]) + bias) >> 4;
    cr = (3 * (3 * n1[j] + f1[j]) + (3 * n1[jn] + f1[jn]) + bias) >> 4;
  }
  int R, G, B;
  if (sub < 0) {
    R = G = B = Y;
  } else {
    // 16-bit fixed point: 1.40200, 1.77200, 0.71414, 0.34414 scaled by 65536 (+0.5), the ONE_HALF of the green sum on the Cb term
    const int xb = cb - 128, xr = cr - 128;
    R = Y + ((91881 * xr + 32768) >> 16);
    B = Y + ((116130 * xb + 32768) >> 16);
    G = Y + ((-22554 * xb + 32768 - 46802 * xr) >> 16);
  }
  uint8_t* o = rgb + ((size_t)y * W + x) * 3;
  o[0] = (uint8_t)min(max(R, 0), 255);
  o[1] = (uint8_t)min(max(G, 0), 255);
  o[2] = (uint8_t)min(max(B, 0), 255);
}

}  // namespace
}  // namespace roma

using namespace roma;


// coef, qt: DEVICE copies of what roma_jpeg_entropy_decode produced; planes: device scratch of (luma blocks + 2 x chroma blocks) x 64
// bytes; rgb: uint8 (height, width, 3).  info as returned by roma_jpeg_info.
extern "C" int roma_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, void* planes, void* rgb, const int* info, void* stream) {
  ROMA_REQUIRE(coef && qt && planes && rgb && info, ROMA_E_ARG, "roma_jpeg_reconstruct: null pointer");
  const int W = info[0], Hh = info[1], nc = info[2], sub = info[3], ybw = info[4], ybh = info[5], cbw = info[6], cbh = info[7];
  ROMA_REQUIRE(W > 0 && Hh > 0 && (nc == 1 || nc == 3) && ybw > 0 && ybh > 0 && ybw * 8 >= W && ybh * 8 >= Hh, ROMA_E_SHAPE, "roma_jpeg_reconstruct: bad info");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* yp = static_cast<uint8_t*>(planes);
  const int ny = ybw * ybh, ncb = cbw * cbh;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((ny + 63) / 64), dim3(64), 0, s, coef, qt, yp, ybw, ny, ybw * 8);
  uint8_t *cbp = yp + (size_t)ny * 64, *crp = cbp + (size_t)ncb * 64;
  if (nc == 3) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((ncb + 63) / 64), dim3(64), 0, s, coef + (size_t)ny * 64, qt + 64, cbp, cbw, ncb, cbw * 8);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((ncb + 63) / 64), dim3(64), 0, s, coef + (size_t)(ny + ncb) * 64, qt + 128, crp, cbw, ncb, cbw * 8);
  }
  const int cw = (W + 1) / 2, ch = (Hh + 1) / 2;                 // libjpeg's down-sampled dimensions: what the up-sampler walks
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((W + 255) / 256, Hh), dim3(256), 0, s, yp, cbp, crp, static_cast<uint8_t*>(rgb), W, Hh, ybw * 8,
                     cbw * 8, cw, ch, sub);
  ROMA_CHECK_LAUNCH();
}
