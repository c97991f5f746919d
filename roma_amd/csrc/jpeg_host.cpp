// Host half of JPEG decoding (jpeg.hip holds the device half): the marker parser and the serial Huffman decoder behind roma_jpeg_info and
// roma_jpeg_entropy_decode.  Plain C++17 without a HIP header, so that it also builds on its own: it is the one place where the library
// reads bytes it did not produce, and tools/jpeg_host_check.cpp runs it under ASan + UBSan (`make jpeg_host_check`).
// What is decoded and what is refused as ROMA_E_UNSUPPORTED: include/roma_hip.h.  What bounds the writes, whatever the bytes say: a DHT
// must be a prefix code, the one SOF a stream may carry fixes the frame's geometry, a scan's table selectors are 0..3, and every block
// address is checked against its component's grid (each of them ROMA_E_ARG).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include "error.h"

namespace roma {
namespace {

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  // canonical code tables: for code length l (1..16): the first code value, the first symbol index, the number of codes
  int mincode[17], valptr[17], maxcode[18];
  uint8_t vals[256];
  uint16_t look[512];                                            // 9-bit fast path: (length << 8) | symbol, 0 = longer code
  bool present = false;
};

struct Comp { int id, h, v, tq, td, ta; };

struct Header {
  int width = 0, height = 0, ncomp = 0;
  Comp comp[3];
  uint16_t qt[4][64];                                            // natural order
  bool qt_present[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int restart = 0;
  size_t scan = 0;                                               // offset of the entropy-coded data, 0 = no SOS yet
  int hmax = 1, vmax = 1;
  bool adobe_rgb = false, jfif = false;
  bool progressive = false, sof = false;
  // the scan the last SOS announced: its components (indices into comp), spectral band, successive-approximation bits
  int sc_ns = 0, sc_ci[3] = {0, 0, 0}, Ss = 0, Se = 63, Ah = 0, Al = 0;
};

// false: the counts are no prefix code (more codes of some length than that length has left), which would index past look / vals
bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    h.valptr[l] = k;
    h.mincode[l] = code;
    code += counts[l - 1];
    k += counts[l - 1];
    if (code > (1 << l)) return false;
    h.maxcode[l] = counts[l - 1] ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  memcpy(h.vals, vals, (size_t)nvals);
  memset(h.look, 0, sizeof(h.look));
  code = 0;
  k = 0;
  for (int l = 1; l <= 9; ++l) {
    for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
      const int lo = code << (9 - l);
      for (int j = 0; j < (1 << (9 - l)); ++j) h.look[lo + j] = (uint16_t)((l << 8) | vals[k]);
    }
    code <<= 1;
  }
  h.present = true;
  return true;
}

// parse the marker segments from byte `i` (2: right behind SOI) up to and including the next SOS: 0 (H.scan = the entropy-coded data, the
// scan's parameters in H), 1 = end of image behind at least one scan, or a negative roma error code
int parse(const uint8_t* d, size_t n, Header& H, size_t i = 2) {
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) { set_error("roma_jpeg: not a JPEG stream (no SOI)"); return ROMA_E_ARG; }
  while (i + 2 <= n) {
    const bool eoi = d[i] == 0xFF && d[i + 1] == 0xD9;           // before the first scan it ends no image: "no start of scan"
    if (eoi && H.scan) return 1;
    if (eoi || i + 4 > n) break;
    if (d[i] != 0xFF) { set_error("roma_jpeg: marker expected at byte %zu", i); return ROMA_E_ARG; }
    const int m = d[i + 1];
    if (m == 0xFF) { ++i; continue; }                            // fill byte
    const size_t L = ((size_t)d[i + 2] << 8) | d[i + 3];
    if (L < 2 || i + 2 + L > n) { set_error("roma_jpeg: truncated segment at byte %zu", i); return ROMA_E_ARG; }
    const uint8_t* s = d + i + 4;
    const size_t sl = L - 2;
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {                   // baseline / extended sequential / progressive, Huffman
      // the one SOF fixes the geometry every later scan is walked by (and the caller's buffer was sized from)
      if (H.sof) { set_error("roma_jpeg: a second SOF"); return ROMA_E_ARG; }
      H.progressive = m == 0xC2;
      if (sl < 6 || s[0] != 8) { set_error("roma_jpeg: %d-bit samples", sl ? s[0] : 0); return ROMA_E_UNSUPPORTED; }
      H.height = (s[1] << 8) | s[2];
      H.width = (s[3] << 8) | s[4];
      H.ncomp = s[5];
      if ((H.ncomp != 1 && H.ncomp != 3) || sl < 6 + 3 * (size_t)H.ncomp || H.width == 0 || H.height == 0) {
        set_error("roma_jpeg: %d components, %d x %d", H.ncomp, H.width, H.height);
        return ROMA_E_UNSUPPORTED;
      }
      for (int c = 0; c < H.ncomp; ++c) {
        H.comp[c] = Comp{s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c] & 3, 0, 0};
        H.hmax = std::max(H.hmax, H.comp[c].h);
        H.vmax = std::max(H.vmax, H.comp[c].v);
      }
      H.sof = true;
    } else if (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      set_error("roma_jpeg: SOF%d (lossless / arithmetic / hierarchical) is not decoded here", m - 0xC0);
      return ROMA_E_UNSUPPORTED;
    } else if (m == 0xDB) {                                      // quantisation tables (zig-zag order in the file)
      size_t o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (tq > 3 || o + 1 + (pq ? 128 : 64) > sl) { set_error("roma_jpeg: bad DQT"); return ROMA_E_ARG; }
        for (int k = 0; k < 64; ++k) H.qt[tq][kZigzag[k]] = pq ? (uint16_t)((s[o + 1 + 2 * k] << 8) | s[o + 2 + 2 * k]) : s[o + 1 + k];
        H.qt_present[tq] = true;
        o += 1 + (pq ? 128 : 64);
      }
    } else if (m == 0xC4) {                                      // Huffman tables: the segment is tables of 17 + (sum of the counts) bytes, no more
      size_t o = 0;
      while (o + 17 <= sl) {
        const int tc = s[o] >> 4, th = s[o] & 15;
        int nv = 0;
        for (int k = 0; k < 16; ++k) nv += s[o + 1 + k];
        if (tc > 1 || th > 3 || nv > 256 || o + 17 + nv > sl || !build_huff(tc ? H.ac[th] : H.dc[th], s + o + 1, s + o + 17, nv)) break;
        o += 17 + nv;
      }
      if (o != sl) { set_error("roma_jpeg: bad DHT"); return ROMA_E_ARG; }
    } else if (m == 0xEE) {                                      // APP14 "Adobe": transform 0 with three components = stored as RGB, not YCbCr
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] == 0) H.adobe_rgb = true;
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF", 4) == 0) H.jfif = true;
    } else if (m == 0xDD) {
      if (sl >= 2) H.restart = (s[0] << 8) | s[1];
    } else if (m == 0xDA) {                                      // start of scan
      if (!H.sof) { set_error("roma_jpeg: SOS before SOF"); return ROMA_E_ARG; }
      const int ns = sl ? s[0] : 0;
      if (ns < 1 || ns > H.ncomp || sl < 1 + 2 * (size_t)ns + 3) { set_error("roma_jpeg: bad SOS"); return ROMA_E_ARG; }
      if (!H.progressive && ns != H.ncomp) {
        set_error("roma_jpeg: a scan with %d of %d components (non-interleaved sequential scans are not decoded here)", ns, H.ncomp);
        return ROMA_E_UNSUPPORTED;
      }
      H.sc_ns = ns;
      for (int c = 0; c < ns; ++c) {
        int ci = -1;
        for (int k = 0; k < H.ncomp; ++k)
          if (H.comp[k].id == s[1 + 2 * c]) ci = k;
        if (ci < 0 || (c > 0 && ci <= H.sc_ci[c - 1])) { set_error("roma_jpeg: scan component order"); return ROMA_E_UNSUPPORTED; }
        H.sc_ci[c] = ci;
        H.comp[ci].td = s[2 + 2 * c] >> 4;
        H.comp[ci].ta = s[2 + 2 * c] & 15;
        if (H.comp[ci].td > 3 || H.comp[ci].ta > 3) { set_error("roma_jpeg: Huffman table selector above 3"); return ROMA_E_ARG; }
      }
      H.Ss = s[1 + 2 * ns];
      H.Se = s[2 + 2 * ns];
      H.Ah = s[3 + 2 * ns] >> 4;
      H.Al = s[3 + 2 * ns] & 15;
      if (!H.progressive) { H.Ss = 0; H.Se = 63; H.Ah = H.Al = 0; }
      if (H.Ss > H.Se || H.Se > 63 || H.Al > 13 || (H.Ss == 0 && H.Se != 0 && H.progressive) || (H.Ss > 0 && ns != 1)) {
        set_error("roma_jpeg: bad progressive scan parameters");
        return ROMA_E_ARG;
      }
      for (int c = 0; c < ns; ++c) {
        const Comp& cp = H.comp[H.sc_ci[c]];
        const bool need_dc = H.Ss == 0 && H.Ah == 0, need_ac = H.Se > 0;
        if ((need_dc && !H.dc[cp.td].present) || (need_ac && !H.ac[cp.ta].present) || !H.qt_present[cp.tq]) {
          set_error("roma_jpeg: a table the scan refers to is missing");
          return ROMA_E_ARG;
        }
      }
      H.scan = i + 2 + L;
      // colour space: YCbCr is what the kernels convert.  libjpeg takes three components for RGB when an Adobe marker says
      // "transform 0", or — without a JFIF marker — when the component ids spell 'R', 'G', 'B'
      if (H.ncomp == 3 && (H.adobe_rgb || (!H.jfif && H.comp[0].id == 'R' && H.comp[1].id == 'G' && H.comp[2].id == 'B'))) {
        set_error("roma_jpeg: three components stored as RGB (no YCbCr transform) are not decoded here");
        return ROMA_E_UNSUPPORTED;
      }
      // sampling: grey, 4:4:4, 4:2:2 or 4:2:0
      if (H.ncomp == 3) {
        const bool c444 = H.comp[0].h == 1 && H.comp[0].v == 1, c420 = H.comp[0].h == 2 && H.comp[0].v == 2;
        const bool c422 = H.comp[0].h == 2 && H.comp[0].v == 1;
        if (!(c444 || c420 || c422) || H.comp[1].h != 1 || H.comp[1].v != 1 || H.comp[2].h != 1 || H.comp[2].v != 1) {
          set_error("roma_jpeg: chroma sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 are decoded here)", H.comp[0].h, H.comp[0].v, H.comp[1].h,
                    H.comp[1].v, H.comp[2].h, H.comp[2].v);
          return ROMA_E_UNSUPPORTED;
        }
      } else {
        H.comp[0].h = H.comp[0].v = H.hmax = H.vmax = 1;          // a single component is never interleaved: one block per MCU
      }
      return 0;
    }
    i += 2 + L;
  }
  set_error("roma_jpeg: no start of scan");
  return ROMA_E_ARG;
}

// The frame's block grids, taken ONCE from the header the first parse() returns: component c is bw x bh blocks (whole MCUs) in raster
// order at coef + off * 64; a single-component scan walks the ow x oh of them that cover the component's own samples, ceil(width_c / 8) per row
struct Frame {
  int mcux, mcuy, bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0}, ow[3] = {0, 0, 0}, oh[3] = {0, 0, 0};
  size_t off[3] = {0, 0, 0}, total = 0;
  explicit Frame(const Header& H) : mcux((H.width + 8 * H.hmax - 1) / (8 * H.hmax)), mcuy((H.height + 8 * H.vmax - 1) / (8 * H.vmax)) {
    for (int c = 0; c < H.ncomp; ++c) {
      bw[c] = mcux * H.comp[c].h;
      bh[c] = mcuy * H.comp[c].v;
      ow[c] = ((H.width * H.comp[c].h + H.hmax - 1) / H.hmax + 7) / 8;
      oh[c] = ((H.height * H.comp[c].v + H.vmax - 1) / H.vmax + 7) / 8;
      off[c] = total;
      total += (size_t)bw[c] * bh[c];
    }
  }
};

struct Bits {
  const uint8_t* d;
  size_t n, pos;
  uint64_t acc = 0;
  int cnt = 0;
  bool hit_marker = false;
  void fill() {
    if (cnt > 32) return;
    // fast path: four stream bytes none of which is 0xFF (no stuffing, no marker) go in at once
    if (!hit_marker && pos + 4 <= n) {
      const uint32_t w = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      if (!((w & ~(w + 0x01010101u) & 0x80808080u))) {           // no byte equals 0xFF (0xFF + 1 carries out of its byte)
        acc |= (uint64_t)w << (32 - cnt);
        cnt += 32;
        pos += 4;
        return;
      }
    }
    while (cnt <= 48) {
      int b = 0;
      if (!hit_marker && pos < n) {
        b = d[pos];
        if (b == 0xFF) {
          if (pos + 1 < n && d[pos + 1] == 0) pos += 2;           // stuffed zero
          else { hit_marker = true; b = 0; }                      // a marker: feed zeros from here (like libjpeg's "insert zeros")
        } else {
          ++pos;
        }
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  int peek(int k) { return (int)(acc >> (64 - k)); }
  void skip(int k) { acc <<= k; cnt -= k; }
  int get(int k) {
    if (k == 0) return 0;
    const int v = peek(k);
    skip(k);
    return v;
  }
  void reset() { acc = 0; cnt = 0; hit_marker = false; }
};

inline int decode_sym(Bits& b, const Huff& h) {
  b.fill();
  const int look = h.look[b.peek(9)];
  if (look) { b.skip(look >> 8); return look & 255; }
  int code = b.peek(10), l = 10;
  while (l <= 16 && code > h.maxcode[l]) { ++l; code = b.peek(l); }
  if (l > 16) return -1;
  b.skip(l);
  return h.vals[h.valptr[l] + code - h.mincode[l]];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// What the blocks of one scan share.  The four block decoders below are those of ITU T.81 Annex F.2.2 (sequential) and G.1.2 (progressive)
struct Scan {
  Bits b;
  const int Ss, Se, p1;                                          // the spectral band, and 1 << Al: the weight of the bit plane this scan delivers
  const bool runs;                                               // end-of-band runs exist (a progressive stream)
  int pred[3] = {0, 0, 0}, eobrun = 0;
};

inline int dc_first(Scan& s, const Huff& h, int c, int16_t* blk) {
  const int sz = decode_sym(s.b, h);
  if (sz < 0 || sz > 15) { set_error("roma_jpeg: corrupt DC code"); return ROMA_E_ARG; }
  s.b.fill();
  if (sz) s.pred[c] += extend(s.b.get(sz), sz);
  blk[0] = (int16_t)(s.pred[c] * s.p1);
  return 0;
}

// one more bit of a coefficient; for AC only where it is already non-zero
inline void dc_refine(Scan& s, int16_t* blk) {
  s.b.fill();
  if (s.b.get(1)) blk[0] |= (int16_t)s.p1;
}
inline void ac_refine_bit(Scan& s, int16_t* cf) {
  s.b.fill();
  if (s.b.get(1) && (*cf & s.p1) == 0) *cf = (int16_t)(*cf + (*cf >= 0 ? s.p1 : -s.p1));
}

// AC first pass over the band [k, Se].  With runs, a (run < 15, size 0) symbol ends the band for 2^run + (run bits) blocks, this one
// included; without (a sequential block: the band 1..63 at Al = 0) it ends this block and no run bits are read
inline int ac_first(Scan& s, const Huff& h, int k, int16_t* blk) {
  if (s.eobrun > 0) { --s.eobrun; return 0; }
  while (k <= s.Se) {
    const int rs = decode_sym(s.b, h);
    if (rs < 0) { set_error("roma_jpeg: corrupt AC code"); return ROMA_E_ARG; }
    const int r = rs >> 4, sz = rs & 15;
    if (sz == 0) {
      if (r == 15) { k += 16; continue; }
      if (s.runs) {
        s.eobrun = (1 << r) - 1;
        if (r) { s.b.fill(); s.eobrun += s.b.get(r); }
      }
      break;
    }
    k += r;
    if (k > s.Se) { set_error("roma_jpeg: AC run past the %s", s.runs ? "band" : "block"); return ROMA_E_ARG; }
    s.b.fill();
    blk[kZigzag[k]] = (int16_t)(extend(s.b.get(sz), sz) * s.p1);
    ++k;
  }
  return 0;
}

// AC refinement: one correction bit for every coefficient that is already non-zero, new +-2^Al coefficients placed after `r` still-zero
// positions (the decoder of Annex G.1.2.3)
inline int ac_refine(Scan& s, const Huff& h, int k, int16_t* blk) {
  if (s.eobrun == 0) {
    for (; k <= s.Se; ++k) {
      const int rs = decode_sym(s.b, h);
      if (rs < 0) { set_error("roma_jpeg: corrupt AC code"); return ROMA_E_ARG; }
      int r = rs >> 4, val = rs & 15;
      if (val) {
        s.b.fill();
        val = s.b.get(1) ? s.p1 : -s.p1;
      } else if (r != 15) {
        s.eobrun = 1 << r;
        if (r) { s.b.fill(); s.eobrun += s.b.get(r); }
        break;
      }
      do {
        int16_t* cf = blk + kZigzag[k];
        if (*cf != 0) ac_refine_bit(s, cf);
        else if (--r < 0) break;
        ++k;
      } while (k <= s.Se);
      if (val && k <= s.Se) blk[kZigzag[k]] = (int16_t)val;
    }
  }
  if (s.eobrun > 0) {
    for (; k <= s.Se; ++k)
      if (blk[kZigzag[k]] != 0) ac_refine_bit(s, blk + kZigzag[k]);
    --s.eobrun;
  }
  return 0;
}

// Walk the scan H announces and add what it carries to the coefficient array: a spectral band and / or one more bit of precision (Annex
// G), or, for a sequential stream, everything: DC first pass, then AC first pass over 1..63.  The units are MCUs for an interleaved scan
// and the component's own blocks for a single-component one.  *end = where the entropy-coded data was left
int decode_scan(const uint8_t* d, size_t n, const Header& H, const Frame& F, int16_t* coef, size_t* end) {
  Scan s{Bits{d, n, H.scan}, H.Ss, H.Se, 1 << H.Al, H.progressive};
  const bool own = H.sc_ns == 1;
  const int nux = own ? F.ow[H.sc_ci[0]] : F.mcux, nuy = own ? F.oh[H.sc_ci[0]] : F.mcuy;
  int togo = H.restart;
  for (int uy = 0; uy < nuy; ++uy)
    for (int ux = 0; ux < nux; ++ux) {
      if (H.restart && togo-- == 0) {                            // restart interval: byte-align behind the next RSTn, start over
        size_t q = s.b.pos;
        while (q + 1 < n && !(d[q] == 0xFF && d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7)) ++q;
        if (q + 1 >= n) { set_error("roma_jpeg: restart marker missing"); return ROMA_E_ARG; }
        s.b.pos = q + 2;
        s.b.reset();
        s.pred[0] = s.pred[1] = s.pred[2] = s.eobrun = 0;
        togo = H.restart - 1;
      }
      for (int sc = 0; sc < H.sc_ns; ++sc) {
        const int c = H.sc_ci[sc];
        const Comp& cp = H.comp[c];
        const int nh = own ? 1 : cp.h, nv = own ? 1 : cp.v;
        for (int v = 0; v < nv; ++v)
          for (int h = 0; h < nh; ++h) {
            const int by = uy * nv + v, bx = ux * nh + h;
            if (by >= F.bh[c] || bx >= F.bw[c]) { set_error("roma_jpeg: a block outside its component's grid"); return ROMA_E_ARG; }
            int16_t* blk = coef + (F.off[c] + (size_t)by * F.bw[c] + bx) * 64;
            int rc = 0;
            if (s.Ss == 0) {
              if (H.Ah == 0) rc = dc_first(s, H.dc[cp.td], c, blk);
              else dc_refine(s, blk);
            }
            const Huff& ha = H.ac[cp.ta];                        // a band that starts at 0 (a sequential scan) has had its DC above
            if (rc == 0 && s.Se > 0) rc = H.Ah == 0 ? ac_first(s, ha, std::max(s.Ss, 1), blk) : ac_refine(s, ha, std::max(s.Ss, 1), blk);
            if (rc) return rc;
          }
      }
    }
  *end = s.b.pos;
  return 0;
}

}  // namespace
}  // namespace roma

using namespace roma;

// info[0..7] = width, height, components, chroma subsampling (0: 4:4:4, 1: 4:2:0, 2: 4:2:2, -1: grey), luma blocks per row, luma block rows, chroma
// blocks per row, chroma block rows.  HOST function.
extern "C" int roma_jpeg_info(const void* data, long nbytes, int* info) {
  ROMA_REQUIRE(data && info && nbytes > 0, ROMA_E_ARG, "roma_jpeg_info: null pointer");
  Header H;
  if (int rc = parse(static_cast<const uint8_t*>(data), (size_t)nbytes, H)) return rc;
  const Frame F(H);
  info[0] = H.width; info[1] = H.height; info[2] = H.ncomp;
  info[3] = H.ncomp == 1 ? -1 : (H.hmax == 2 ? (H.vmax == 2 ? 1 : 2) : 0);
  info[4] = F.bw[0]; info[5] = F.bh[0];
  info[6] = H.ncomp == 1 ? 0 : F.bw[1]; info[7] = H.ncomp == 1 ? 0 : F.bh[1];
  return 0;
}

// Huffman-decode the scans: coef = the quantised coefficients, int16, natural (row-major) order inside a block, the blocks of component c
// in raster order at coef + off_c * 64 (off_0 = 0, off_1 = luma blocks, off_2 = luma + chroma blocks); qt = 3 x 64 uint16 de-quantisation
// tables in natural order (the component's own table at row c).  HOST function: all pointers in host memory.
extern "C" int roma_jpeg_entropy_decode(const void* data, long nbytes, int16_t* coef, uint16_t* qt) {
  ROMA_REQUIRE(data && coef && qt && nbytes > 0, ROMA_E_ARG, "roma_jpeg_entropy_decode: null pointer");
  const uint8_t* d = static_cast<const uint8_t*>(data);
  const size_t n = (size_t)nbytes;
  Header H;
  if (int rc = parse(d, n, H)) return rc;
  const Frame F(H);
  memset(coef, 0, F.total * 64 * sizeof(int16_t));
  // a sequential stream is its one scan; a progressive one goes on with the next marker segment: further tables and scans, or the end of the image
  for (int nscan = 0; nscan < 1000; ++nscan) {
    size_t q;
    if (int rc = decode_scan(d, n, H, F, coef, &q)) return rc;
    if (!H.progressive) break;
    while (q + 1 < n && !(d[q] == 0xFF && d[q + 1] != 0 && !(d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7) && d[q + 1] != 0xFF)) ++q;
    if (q + 1 >= n) break;                                       // no EOI: what has been decoded stands (libjpeg warns and does the same)
    const int rc = parse(d, n, H, q);
    if (rc == 1) break;
    if (rc < 0) return rc;
  }
  for (int c = 0; c < H.ncomp; ++c) memcpy(qt + 64 * c, H.qt[H.comp[c].tq], 128);   // as they stand at the end: a progressive stream may define them between its scans
  return 0;
}
