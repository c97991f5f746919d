// The host half of the JPEG stage (roma_amd/csrc/jpeg_host.cpp) alone, under ASan + UBSan: `make -C roma_amd/csrc jpeg_host_check`, then
//   roma_amd/csrc/jpeg_host_check [--mutations N] FILE.jpg ...
// A CPU program: it links jpeg_host.cpp and error.cpp and nothing else, and is neither a test nor loaded into Python.  Per file it
// decodes the stream, then a seeded sweep of N mutations (default 20 000; 1-3 bytes behind the first SOF segment overwritten), then
// the crafted streams that can be derived from it (a duplicated SOF claiming 1024 x 1024 before the first AC scan of a progressive
// stream; table selectors above 3 and a DHT with one value too many in a sequential one); the DHT whose 255 one-bit codes are no prefix
// code needs no file.  The coefficient array is allocated at exactly the size roma_jpeg_info announces, so that a write behind it is the
// sanitizer's to report.  One summary line per file; exit status 1 on a return code other than 0, ROMA_E_ARG, ROMA_E_UNSUPPORTED.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/roma_hip.h"

typedef std::vector<uint8_t> Bytes;

static int g_bad = 0;

struct Codes { int info, dec; };

// both host calls; `nblocks` < 0: size the array from this stream's own info (and skip the second call if there is none)
static Codes decode(const Bytes& d, long nblocks = -1) {
  int info[8] = {0};
  Codes rc{roma_jpeg_info(d.data(), (long)d.size(), info), 0};
  if (nblocks < 0) nblocks = rc.info == 0 ? (long)info[4] * info[5] + 2L * info[6] * info[7] : 0;
  if (nblocks > 0) {
    std::vector<int16_t> coef((size_t)nblocks * 64);
    uint16_t qt[3 * 64];
    rc.dec = roma_jpeg_entropy_decode(d.data(), (long)d.size(), coef.data(), qt);
  }
  for (int r : {rc.info, rc.dec})
    if (r != 0 && r != ROMA_E_ARG && r != ROMA_E_UNSUPPORTED) { ++g_bad; fprintf(stderr, "return code %d (%s)\n", r, roma_last_error()); }
  return rc;
}

struct Segment { int marker; size_t at, end; };

// the marker segments up to EOI, stepping over the entropy-coded data
static std::vector<Segment> segments(const Bytes& d) {
  std::vector<Segment> out;
  size_t i = 2;
  while (i + 4 <= d.size() && !(d[i] == 0xFF && d[i + 1] == 0xD9)) {
    const int m = d[i + 1];
    if (d[i] != 0xFF || m == 0 || m == 0xFF || (m >= 0xD0 && m <= 0xD7)) { ++i; continue; }
    const size_t end = i + 2 + ((size_t)d[i + 2] << 8 | d[i + 3]);
    if (end > d.size()) break;
    out.push_back({m, i, end});
    i = end;
  }
  return out;
}

static uint64_t g_rng;
static uint32_t rnd() {                                            // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static const char* name_of(int rc) { return rc == 0 ? "0" : rc == ROMA_E_ARG ? "E_ARG" : rc == ROMA_E_UNSUPPORTED ? "E_UNSUPPORTED" : "OTHER"; }

int main(int argc, char** argv) {
  long mutations = 20000;
  std::vector<std::string> files;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--mutations") && a + 1 < argc) mutations = atol(argv[++a]);
    else files.push_back(argv[a]);
  }
  Bytes dht = {0xFF, 0xD8, 0xFF, 0xC4, 0x01, 0x12, 0x00, 255};      // SOI, DHT of 2 + 17 + 255 bytes: table 0, 255 codes of one bit
  dht.resize(dht.size() + 15, 0);
  for (int v = 0; v < 255; ++v) dht.push_back((uint8_t)v);
  printf("DHT with 255 one-bit codes: info %s\n", name_of(decode(dht).info));
  for (const std::string& f : files) {
    FILE* fh = fopen(f.c_str(), "rb");
    if (!fh) { fprintf(stderr, "%s: cannot open\n", f.c_str()); return 2; }
    Bytes d;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof(chunk), fh)) > 0;) d.insert(d.end(), chunk, chunk + got);
    fclose(fh);
    int info[8] = {0};
    const Codes whole = decode(d);
    roma_jpeg_info(d.data(), (long)d.size(), info);
    const long nblocks = (long)info[4] * info[5] + 2L * info[6] * info[7];
    const std::vector<Segment> segs = segments(d);
    size_t sof = 0, sos = 0, ac_sos = 0, dht_at = 0;
    for (const Segment& s : segs) {
      if (s.marker >= 0xC0 && s.marker <= 0xC2 && !sof) sof = s.at;
      if (s.marker == 0xC4 && !dht_at) dht_at = s.at;
      if (s.marker == 0xDA && !sos) sos = s.at;
      if (s.marker == 0xDA && !ac_sos && d[s.end - 3] > 0) ac_sos = s.at;
    }
    if (whole.info != 0 || whole.dec != 0 || !sof) { printf("%s: info %s, decode %s: not swept\n", f.c_str(), name_of(whole.info), name_of(whole.dec)); continue; }
    // the sweep: the frame, and with it the array, stays what the intact stream announced
    const size_t first = sof + 2 + ((size_t)d[sof + 2] << 8 | d[sof + 3]);
    long n_ok = 0, n_arg = 0, n_uns = 0;
    g_rng = 0x6A7065675F686F73ull;
    for (long m = 0; m < mutations; ++m) {
      Bytes x = d;
      for (int k = 1 + (int)(rnd() % 3); k > 0; --k) x[first + rnd() % (x.size() - first)] = (uint8_t)rnd();
      const Codes rc = decode(x, nblocks);
      const int worst = rc.info ? rc.info : rc.dec;
      ++(worst == 0 ? n_ok : worst == ROMA_E_ARG ? n_arg : n_uns);
    }
    // the crafted streams
    std::string crafted;
    auto crafted_rc = [&](const char* what, const Bytes& x) {
      const Codes rc = decode(x);
      crafted += std::string("; ") + what + ": " + (rc.info ? "info " : "decode ") + name_of(rc.info ? rc.info : rc.dec);
    };
    if (ac_sos) {
      Bytes copy(d.begin() + sof, d.begin() + first), x = d;
      copy[5] = copy[7] = 0x04;                                    // height, width = 1024
      copy[6] = copy[8] = 0x00;
      x.insert(x.begin() + ac_sos, copy.begin(), copy.end());
      crafted_rc("second SOF", x);
    } else {
      Bytes x = d;
      x[sos + 6] = 0x70;                                           // FF DA, length, Ns, component id, selectors
      crafted_rc("DC selector 7", x);
      x[sos + 6] = 0x07;
      crafted_rc("AC selector 7", x);
    }
    if (dht_at) {
      Bytes x = d;
      const size_t L = ((size_t)x[dht_at + 2] << 8 | x[dht_at + 3]) + 1;
      x[dht_at + 2] = (uint8_t)(L >> 8);
      x[dht_at + 3] = (uint8_t)L;
      x.insert(x.begin() + dht_at + 2 + L - 1, 0);
      crafted_rc("DHT with one value too many", x);
    }
    printf("%s: %d x %d, %ld blocks, decode 0; %ld mutations: %ld x 0, %ld x E_ARG, %ld x E_UNSUPPORTED%s\n", f.c_str(), info[0], info[1], nblocks,
           mutations, n_ok, n_arg, n_uns, crafted.c_str());
  }
  printf("%s\n", g_bad ? "FAILED: a return code outside {0, ROMA_E_ARG, ROMA_E_UNSUPPORTED}" : "all return codes in {0, ROMA_E_ARG, ROMA_E_UNSUPPORTED}");
  return g_bad ? 1 : 0;
}
