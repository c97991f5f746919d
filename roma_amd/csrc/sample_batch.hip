// Batched sampling for P pairs at once (RegressionMatcher.sample_batch): the two selections of sample() as a radix select with a
// total order, and the KDE over P point sets in one launch with the gather fused into the load.
//
// Selection.  Row p keeps its k best items under (key descending, counter ascending), key = the exponential-race key of
// sample_device.h (bitwise that of roma_race_keys), counter = the value the key hashes (the item's position when no counter is
// given).  Both go into one 64-bit composite whose unsigned order is that order:
//   composite = monotone(key bits) << 32 | (0xFFFFFFFF - counter)
// monotone() is the usual float-to-unsigned map (negative: all bits flipped, else sign bit set), so a key of -inf — u rounds to 1
// for one hash value in 2^24, E = -0 — sorts below 0 as it does for a float comparison.  Counters of one row are distinct, so all
// composites are, and the k-th largest is a unique threshold T: exactly k items have composite >= T.
// T is found most significant digit first, 11 bits per pass (5 x 11 + 9), one launch per pass.  Every workgroup of a pass
// histograms, in LDS, the digit of the items whose resolved high bits equal T's (keys are recomputed from the hash, never stored)
// and adds its non-empty bins to the row's global histogram of that pass with integer atomics.  The workgroups of the NEXT launch
// each walk that histogram downwards on their own — 2048 bins, the same answer in every workgroup — to fix the digit and the rank
// that remains inside its bin, so no launch exists only to scan.  When the bin holds exactly the remaining rank there is no tie to
// break: the row is done and its later passes return at once.  The kernel boundary is the only synchronisation; integer adds
// commute, so a histogram does not depend on arrival order or on the grid.  The last launch writes the k items with
// composite >= T (in arrival order: the caller sorts the k distinct sort keys, which makes the draw order unique).
#include "common.h"
#include "sample_device.h"

namespace roma {
namespace {

constexpr int RS_BINS = 2048, RS_PASSES = 6, RS_ITEMS = 8;
constexpr long RS_MAX_N = 1l << 24;

__host__ __device__ constexpr int rs_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
__host__ __device__ constexpr int rs_width(int pass) { return pass < 5 ? 11 : 9; }

struct RowState {
  unsigned long long T;      // the digits resolved so far, in place; the bits below them are 0
  uint32_t k_rem;            // rank of the wanted item among the candidates (items whose resolved digits equal T's), 1-based
  uint32_t done;             // T is final
  uint32_t pad;
};

__device__ __forceinline__ unsigned long long composite(float key, uint32_t ctr) {
  uint32_t b = __float_as_uint(key);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - ctr);
}

// workspace: RowState st[P][RS_PASSES] (st[r][i] = the state after pass i), uint32 count[P], uint32 hist[P][RS_PASSES][RS_BINS]
__host__ __device__ inline size_t rs_state_bytes(int P) { return (size_t)P * RS_PASSES * sizeof(RowState); }

__global__ __launch_bounds__(256) void rs_init_kernel(uint32_t* __restrict__ count_and_hist, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) count_and_hist[i] = 0;
}

// The state after pass `pass`, from the state before it and the pass's finished histogram: the bin that holds the k_rem-th largest
// candidate.  Called by all 256 threads of a workgroup; thread t owns the 8 bins below RS_BINS - 8 t.
__device__ __forceinline__ RowState rs_scan(const uint32_t* __restrict__ h, const RowState& s, int pass) {
  __shared__ uint32_t wsum[4];
  __shared__ RowState next;
  if (s.done) return s;                                  // uniform: s is the same in every thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t v[8], sum = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = h[RS_BINS - 1 - (8 * tid + j)];
    sum += v[j];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = incl - sum;                          // candidates in the bins above this thread's
  for (int q = 0; q < wave; ++q) before += wsum[q];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (before < s.k_rem && s.k_rem <= before + v[j]) {  // true for exactly one bin: the candidates number at least k_rem
      const uint32_t bin = RS_BINS - 1 - (8 * tid + j), rem = s.k_rem - before;
      next = RowState{s.T | ((unsigned long long)bin << rs_shift(pass)), rem, (v[j] == rem || pass == RS_PASSES - 1) ? 1u : 0u, 0u};
    }
    before += v[j];
  }
  __syncthreads();
  return next;
}

// the state before pass `pass` of a row: pass 0 starts from (T = 0, rank k); later passes scan the histogram of the pass before
__device__ __forceinline__ RowState rs_state_before(RowState* __restrict__ st, const uint32_t* __restrict__ hist, int row, int pass,
                                                    int k, bool writer) {
  const RowState first{0ull, (uint32_t)k, 0u, 0u};
  if (pass == 0) return first;
  const RowState prev = pass == 1 ? first : st[(size_t)row * RS_PASSES + pass - 2];
  const RowState s = rs_scan(hist + ((size_t)row * RS_PASSES + pass - 1) * RS_BINS, prev, pass - 1);
  if (writer && threadIdx.x == 0) st[(size_t)row * RS_PASSES + pass - 1] = s;     // for the next launch; every workgroup computes the same
  return s;
}

__global__ __launch_bounds__(256) void rs_hist_kernel(const float* __restrict__ p, const long* __restrict__ counter,
                                                      const long* __restrict__ seeds, RowState* __restrict__ st,
                                                      uint32_t* __restrict__ hist, long N, int k, float thresh, uint32_t stage,
                                                      int pass) {
  __shared__ uint32_t h[RS_BINS];
  const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const RowState s = rs_state_before(st, hist, row, pass, k, blockIdx.x == 0);
  if (s.done) return;
  for (int t = tid; t < RS_BINS; t += 256) h[t] = 0;
  __syncthreads();
  const float* pr = p + (size_t)row * N;
  const long* cr = counter ? counter + (size_t)row * N : nullptr;
  const uint32_t stream = race_stream((uint32_t)seeds[row], stage);
  const int shift = rs_shift(pass), hs = shift + rs_width(pass);
  const uint32_t mask = (1u << rs_width(pass)) - 1u;
  const unsigned long long want = hs < 64 ? (s.T >> hs) : 0ull;
  for (long base = (long)blockIdx.x * 256; base < N; base += (long)gridDim.x * 256) {     // uniform trip count per workgroup
    const long i = base + tid;
    bool cand = false;
    uint32_t digit = 0;
    if (i < N) {
      const uint32_t ctr = (uint32_t)(cr ? cr[i] : i);
      const unsigned long long c = composite(race_key(pr[i], thresh, stream, ctr), ctr);
      cand = hs >= 64 || (c >> hs) == want;
      digit = (uint32_t)(c >> shift) & mask;
    }
    // all-equal digits (every weight 0, or one exponent bin) would serialise 64 LDS adds on one address: one add per wave then
    const unsigned long long m = __ballot(cand);
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
      if (__ballot(cand && digit == d0) == m) {
        if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(m));
      } else if (cand) {
        atomicAdd(&h[digit], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* hg = hist + ((size_t)row * RS_PASSES + pass) * RS_BINS;
  for (int t = tid; t < RS_BINS; t += 256)
    if (h[t]) atomicAdd(&hg[t], h[t]);
}

__global__ __launch_bounds__(256) void rs_collect_kernel(const float* __restrict__ p, const long* __restrict__ counter,
                                                         const long* __restrict__ seeds, RowState* __restrict__ st,
                                                         const uint32_t* __restrict__ hist, uint32_t* __restrict__ count, long N,
                                                         int k, float thresh, uint32_t stage, long* __restrict__ sel_key,
                                                         long* __restrict__ sel_idx) {
  __shared__ uint32_t s_total, s_base;
  const int row = blockIdx.y, tid = threadIdx.x;
  const unsigned long long T = rs_state_before(st, hist, row, RS_PASSES, k, false).T;
  if (tid == 0) s_total = 0;
  __syncthreads();
  const float* pr = p + (size_t)row * N;
  const long* cr = counter ? counter + (size_t)row * N : nullptr;
  const uint32_t stream = race_stream((uint32_t)seeds[row], stage);
  const long base = (long)blockIdx.x * (256 * RS_ITEMS);
  unsigned long long c[RS_ITEMS];
  uint32_t sel = 0;
#pragma unroll
  for (int j = 0; j < RS_ITEMS; ++j) {
    const long i = base + j * 256 + tid;
    c[j] = 0;
    if (i < N) {
      const uint32_t ctr = (uint32_t)(cr ? cr[i] : i);
      c[j] = composite(race_key(pr[i], thresh, stream, ctr), ctr);
      if (c[j] >= T) sel |= 1u << j;
    }
  }
  const uint32_t cnt = __popc(sel);
  const uint32_t lbase = cnt ? atomicAdd(&s_total, cnt) : 0u;
  __syncthreads();
  if (tid == 0) s_base = s_total ? atomicAdd(&count[row], s_total) : 0u;      // one global add per workgroup
  __syncthreads();
  uint32_t o = s_base + lbase;
#pragma unroll
  for (int j = 0; j < RS_ITEMS; ++j) {
    if (!((sel >> j) & 1u)) continue;
    if (o < (uint32_t)k) {                                 // exactly k items pass; the bound keeps a broken invariant inside the buffer
      sel_key[(size_t)row * k + o] = (long)(c[j] ^ 0x8000000000000000ull);       // signed order = composite order
      sel_idx[(size_t)row * k + o] = base + j * 256 + tid;
    }
    ++o;
  }
}

// point j of pair blockIdx.y: row index[j] of the pair's (N,4) matches (row j when index is NULL), rounded to fp16 in half mode
template <bool HALF>
struct BatchPoints {
  const float4_t* x;
  const long* index;
  long N;
  __device__ __forceinline__ float4_t operator()(int j) const {
    long r = index ? index[j] : (long)j;
    r = r < 0 ? 0 : (r >= N ? N - 1 : r);                   // a bad index reads a wrong row, never outside the pair
    float4_t v = x[r];
    if (HALF) v = float4_t{r16(v[0]), r16(v[1]), r16(v[2]), r16(v[3])};
    return v;
  }
};

template <bool HALF>
__global__ __launch_bounds__(256) void kde_batch_kernel(const float4_t* __restrict__ x, const long* __restrict__ index,
                                                        float* __restrict__ density, long N, int n, int down, float neg_scale_log2,
                                                        float two_var) {
  const size_t pair = blockIdx.y;
  const BatchPoints<HALF> load{x + pair * (size_t)N, index ? index + pair * (size_t)n : nullptr, N};
  kde_body<HALF>(load, density + pair * (size_t)n, blockIdx.x, n, down, neg_scale_log2, two_var);
}

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_race_select_workspace(int P, long N, int k) {
  ROMA_REQUIRE(P >= 1 && P <= 65535 && N >= 1 && N <= RS_MAX_N && k >= 1 && k <= N, ROMA_E_SHAPE,
               "roma_race_select_workspace: bad shape P=%d N=%ld k=%d (1 <= P <= 65535, 1 <= k <= N <= 2^24)", P, N, k);
  return (long)(rs_state_bytes(P) + (size_t)P * sizeof(uint32_t) * (1 + RS_PASSES * RS_BINS));
}

extern "C" int roma_race_select(const float* p, const long* counter, const long* seeds, int P, long N, int k, float thresh,
                                unsigned stage, long* sel_key, long* sel_idx, void* workspace, long workspace_bytes, void* stream) {
  ROMA_REQUIRE(p && seeds && sel_key && sel_idx && workspace, ROMA_E_ARG, "roma_race_select: null pointer");
  ROMA_REQUIRE(P >= 1 && P <= 65535 && N >= 1 && N <= RS_MAX_N && k >= 1 && k <= N, ROMA_E_SHAPE,
               "roma_race_select: bad shape P=%d N=%ld k=%d (1 <= P <= 65535, 1 <= k <= N <= 2^24)", P, N, k);
  ROMA_REQUIRE(workspace_bytes >= roma_race_select_workspace(P, N, k), ROMA_E_ARG,
               "roma_race_select: workspace of %ld bytes, %ld needed", workspace_bytes, roma_race_select_workspace(P, N, k));
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, ROMA_E_ALIGN, "roma_race_select: workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowState* st = static_cast<RowState*>(workspace);
  uint32_t* count = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + rs_state_bytes(P));
  uint32_t* hist = count + P;
  // workgroups per row of a pass: enough to fill the device at small P; the result does not depend on it
  long cap = 1024 / P;
  if (cap < 64) cap = 64;
  long gx = (N + 2047) / 2048;
  if (gx > cap) gx = cap;
  const long nzero = (long)P * (1 + RS_PASSES * RS_BINS);
  long gz = (nzero + 2047) / 2048;
  if (gz > 256) gz = 256;
  hipLaunchKernelGGL(rs_init_kernel, dim3((unsigned)gz), dim3(256), 0, s, count, nzero);
  for (int pass = 0; pass < RS_PASSES; ++pass)
    hipLaunchKernelGGL(rs_hist_kernel, dim3((unsigned)gx, P), dim3(256), 0, s, p, counter, seeds, st, hist, N, k, thresh, (uint32_t)stage, pass);
  const long gc = (N + 256 * RS_ITEMS - 1) / (256 * RS_ITEMS);
  hipLaunchKernelGGL(rs_collect_kernel, dim3((unsigned)gc, P), dim3(256), 0, s, p, counter, seeds, st, hist, count, N, k, thresh,
                     (uint32_t)stage, sel_key, sel_idx);
  ROMA_CHECK_LAUNCH();
}

extern "C" int roma_kde_density_batch(const float* x, const long* index, float* density, int P, long N, int n, int down, float std,
                                      int half_mode, void* stream) {
  ROMA_REQUIRE(x && density, ROMA_E_ARG, "roma_kde_density_batch: null pointer");
  ROMA_REQUIRE(P >= 1 && P <= 65535 && n >= 1 && N >= 1 && N <= 0x7fffffffl && (index || N == n) && down >= 1 && std > 0.f, ROMA_E_SHAPE,
               "roma_kde_density_batch: bad arguments P=%d N=%ld n=%d down=%d std=%g (N == n without an index)", P, N, n, down, std);
  ROMA_REQUIRE(aligned16(x), ROMA_E_ALIGN, "roma_kde_density_batch: x must be 16-byte aligned");
  const float neg_scale_log2 = -1.4426950408889634f / (2.f * std * std);
  const float two_var = (float)(2.0 * (double)std * (double)std);
  const dim3 grid((n + KDE_QP - 1) / KDE_QP, P);
  if (half_mode)
    hipLaunchKernelGGL(kde_batch_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const float4_t*>(x),
                       index, density, N, n, down, neg_scale_log2, two_var);
  else
    hipLaunchKernelGGL(kde_batch_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const float4_t*>(x),
                       index, density, N, n, down, neg_scale_log2, two_var);
  ROMA_CHECK_LAUNCH();
}
