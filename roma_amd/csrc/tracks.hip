// Multi-view tracks from pairwise matches (DESIGN.md §3.4 "Tracks from pairwise matches", include/roma_hip.h roma_build_tracks;
// tests/tracks_ref.py restates every step in numpy and the outputs are compared for equality).
//
// Every view is cut into cells of `cell` pixels; a cell that receives a usable match endpoint is a node, a usable match is an edge
// between its two nodes, and a connected component that has at most one node per view is a track.  Eight launches on one stream, the
// kernel boundary the only synchronisation between them:
//   init      per-cell state (parent[i] = i), outputs and counters
//   endpoints one 64-bit atomic max per endpoint: the cell's representative = highest certainty, then lowest endpoint index
//   union     lock-free union-find (ECL-CC, Jaiganesh & Burtscher, HPDC 2018): path halving, the larger root hooked under the
//             smaller by compare-and-swap.  parent[i] <= i always and only ever decreases, so every walk ends and every value a
//             load can return, fresh or stale, is an ancestor of i; a lost compare-and-swap returns the winner's value, so a retry
//             always starts lower.  No thread waits for another.
//   flatten   parent[i] = root(i); views[root] |= bit(view of i); a bit that was already there marks the root as conflicting
//   count     per block of 256 cells: qualifying, conflicting and too-short roots
//   scan      one workgroup: exclusive scan of the qualifying counts, the three totals
//   rank      row[root] = its rank among the qualifying roots (ascending root id), -1 for every other cell or a rank >= T
//   scatter   x / visible per node, track_of_match per match
// Integer atomics only (max, or, compare-and-swap), all of them set operations: no result depends on the order of arrival.
#include <algorithm>
#include "multiview.h"

namespace roma {
namespace {

constexpr int THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr unsigned UNION_RETRY_CAP = 1u << 20;      // a guard against a mistake hanging the device, not a path correct code takes

struct TrackGrid {                  // per view, prepared on the host
  int base[MAX_VIEWS + 1];          // global id of the view's first cell; base[V] = C
  int wc[MAX_VIEWS], hc[MAX_VIEWS]; // cells per row, rows of cells
  float w[MAX_VIEWS], h[MAX_VIEWS]; // the size in pixels
  float hw[MAX_VIEWS], hh[MAX_VIEWS];  // 0.5f * size
};

struct TrackParams {
  const float4* matches;
  const float* certainty;
  const unsigned char* mask;
  const int* pairs;
  long mk;                          // M * k
  int k, V, C, T;
  float inv_cell, thresh;
};

struct Workspace {
  unsigned long long* key;          // (C) the representative's key, 0 = the cell is no node
  unsigned* parent;                 // (C)
  unsigned* views;                  // (C) at a root: the views of its component
  int* row;                         // (C) written by the rank kernel
  unsigned* block_counts;           // (blocks, 3)
  unsigned char* conflict;          // (C) at a root
};

__device__ __forceinline__ unsigned load_parent(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_parent(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// pixels and global cell id of a normalised endpoint in view v; false = outside (NaN included)
__device__ __forceinline__ bool endpoint(const TrackGrid& g, int v, float x, float y, float inv, float& px, float& py, int& id) {
  px = (x + 1.0f) * g.hw[v];
  py = (y + 1.0f) * g.hh[v];
  if (!(px >= 0.f && px < g.w[v] && py >= 0.f && py < g.h[v])) return false;
  const int cx = (int)floorf(px * inv), cy = (int)floorf(py * inv);
  if (cx >= g.wc[v] || cy >= g.hc[v]) return false;
  id = g.base[v] + cy * g.wc[v] + cx;
  return true;
}

// the two nodes of match e (flat index over (M,k)); false = not usable
__device__ __forceinline__ bool match_edge(const TrackParams& p, const TrackGrid& g, long e, int& ca, int& cb) {
  const long m = e / p.k;
  const int a = p.pairs[2 * m], b = p.pairs[2 * m + 1];
  if ((unsigned)a >= (unsigned)p.V || (unsigned)b >= (unsigned)p.V || a == b) return false;
  const float c = p.certainty[e];
  if (!(c > p.thresh && c < __builtin_inff())) return false;
  if (p.mask && !p.mask[e]) return false;
  const float4 r = p.matches[e];
  float px, py;
  return endpoint(g, a, r.x, r.y, p.inv_cell, px, py, ca) && endpoint(g, b, r.z, r.w, p.inv_cell, px, py, cb);
}

__device__ __forceinline__ int view_of_cell(const TrackGrid& g, int V, int id) {
  int v = 0;
  while (v + 1 < V && id >= g.base[v + 1]) ++v;
  return v;
}

__global__ void __launch_bounds__(THREADS) tracks_init_kernel(Workspace ws, int C, float* x, unsigned char* visible, long vt, int* views,
                                                              unsigned char* num_views, int T, int* track_of_match, long mk, int* counts) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i < C) {
    ws.key[i] = 0ull;
    ws.parent[i] = (unsigned)i;
    ws.views[i] = 0u;
    ws.conflict[i] = 0;
  }
  if (i < vt) {
    x[2 * i] = __builtin_nanf("");
    x[2 * i + 1] = __builtin_nanf("");
    visible[i] = 0;
  }
  if (i < T) {
    views[i] = 0;
    num_views[i] = 0;
  }
  if (i < mk) track_of_match[i] = -1;
  if (i < 4) counts[i] = 0;
}

__global__ void __launch_bounds__(THREADS) tracks_endpoints_kernel(TrackParams p, TrackGrid g, Workspace ws) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= p.mk) return;
  int ca, cb;
  if (!match_edge(p, g, e, ca, cb)) return;
  const unsigned long long hi = (unsigned long long)__float_as_uint(p.certainty[e]) << 32;
  const unsigned idx = (unsigned)(2 * e);
  atomicMax(&ws.key[ca], hi | (0xFFFFFFFFu - idx));
  atomicMax(&ws.key[cb], hi | (0xFFFFFFFFu - (idx + 1u)));
}

// the root of i, halving the path on the way: every store replaces a parent by a further ancestor
__device__ __forceinline__ unsigned find_root(unsigned* parent, unsigned i) {
  unsigned cur = load_parent(parent + i);
  if (cur == i) return i;
  unsigned prev = i, next;
  while (cur > (next = load_parent(parent + cur))) {
    store_parent(parent + prev, next);
    prev = cur;
    cur = next;
  }
  return cur;
}

__global__ void __launch_bounds__(THREADS) tracks_union_kernel(TrackParams p, TrackGrid g, Workspace ws, int* counts) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= p.mk) return;
  int ca, cb;
  if (!match_edge(p, g, e, ca, cb)) return;
  unsigned a = find_root(ws.parent, (unsigned)ca), b = find_root(ws.parent, (unsigned)cb);
  unsigned rounds = 0;
  while (a != b) {
    const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
    const unsigned old = atomicCAS(&ws.parent[hi], hi, lo);
    if (old == hi) break;                           // hooked
    if (++rounds == UNION_RETRY_CAP) {
      atomicOr(&counts[3], 1);
      break;
    }
    a = find_root(ws.parent, old);                  // another hook of hi won: go on from where it points
    b = find_root(ws.parent, lo);
  }
}

__global__ void __launch_bounds__(THREADS) tracks_flatten_kernel(TrackGrid g, Workspace ws, int C, int V) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= C || ws.key[i] == 0ull) return;
  unsigned root = (unsigned)i, up;
  while ((up = load_parent(ws.parent + root)) != root) root = up;    // roots do not change in this launch
  store_parent(ws.parent + i, root);
  const unsigned bit = 1u << view_of_cell(g, V, (int)i);
  // A bit found set was set by another node of this view, so the component conflicts whichever of the two came first; a load that
  // is behind the times only sends this node to the atomic.  Without the two loads every node of a large component adds an atomic
  // and a store to one address: 47 ms of a 59 ms call at 8 M nodes in a handful of components (profiles/tracks_micro.txt).
  unsigned seen = __hip_atomic_load(&ws.views[root], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!(seen & bit)) seen = atomicOr(&ws.views[root], bit);
  if ((seen & bit) && !__hip_atomic_load(&ws.conflict[root], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ws.conflict[root] = 1;
}

// 0: no root of a component, 1: qualifies, 2: conflicting, 3: fewer than min_views views
__device__ __forceinline__ int classify(const Workspace& ws, long i, int C, int min_views) {
  if (i >= C || ws.key[i] == 0ull || ws.parent[i] != (unsigned)i) return 0;
  if (ws.conflict[i]) return 2;
  return __popc(ws.views[i]) >= min_views ? 1 : 3;
}

__global__ void __launch_bounds__(THREADS) tracks_count_kernel(Workspace ws, int C, int min_views) {
  __shared__ unsigned s_n[3][THREADS / 64];
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const int cls = classify(ws, i, C, min_views);
  const int wave = threadIdx.x >> 6;
  for (int c = 0; c < 3; ++c) {
    const unsigned n = (unsigned)__popcll(__ballot(cls == c + 1));
    if ((threadIdx.x & 63) == 0) s_n[c][wave] = n;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned n = 0;
    for (int w = 0; w < THREADS / 64; ++w) n += s_n[threadIdx.x][w];
    ws.block_counts[3 * (size_t)blockIdx.x + threadIdx.x] = n;
  }
}

// (the loop of depth_fuse.hip's fuse_scan_kernel, written out in both: profiles/multiview_shared_code_micro.txt)
// one workgroup: block_counts[b][0] becomes the number of qualifying roots in the blocks before b; counts[0..2] the totals
__global__ void __launch_bounds__(SCAN_THREADS) tracks_scan_kernel(Workspace ws, int blocks, int* counts) {
  __shared__ unsigned s_wave[SCAN_THREADS / 64];
  __shared__ unsigned s_tot[2][SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0, conflicting = 0, too_short = 0;
  for (int b0 = 0; b0 < blocks; b0 += SCAN_THREADS) {
    const int b = b0 + threadIdx.x;
    const unsigned v = b < blocks ? ws.block_counts[3 * (size_t)b] : 0u;
    if (b < blocks) {
      conflicting += ws.block_counts[3 * (size_t)b + 1];
      too_short += ws.block_counts[3 * (size_t)b + 2];
    }
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const unsigned n = s_wave[w];
      if (w < wave) before += n;
      total += n;
    }
    if (b < blocks) ws.block_counts[3 * (size_t)b] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) {
    conflicting += __shfl_xor(conflicting, o, 64);
    too_short += __shfl_xor(too_short, o, 64);
  }
  if (lane == 0) { s_tot[0][wave] = conflicting; s_tot[1][wave] = too_short; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0, s = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) { c += s_tot[0][w]; s += s_tot[1][w]; }
    counts[0] = (int)carry;
    counts[1] = (int)c;
    counts[2] = (int)s;
  }
}

__global__ void __launch_bounds__(THREADS) tracks_rank_kernel(Workspace ws, int C, int min_views, int T, int* views, unsigned char* num_views) {
  __shared__ unsigned s_n[THREADS / 64];
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const bool q = classify(ws, i, C, min_views) == 1;
  const unsigned long long votes = __ballot(q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_n[wave] = (unsigned)__popcll(votes);
  __syncthreads();
  if (i >= C) return;
  unsigned r = ws.block_counts[3 * (size_t)blockIdx.x] + (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) r += s_n[w];
  const bool kept = q && r < (unsigned)T;
  ws.row[i] = kept ? (int)r : -1;
  if (kept) {
    const unsigned seen = ws.views[i];
    views[r] = (int)seen;
    num_views[r] = (unsigned char)__popc(seen);
  }
}

__global__ void __launch_bounds__(THREADS) tracks_scatter_kernel(TrackParams p, TrackGrid g, Workspace ws, float* x, unsigned char* visible,
                                                                 int* track_of_match) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i < p.C) {
    const unsigned long long key = ws.key[i];
    const int r = key ? ws.row[ws.parent[i]] : -1;
    if (r >= 0) {
      // the representative: the endpoint named in the key's low word
      const unsigned idx = 0xFFFFFFFFu - (unsigned)key;
      const long e = idx >> 1;
      const int side = idx & 1;
      const int v = p.pairs[2 * (e / p.k) + side];
      const float4 m = p.matches[e];
      float px, py;
      int id;
      endpoint(g, v, side ? m.z : m.x, side ? m.w : m.y, p.inv_cell, px, py, id);
      const size_t o = (size_t)v * p.T + r;
      x[2 * o] = px;
      x[2 * o + 1] = py;
      visible[o] = 1;
    }
  }
  if (i < p.mk) {
    int ca, cb;
    if (match_edge(p, g, i, ca, cb)) track_of_match[i] = ws.row[ws.parent[ca]];
  }
}

// the grid of cells; 0, or a negative code with the error set
int make_grid(const char* who, int V, const int* sizes, int cell, TrackGrid& g) {
  ROMA_REQUIRE(sizes, ROMA_E_ARG, "%s: null pointer", who);
  ROMA_REQUIRE(V >= 2 && V <= MAX_VIEWS, ROMA_E_SHAPE, "%s: bad shape V=%d (2 to %d views)", who, V, MAX_VIEWS);
  ROMA_REQUIRE(cell >= 1 && cell <= 64, ROMA_E_ARG, "%s: cell must be in [1, 64] pixels, got %d", who, cell);
  long total = 0;
  for (int v = 0; v < MAX_VIEWS; ++v) {
    const int u = v < V ? v : 0;
    const int H = sizes[2 * u], W = sizes[2 * u + 1];
    ROMA_REQUIRE(H >= 1 && H <= 65536 && W >= 1 && W <= 65536, ROMA_E_SHAPE, "%s: bad shape of view %d: %d x %d (1 to 65536 pixels a side)", who,
                 u, H, W);
    g.wc[v] = (W + cell - 1) / cell;
    g.hc[v] = (H + cell - 1) / cell;
    g.w[v] = (float)W; g.h[v] = (float)H;
    g.hw[v] = 0.5f * (float)W; g.hh[v] = 0.5f * (float)H;
    if (v < V) {
      ROMA_REQUIRE(total < (1L << 31), ROMA_E_SHAPE, "%s: 2^31 cells or more; use a larger cell", who);
      g.base[v] = (int)total;
      total += (long)g.wc[v] * g.hc[v];
    }
  }
  ROMA_REQUIRE(total < (1L << 31), ROMA_E_SHAPE, "%s: %ld cells, the limit is 2^31 - 1; use a larger cell", who, total);
  for (int v = V; v <= MAX_VIEWS; ++v) g.base[v] = (int)total;
  return 0;
}

inline long blocks_of(long n) { return (n + THREADS - 1) / THREADS; }
inline long workspace_bytes(long C) { return (21 * C + 12 * blocks_of(C) + 15) & ~15L; }

}  // namespace
}  // namespace roma

using namespace roma;

extern "C" long roma_tracks_workspace(int V, const int* sizes, int cell, long* cells) {
  TrackGrid g;
  if (int rc = make_grid("roma_tracks_workspace", V, sizes, cell, g)) return rc;
  if (cells) *cells = g.base[V];
  return workspace_bytes(g.base[V]);
}

extern "C" int roma_build_tracks(const float* matches, const float* certainty, const unsigned char* mask, const int* pairs, const int* sizes,
                                 int M, int k, int V, int cell, float certainty_thresh, int min_views, int T, float* x,
                                 unsigned char* visible, int* views, unsigned char* num_views, int* track_of_match, int* counts,
                                 void* workspace, long workspace_size, void* stream) {
  ROMA_REQUIRE(matches && certainty && pairs && sizes && x && visible && views && num_views && track_of_match && counts && workspace,
               ROMA_E_ARG, "roma_build_tracks: null pointer");
  TrackGrid g;
  if (int rc = make_grid("roma_build_tracks", V, sizes, cell, g)) return rc;
  ROMA_REQUIRE(M >= 1 && k >= 1 && (long)M * k < (1L << 31), ROMA_E_SHAPE, "roma_build_tracks: bad shape M=%d k=%d (M * k from 1 to 2^31 - 1)", M,
               k);
  ROMA_REQUIRE(T >= 1 && (long)V * T < (1L << 30), ROMA_E_SHAPE, "roma_build_tracks: bad shape max_tracks=%d (at least 1, V * max_tracks < 2^30)",
               T);
  ROMA_REQUIRE(min_views >= 2 && min_views <= V, ROMA_E_ARG, "roma_build_tracks: min_views must be in [2, V=%d], got %d", V, min_views);
  ROMA_REQUIRE(certainty_thresh >= 0.f && certainty_thresh < __builtin_inff(), ROMA_E_ARG,
               "roma_build_tracks: certainty_thresh must be finite and not negative, got %g", (double)certainty_thresh);
  const long C = g.base[V];
  ROMA_REQUIRE(workspace_size >= workspace_bytes(C), ROMA_E_SHAPE, "roma_build_tracks: workspace of %ld bytes, roma_tracks_workspace asks for %ld",
               workspace_size, workspace_bytes(C));
  ROMA_REQUIRE(aligned16(matches) && aligned16(workspace), ROMA_E_ALIGN, "roma_build_tracks: matches and workspace must be 16-byte aligned");
  ROMA_REQUIRE(aligned8(x) && aligned4(certainty) && aligned4(pairs) && aligned4(views) && aligned4(track_of_match) && aligned4(counts),
               ROMA_E_ALIGN, "roma_build_tracks: a pointer is not aligned to its element");

  const long mk = (long)M * k, vt = (long)V * T;
  TrackParams p;
  p.matches = reinterpret_cast<const float4*>(matches); p.certainty = certainty; p.mask = mask; p.pairs = pairs;
  p.mk = mk; p.k = k; p.V = V; p.C = (int)C; p.T = T;
  p.inv_cell = 1.0f / (float)cell; p.thresh = certainty_thresh;
  const long cell_blocks = blocks_of(C);
  Workspace ws;
  char* at = static_cast<char*>(workspace);
  ws.key = reinterpret_cast<unsigned long long*>(at); at += 8 * C;
  ws.parent = reinterpret_cast<unsigned*>(at); at += 4 * C;
  ws.views = reinterpret_cast<unsigned*>(at); at += 4 * C;
  ws.row = reinterpret_cast<int*>(at); at += 4 * C;
  ws.block_counts = reinterpret_cast<unsigned*>(at); at += 12 * cell_blocks;
  ws.conflict = reinterpret_cast<unsigned char*>(at);

  hipStream_t s = static_cast<hipStream_t>(stream);
  const long most = std::max(std::max(C, mk), std::max(vt, (long)T));
  const dim3 block(THREADS);
  hipLaunchKernelGGL(tracks_init_kernel, dim3((unsigned)blocks_of(most)), block, 0, s, ws, (int)C, x, visible, vt, views, num_views, T,
                     track_of_match, mk, counts);
  hipLaunchKernelGGL(tracks_endpoints_kernel, dim3((unsigned)blocks_of(mk)), block, 0, s, p, g, ws);
  hipLaunchKernelGGL(tracks_union_kernel, dim3((unsigned)blocks_of(mk)), block, 0, s, p, g, ws, counts);
  hipLaunchKernelGGL(tracks_flatten_kernel, dim3((unsigned)cell_blocks), block, 0, s, g, ws, (int)C, V);
  hipLaunchKernelGGL(tracks_count_kernel, dim3((unsigned)cell_blocks), block, 0, s, ws, (int)C, min_views);
  hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, ws, (int)cell_blocks, counts);
  hipLaunchKernelGGL(tracks_rank_kernel, dim3((unsigned)cell_blocks), block, 0, s, ws, (int)C, min_views, T, views, num_views);
  hipLaunchKernelGGL(tracks_scatter_kernel, dim3((unsigned)blocks_of(std::max(C, mk))), block, 0, s, p, g, ws, x, visible, track_of_match);
  ROMA_CHECK_LAUNCH();
}
