// multiview.h's fill_obs_table alone under ASan + UBSan: a CPU program of its own (`make -C roma_amd/csrc multiview_host_check`), never
// part of the library.  The table is filled from exactly V pointers, V scale rows and V visibility pointers, each in a heap block of
// exactly that size, so a read past view V - 1 is reported; the pointers themselves are never followed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../roma_amd/csrc/multiview.h"

using namespace roma;

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void run(int V, int null_view, int odd_view, bool with_px, bool with_vis) {
  alignas(16) static float pixels[MAX_VIEWS][4];
  static unsigned char seen[MAX_VIEWS][4];
  std::vector<const float*> obs(V);
  std::vector<const unsigned char*> vis(V);
  std::vector<float> px(4 * V);
  for (int v = 0; v < V; ++v) {
    obs[v] = v == null_view ? nullptr : pixels[v] + (v == odd_view ? 1 : 0);
    vis[v] = seen[v];
    for (int i = 0; i < 4; ++i) px[4 * v + i] = (float)(10 * v + i);
  }
  ObsTable tab;
  std::memset(&tab, 0xff, sizeof(tab));
  const int rc = fill_obs_table("check", obs.data(), with_px ? px.data() : nullptr, with_vis ? vis.data() : nullptr, V, tab);
  const char* msg = roma_last_error();
  if (null_view >= 0 && (odd_view < 0 || null_view < odd_view)) {
    char want[96];
    std::snprintf(want, sizeof want, "check: null pointer (observations of view %d)", null_view);
    EXPECT(rc == ROMA_E_ARG && std::strcmp(msg, want) == 0);
    return;
  }
  if (odd_view >= 0) {
    char want[96];
    std::snprintf(want, sizeof want, "check: the observations of view %d must be 8-byte aligned", odd_view);
    EXPECT(rc == ROMA_E_ALIGN && std::strcmp(msg, want) == 0);
    return;
  }
  EXPECT(rc == 0);
  for (int v = 0; v < MAX_VIEWS; ++v) {
    const int u = v < V ? v : 0;                                       // the entries above V repeat view 0
    EXPECT(tab.obs[v] == obs[u] && tab.vis[v] == (with_vis ? vis[u] : nullptr));
    for (int i = 0; i < 4; ++i) EXPECT(tab.px[v][i] == (with_px ? px[4 * u + i] : ((i & 1) ? 0.f : 1.f)));
  }
}

int main() {
  for (int V : {2, 3, MAX_VIEWS})
    for (int px = 0; px < 2; ++px)
      for (int vis = 0; vis < 2; ++vis) {
        run(V, -1, -1, px, vis);
        run(V, V - 1, -1, px, vis);                                    // a null view
        run(V, 0, -1, px, vis);
        run(V, -1, V - 1, px, vis);                                    // a misaligned view
        run(V, -1, 0, px, vis);
        run(V, 1, 0, px, vis);                                         // the first refusal in view order wins
      }
  std::printf(failures ? "%d checks failed\n" : "fill_obs_table: every check passed\n", failures);
  return failures ? 1 : 0;
}
