// PERF TOOLING ONLY -- the host emulation built with -DCOTIX_STATS
// (tools/collider_stats.py), with the fused scan's settle positions:
// out[0..17] the kernel's histogram (0..15, >= 16, list ran out), then for
// M = 2, 4, 8 what a round 0 over each item's first M candidates would leave:
// out[18..20] the items still pending, out[21..23] the lazy rounds they take.
// The replay is this file's: the kernel hands over every lane's two owner
// items at the end of a scan (cxk::g_settle_hook), 64 calls make a wave-step,
// and the rounds follow ph_M_fused's rule (the first min(n, ranks) pending
// items in id order draw G = 64 / min(n, ranks) candidates each).
// Call emu_stats_settle before emu_stats, which clears the kernel's counters.
#include "../tests/emu/cotix_emu.cpp"

namespace {
int s_at[2 * cxk::WAVE], s_len[2 * cxk::WAVE], s_calls = 0;
unsigned long long s_left[3], s_rounds[3];

void replay() {
  using namespace cxk;
  for (int k = 0; k < 3; ++k) {
    const int M = 2 << k;
    int d[2 * WAVE], ex[2 * WAVE], n = 0;  // pending items in id order: candidates to go, "runs out"
    for (int id = 0; id < 2 * WAVE; ++id)
      if (s_at[id] >= M && s_len[id] > M) {
        ex[n] = s_at[id] == s_len[id];
        d[n++] = s_at[id] - M;
      }
    s_left[k] += n;
    while (n > 0) {
      ++s_rounds[k];
      const int ns = n < COTIX_SCAN_RANKS ? n : COTIX_SCAN_RANKS, G = lanes_per_item(ns);
      int m = 0;
      for (int q = 0; q < n; ++q) {
        // a drawing item is done when its winner is among the G drawn, or its list ends there
        const bool done = q < ns && (ex[q] ? d[q] <= G : d[q] < G);
        if (q < ns) d[q] -= G;
        if (!done) {
          d[m] = d[q];
          ex[m++] = ex[q];
        }
      }
      n = m;
    }
  }
}
void hook(int lane, int at0, int len0, int at1, int len1) {
  s_at[lane] = at0;
  s_len[lane] = len0;
  s_at[lane + cxk::WAVE] = at1;
  s_len[lane + cxk::WAVE] = len1;
  if (++s_calls == cxk::WAVE) {  // every lane of the wave-step has reported
    s_calls = 0;
    replay();
  }
}
}  // namespace

extern "C" int emu_stats_settle(unsigned long long* out) {
  for (int q = 0; q < 18; ++q) out[q] = cxk::g_stats.settle[q];
  for (int k = 0; k < 3; ++k) {
    out[18 + k] = s_left[k];
    out[21 + k] = s_rounds[k];
    s_left[k] = s_rounds[k] = 0;
  }
  cxk::g_settle_hook = hook;  // (the first call arms the replay)
  return 24;
}
