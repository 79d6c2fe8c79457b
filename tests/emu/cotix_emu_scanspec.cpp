// TEST INFRASTRUCTURE ONLY -- the host emulation of the step program with the
// key helper's level-1 key ring AND its speculative draw words
// (cotix_kernel.h scan_spec_fill / m_spec: the helper draws each cell's first
// M candidates ahead, the fused scan's round 0 settles from them), on the
// fiber lanes of cotix_emu.cpp.  As in cotix_emu_keyl1.cpp, whose entry points
// this library also carries, the helper's work up to its next barrier runs at
// each barrier of the step wave, and the barrier counts are compared with
// cxk::key_l1_barriers.  M is the kernel's cxk::SCAN_M, or a test build's
// -DCOTIX_EMU_SCAN_M (a list shorter than M).
#include "cotix_emu_keyl1.cpp"

#ifndef COTIX_EMU_SCAN_M
#define COTIX_EMU_SCAN_M cxk::SCAN_M
#endif

namespace {
constexpr int EMU_M = COTIX_EMU_SCAN_M;

template <int EW>
struct HostScanSpecHelp {
  static constexpr bool on = true;
  static constexpr bool l1 = true;
  static constexpr int spec = EMU_M;
  int kwalt;
  int l1o;
  int spo;
  cxk::KeyL1<EW>* h;
  const cxk::KArgs* a;
  const cxk::Ctx* c;
  const HostRun* run;
  int* nbar;
  void bar() const {
    ++*nbar;
    cxk::key_l1_next<EW>(*a, *c, *h, *run);
  }
};

int run_blocks_spec(const cxk::KArgs& a) {
  constexpr int EW = 4;
  const cxk::SceneDev& sc = *a.sc;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nwaves = (a.B + EW - 1) / EW;
  const int nk1 = cxk::key_l1_keys(sc, sc.hot);
  // exactly the words of one env group in the kernel's workgroup
  const int rw = cxk::help_region_words<EW>(c), hw = cxk::KWIN * c.L.kww * EW, gw = cxk::key_l1_ring_words<EW>(nk1),
            sw = cxk::scan_spec_ring_words<EW>(sc);
  if ((size_t)4 * (sc.nhot + 4 * (rw + hw + gw + sw)) != cxk::help_l1_lds_bytes<EW>(sc, 4, nk1, true))
    return g_err = "help_l1_lds_bytes is not the tables + 4 (region + window buffer + key ring + draw ring)", -1;
  if (sw != 2 * cxk::KL1R * c.nl * EW) return g_err = "the draw ring is not a word per item and ring step", -1;
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)rw + (size_t)hw + (size_t)gw + (size_t)sw);
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  const int want = cxk::key_l1_barriers(a);
  for (int wv = 0; wv < nwaves; ++wv) {
    std::fill(lds.begin() + sc.nhot, lds.end(), 0x7FBADBADu);  // poison
    const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
    uint32_t* const hb = lds.data() + sc.nhot + rw;
    uint32_t* const rb = hb + hw;
    uint32_t* const sb = rb + gw;
    const int env0 = wv * EW;
    int step_bars[64], help_bars[64], help_end[64];
    cxk_simt::run([&](int lane) {
      const HostRun run{lane};
      cxk::KeyL1<EW> kh;
      kh.kh.tm = t;
      kh.kh.th = cxk::Tile<EW>{hb - c.L.kw * EW, lds.data(), nullptr};
      kh.kh.env0 = env0;
      kh.l1o = (int)(rb - t.u) / EW;
      kh.nk1 = nk1;
      kh.sm = EMU_M;
      kh.spo = (int)(sb - t.u) / EW;
      int nbar = 0;
      const HostScanSpecHelp<EW> help{(int)(hb - t.u) / EW - c.L.kw, kh.l1o, kh.spo, &kh, &a, &c, &run, &nbar};
      cxk::run_wave<EW, 1, false, false, false>(a, c, t, env0, run, false, help);
      step_bars[lane] = nbar;
      help_bars[lane] = kh.q;
      help_end[lane] = kh.s0;
    });
    for (int l = 0; l < 64; ++l) {
      if (step_bars[l] != want || help_bars[l] != want)
        return g_err = "barriers: the step wave passed " + std::to_string(step_bars[l]) + ", the helper " +
                       std::to_string(help_bars[l]) + ", key_l1_barriers says " + std::to_string(want),
               -1;
      if (want > 0 && (help_end[l] < a.n_steps || help_end[l] >= a.n_steps + cxk::KL1R))
        return g_err = "the helper's last half ends at step " + std::to_string(help_end[l]) + " of " +
                       std::to_string(a.n_steps),
               -1;
    }
  }
  return 0;
}
}  // namespace

// emu_step_keyl1 through the form with the speculative draw words
extern "C" int emu_step_scanspec(void* scene, float* dyn, uint32_t* keys, uint32_t* err, const float* geom,
                                 int gstride, int B, int n_steps, float dt, int stages, const float* action,
                                 int action_body, const float* dyn_reset, uint32_t* resets, int32_t* chosen,
                                 int32_t* cells) {
  EmuScene* s = static_cast<EmuScene*>(scene);
  if (!cxl::key_helper_may_run(s->fnset, 4, n_steps) || !cxk::scan_fused<4>(cxk::make_ctx<4>(s->s)))
    return g_err = "not a launch of the level-1 key form", -1;
  cxk::KArgs a{};
  a.sc = &s->s;
  a.dyn = dyn;
  a.keys = keys;
  a.err = err;
  a.geom = geom;
  a.gstride = gstride;
  a.B = B;
  a.n_steps = n_steps;
  a.dt = dt;
  a.stages = stages;
  a.action = action;
  a.action_body = action_body;
  a.dyn_reset = dyn_reset;
  a.reset_mode = dyn_reset ? 1 : 0;
  a.resets = resets;
  a.trace_chosen = chosen;
  a.trace_cells = cells;
  return run_blocks_spec(a);
}

// the items that the scan's round 0 (cxk::m_spec) settled or finished since
// the last call: a launch's proof that the round-0 path ran
extern "C" unsigned long long emu_scanspec_round0_done() {
  const unsigned long long n = cxk::g_emu_round0_done;
  cxk::g_emu_round0_done = 0;
  return n;
}
// this build's M and the kernel's
extern "C" int emu_scanspec_m(int* kernel_m) {
  if (kernel_m) *kernel_m = cxk::SCAN_M;
  return EMU_M;
}
// the scene's cells: per cell ci, cj, the list length and (cand != null) its
// candidates in list order as the collider trace codes them
// (i1 | i2 << 9 | type << 18), at most `stride` per cell; returns nl
extern "C" int emu_scanspec_lists(void* scene, int* ci, int* cj, int* len, int32_t* cand, int stride) {
  const cxk::SceneDev& s = static_cast<EmuScene*>(scene)->s;
  for (int l = 0; l < s.nl; ++l) {
    ci[l] = (int)s.hot[s.o_ci + l];
    cj[l] = (int)s.hot[s.o_cj + l];
    len[l] = (int)s.hot[s.o_ccnt + l];
    for (int q = 0; cand != nullptr && q < len[l] && q < stride; ++q) {
      const uint32_t cd = s.hot[s.o_cand + s.hot[s.o_cbeg + l] + q];
      cand[l * stride + q] = (int32_t)((cd & 0x3FFFFu) | ((cd >> 27) << 18));
    }
  }
  return s.nl;
}
// the draw-word producer alone: the words of steps s0 .. s0 + n - 1 (n <= KL1R)
// from the ring keys l1keys u32 [n][nk1][2][4 envs] -> out u32 [n][nl][4]
extern "C" int emu_scanspec_fill(void* scene, const uint32_t* l1keys, int s0, int n, uint32_t* out) {
  constexpr int EW = 4;
  const cxk::SceneDev& sc = static_cast<EmuScene*>(scene)->s;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nk1 = cxk::key_l1_keys(sc, sc.hot);
  if (n < 1 || n > cxk::KL1R || s0 < 0 || s0 % cxk::KL1R != 0) return g_err = "s0 a half's first step, 1 <= n <= KL1R", -1;
  const int rw = cxk::help_region_words<EW>(c), gw = cxk::key_l1_ring_words<EW>(nk1),
            sw = cxk::scan_spec_ring_words<EW>(sc);
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)rw + (size_t)gw + (size_t)sw, 0x7FBADBADu);
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
  const int l1o = rw / EW, spo = (rw + gw) / EW;
  for (int s = 0; s < n; ++s)
    for (int q = 0; q < 2 * nk1 * EW; ++q)
      t.u[(size_t)(l1o + ((s0 + s) % (2 * cxk::KL1R)) * 2 * nk1) * EW + q] = l1keys[(size_t)s * 2 * nk1 * EW + q];
  cxk_simt::run([&](int lane) {
    const HostRun run{lane};
    run(cxk::PH_K, [&](int l) { cxk::scan_spec_fill<EW>(c, t, l1o, nk1, spo, EMU_M, s0, n, l); });
  });
  for (int s = 0; s < n; ++s)
    for (int q = 0; q < c.nl * EW; ++q)
      out[(size_t)s * c.nl * EW + q] = t.u[(size_t)(spo + ((s0 + s) % (2 * cxk::KL1R)) * c.nl) * EW + q];
  return c.nl;
}
