// TEST INFRASTRUCTURE ONLY -- the host emulation of the step program with the
// key helper's level-1 key ring (cotix_kernel.h KeyL1 / key_l1_next, m_draw's
// L1 variant) on the 64 fiber lanes of cotix_emu.cpp, whose entry points this
// library also carries.  The helper's work up to its next barrier runs at each
// barrier of the step wave, so the two sides' counts are equal by
// construction; what is checked is that they equal the launch's count function
// (cxk::key_l1_barriers: the number the GPU's helper and idle waves loop to)
// and that the helper's last half is the launch's last.  The helper's work
// runs here at the barrier that releases it, not one interval earlier as on
// the GPU: a half or window overwritten while the step wave still reads it
// would not show here.  That the schedule has no such overwrite is argued in
// cotix_kernel.h (call q writes half q & 1 and window buffer (q KL1R / KWIN) & 1
// while the step wave reads the other ones), not tested.
#include "cotix_emu.cpp"

namespace {
// the step wave's side: windows and ring halves computed at its barriers
template <int EW>
struct HostKeyL1Help {
  static constexpr bool on = true;
  static constexpr bool l1 = true;
  int kwalt;
  int l1o;
  cxk::KeyL1<EW>* h;
  const cxk::KArgs* a;
  const cxk::Ctx* c;
  const HostRun* run;
  int* nbar;  // the step wave's barriers (this lane's count)
  void bar() const {
    ++*nbar;
    cxk::key_l1_next<EW>(*a, *c, *h, *run);
  }
};

// 0, or -1 with the reason: a wave whose barrier counts differ
int run_blocks_l1(const cxk::KArgs& a) {
  constexpr int EW = 4;
  const cxk::SceneDev& sc = *a.sc;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nwaves = (a.B + EW - 1) / EW;
  const int nk1 = cxk::key_l1_keys(sc, sc.hot);
  // the tables, the wave's region, the helper's window buffer, the ring:
  // exactly the words of one env group in the kernel's workgroup
  const int rw = cxk::help_region_words<EW>(c), hw = cxk::KWIN * c.L.kww * EW, gw = cxk::key_l1_ring_words<EW>(nk1);
  if ((size_t)4 * (sc.nhot + 4 * (rw + hw + gw)) != cxk::help_l1_lds_bytes<EW>(sc, 4, nk1))
    return g_err = "help_l1_lds_bytes is not the tables + 4 (region + window buffer + ring)", -1;
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)rw + (size_t)hw + (size_t)gw);
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  const int want = cxk::key_l1_barriers(a);
  for (int wv = 0; wv < nwaves; ++wv) {
    std::fill(lds.begin() + sc.nhot, lds.end(), 0x7FBADBADu);  // poison (a NaN pattern)
    const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
    uint32_t* const hb = lds.data() + sc.nhot + rw;
    uint32_t* const rb = hb + hw;
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
      int nbar = 0;
      const HostKeyL1Help<EW> help{(int)(hb - t.u) / EW - c.L.kw, kh.l1o, &kh, &a, &c, &run, &nbar};
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

// emu_step_ex through the step program with the level-1 key ring (4 envs per
// wave, the analytic program, more than one key window, the fused scan)
extern "C" int emu_step_keyl1(void* scene, float* dyn, uint32_t* keys, uint32_t* err, const float* geom, int gstride,
                              int B, int n_steps, float dt, int stages, const float* action, int action_body,
                              const float* dyn_reset, uint32_t* resets, int32_t* chosen, int32_t* cells) {
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
  return run_blocks_l1(a);
}

// the scene's types and their first-level split sizes (tn2); returns nt
extern "C" int emu_keyl1_tn2(void* scene, int* out, int n) {
  const cxk::SceneDev& s = static_cast<EmuScene*>(scene)->s;
  for (int q = 0; q < s.nt && q < n; ++q) out[q] = (int)s.hot[s.o_tn2 + q];
  return s.nt;
}
// the ring producer alone: the slots of steps s0 .. s0 + n - 1 (n <= KL1R) from
// the type keys tkeys u32 [n][nt][2][4 envs] -> out u32 [n][nk1][2][4]
extern "C" int emu_keyl1_fill(void* scene, const uint32_t* tkeys, int s0, int n, uint32_t* out) {
  constexpr int EW = 4;
  const cxk::SceneDev& sc = static_cast<EmuScene*>(scene)->s;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nk1 = cxk::key_l1_keys(sc, sc.hot);
  if (n < 1 || n > cxk::KL1R || s0 < 0 || s0 % cxk::KL1R != 0) return g_err = "s0 a half's first step, 1 <= n <= KL1R", -1;
  const int rw = cxk::help_region_words<EW>(c), gw = cxk::key_l1_ring_words<EW>(nk1);
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)rw + (size_t)gw, 0x7FBADBADu);
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
  const int l1o = rw / EW;
  for (int s = 0; s < n; ++s)
    for (int ty = 0; ty < sc.nt; ++ty)
      for (int w = 0; w < 2; ++w)
        for (int e = 0; e < EW; ++e)
          t.w(c.L.kw + ((s0 + s) % cxk::KWIN) * c.L.kww + 2 + 2 * ty + w, e) = tkeys[((s * sc.nt + ty) * 2 + w) * EW + e];
  cxk_simt::run([&](int lane) {
    const HostRun run{lane};
    run(cxk::PH_K, [&](int l) { cxk::key_l1_fill<EW>(c, t, t, l1o, nk1, s0, n, l); });
  });
  for (int s = 0; s < n; ++s)
    for (int q = 0; q < 2 * nk1 * EW; ++q)
      out[(size_t)s * 2 * nk1 * EW + q] = t.u[(size_t)(l1o + ((s0 + s) % (2 * cxk::KL1R)) * 2 * nk1) * EW + q];
  return nk1;
}
// split(key, num)[idx] in the scene's PRNG layout (cx::split_at_l, the step wave's expression)
extern "C" int emu_keyl1_split_at(void* scene, const uint32_t* key, int num, int idx, uint32_t* out) {
  const cxk::SceneDev& sc = static_cast<EmuScene*>(scene)->s;
  const cx::key2 r = cx::split_at_l(cx::key2{key[0], key[1]}, (uint32_t)num, (uint32_t)idx, sc.prng != 0);
  out[0] = r.a;
  out[1] = r.b;
  return 0;
}
