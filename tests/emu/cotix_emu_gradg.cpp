// TEST INFRASTRUCTURE ONLY -- the host emulation's backward with the shape
// geometry's gradient (cotix_rollout_backward_ex3's grad_geom): the level-2
// instantiations of the kernel's backward wave programs (cotix_kernel.h
// run_wave_backward_tape / run_wave_backward, GP == 2) on the 64 fiber lanes
// of cotix_emu.cpp, whose entry points this library also carries.  Built with
// -DCOTIX_NO_GREGS it runs phase G's tile form on every scene.
#include "cotix_emu.cpp"

namespace {
template <int EW>
void run_blocks_gg(const cxk::KArgs& a, bool tape) {
  const cxk::SceneDev& sc = *a.sc;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nwaves = (a.B + EW - 1) / EW;
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)cxk::help_region_words<EW>(c));
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  // the plan's contact-function program (a launch with grad_geom is never the split form)
  const int F = cxk::launch_fnset(sc.fnset, tape ? 4 : 2);
  for (int wv = 0; wv < nwaves; ++wv) {
    std::fill(lds.begin() + sc.nhot, lds.end(), 0x7FBADBADu);  // poison (a NaN pattern)
    const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
    const int env0 = wv * EW;
    cxk_simt::run([&](int lane) {
      const HostRun run{lane};
      if (tape)
        F == 1 ? cxk::run_wave_backward_tape<EW, 1, 2>(a, c, t, env0, run)
               : cxk::run_wave_backward_tape<EW, 15, 2>(a, c, t, env0, run);
      else
        F == 1 ? cxk::run_wave_backward<EW, 1, 2>(a, c, t, env0, run)
               : cxk::run_wave_backward<EW, 15, 2>(a, c, t, env0, run);
    });
  }
}
}  // namespace

// the rows of grad_geom (cotix_scene_geom_part_words)
extern "C" int emu_geom_part_words(void* scene) { return cxk::geom_part_words(static_cast<EmuScene*>(scene)->s); }

// emu_rollout_backward plus grad_geom f32 [GW][B] (required) and grad_params
// f32 [nb][4][B] (nullable); the library's argument checks (cotix_step.hip)
extern "C" int emu_rollout_backward_geom(void* scene, const float* saved_dyn, const uint32_t* saved_keys,
                                         const uint32_t* tape, const float* geom, int gstride, int B, int n_steps,
                                         float dt, int stages, const float* action, int action_body,
                                         const float* ret_w, float* grad_action, float* grad_dyn0, float* grad_params,
                                         float* grad_geom, int E) {
  EmuScene* s = static_cast<EmuScene*>(scene);
  if (!grad_geom) return g_err = "grad_geom is null", -1;
  if ((s->fnset & cxk::FNS_CIRCLE_POLY) && s->s.gjk_steps > cx::CP_GJK_MAX)
    return g_err = "differentiable rollout: circle x polygon gradients record every GJK point: gjk_max_steps <= 32", -1;
  if ((stages & COTIX_STAGE_LUNAR) && !(s->fnset & ~1))
    return g_err = "differentiable rollout: the LunarLander joint stage needs the polygon program", -1;
  if (s->s.epar != 0 && (!geom || gstride == 0))
    return g_err = "grad_geom of a per-env scene needs geom with a geom_stride (one row per env)", -1;
  cxk::KArgs a{};
  a.sc = &s->s;
  a.geom = geom;
  a.gstride = gstride;
  a.B = B;
  a.n_steps = n_steps;
  a.dt = dt;
  a.stages = stages & ~COTIX_STAGE_BROADPHASE;
  a.action = action;
  a.action_body = action_body;
  a.save_dyn = const_cast<float*>(saved_dyn);
  a.save_keys = const_cast<uint32_t*>(saved_keys);
  a.tape = const_cast<uint32_t*>(tape);
  a.tw = emu_rollout_tape_words(scene);
  a.grad_action = grad_action;
  a.grad_dyn = grad_dyn0;
  a.grad_params = grad_params;
  a.grad_geom = grad_geom;
  for (int k = 0; k < s->s.nb * 6; ++k) a.ret_w[k] = ret_w[k];
  if (E == 1) run_blocks_gg<1>(a, tape != nullptr);
  else if (E == 4) run_blocks_gg<4>(a, tape != nullptr);
  else if (E == 8) run_blocks_gg<8>(a, tape != nullptr);
  else run_blocks_gg<2>(a, tape != nullptr);
  return 0;
}

// emu_launch_plan for a backward launch that asks for grad_geom (and
// grad_params): the same 14 words
extern "C" int emu_launch_plan_geom(void* scene, int envs_per_wave, int specialize, int mode, int B, int n_steps,
                                    int stages, int grad_params, int grad_geom, int cus, int split_bwd_on, long* out) {
  const EmuScene* s = static_cast<EmuScene*>(scene);
  static uint32_t tape;  // (never read: the plan looks at the pointers only)
  static float gp, gg;
  cxk::KArgs a{};
  a.B = B;
  a.n_steps = n_steps;
  a.stages = stages & ~COTIX_STAGE_BROADPHASE;
  a.tape = mode == 4 ? &tape : nullptr;
  a.grad_params = grad_params ? &gp : nullptr;
  a.grad_geom = grad_geom ? &gg : nullptr;
  const cxl::LaunchPlan p = cxl::plan_launch(s->s, s->fnset, {envs_per_wave, specialize}, a, mode,
                                             cxl::Device{cus, true, split_bwd_on != 0});
  const bool listed = p.family == cxl::FAM_STEP    ? cxl::compiled(p.ew, cxl::step_key(p))
                      : p.family == cxl::FAM_SPLIT ? cxl::compiled(p.ew, cxl::split_key(p))
                                                   : cxl::compiled(p.ew, cxl::help_key(p));
  const long v[] = {p.family, p.ew,    p.wpb,  p.fnset,     p.mode,      p.spec,      p.gp,
                    p.sdefer, p.nb,    p.grid, p.block, (long)p.lds, p.error != nullptr, listed};
  for (int k = 0; k < 14; ++k) out[k] = v[k];
  return 14;
}
