// TEST INFRASTRUCTURE ONLY -- the host emulation of the differentiable eval
// (cotix_eval_rollout / cotix_eval_backward): the kernel's saving eval forward
// (cotix_kernel.h run_wave ESAVE) and its tape backward
// (run_wave_backward_tape EV) on the 64 fiber lanes of cotix_emu.cpp, whose
// entry points this library also carries.  Built with -DCOTIX_NO_GREGS it runs
// phase G's tile form on every scene.
#include "cotix_emu.cpp"

namespace {
template <int EW>
void run_blocks_ev(const cxk::KArgs& a, bool backward) {
  const cxk::SceneDev& sc = *a.sc;
  const cxk::Ctx c = cxk::make_ctx<EW>(sc);
  const int nwaves = (a.B + EW - 1) / EW;
  std::vector<uint32_t> lds((size_t)sc.nhot + (size_t)cxk::help_region_words<EW>(c));
  for (int q = 0; q < sc.nhot; ++q) lds[q] = sc.hot[q];
  const int F = cxk::launch_fnset(sc.fnset, backward ? 6 : 5);  // the plan's contact-function program
  for (int wv = 0; wv < nwaves; ++wv) {
    std::fill(lds.begin() + sc.nhot, lds.end(), 0x7FBADBADu);  // poison (a NaN pattern)
    const cxk::Tile<EW> t{lds.data() + sc.nhot, lds.data(), lds.data() + sc.nhot + (size_t)c.L.S * EW};
    const int env0 = wv * EW;
    cxk_simt::run([&](int lane) {
      const HostRun run{lane};
      if (backward)
        F == 1 ? cxk::run_wave_backward_tape<EW, 1, false, true>(a, c, t, env0, run)
               : cxk::run_wave_backward_tape<EW, 15, false, true>(a, c, t, env0, run);
      else
        F == 1 ? cxk::run_wave<EW, 1, false, true, false, true>(a, c, t, env0, run)
               : cxk::run_wave<EW, 15, false, true, false, true>(a, c, t, env0, run);
    });
  }
}
void run_ev(const cxk::KArgs& a, int E, bool backward) {
  if (E == 1) run_blocks_ev<1>(a, backward);
  else if (E == 4) run_blocks_ev<4>(a, backward);
  else if (E == 8) run_blocks_ev<8>(a, backward);
  else run_blocks_ev<2>(a, backward);
}
// the library's scene restrictions on a differentiable launch (cotix_step.hip)
int ev_scene_ok(const EmuScene* s, int stages) {
  if ((s->fnset & cxk::FNS_CIRCLE_POLY) && s->s.gjk_steps > cx::CP_GJK_MAX)
    return g_err = "differentiable eval: circle x polygon gradients record every GJK point: gjk_max_steps <= 32", -1;
  if ((stages & COTIX_STAGE_LUNAR) && !(s->fnset & ~1))
    return g_err = "differentiable eval: the LunarLander joint stage needs the polygon program", -1;
  return 0;
}
}  // namespace

// cotix_eval_rollout on the host
extern "C" int emu_eval_rollout(void* scene, float* dyn, uint32_t* keys, uint32_t* err, const float* geom, int gstride,
                                int B, int n_nfe, int wfe, float dt, int stages, const cotix_judge* judge,
                                const cotix_control* control, float* reward, uint32_t* finished, float* saved_dyn,
                                uint32_t* saved_keys, uint32_t* tape, uint32_t* judge_rec, int E) {
  EmuScene* s = static_cast<EmuScene*>(scene);
  if (!judge) return g_err = "the differentiable eval needs a judge", -1;
  if (!tape) return g_err = "the differentiable eval needs the tape", -1;
  if (!reward || !finished || !saved_dyn || !saved_keys || !judge_rec) return g_err = "null argument", -1;
  if (ev_scene_ok(s, stages)) return -1;
  if (B == 0 || n_nfe == 0 || wfe == 0) return 0;
  cxk::KArgs a{};
  const int nb = s->s.nb;
  if (cxk::pack_judge(judge, nb * 6, nb, a.judge, g_err) || cxk::pack_control(control, nb, a.ctl, g_err)) return -1;
  a.sc = &s->s;
  a.dyn = dyn;
  a.keys = keys;
  a.err = err;
  a.geom = geom;
  a.gstride = gstride;
  a.B = B;
  a.n_steps = n_nfe * wfe;
  a.nfe_len = wfe;
  a.dt = dt;
  a.stages = stages;
  a.reward = reward;
  a.finished = finished;
  a.save_dyn = saved_dyn;
  a.save_keys = saved_keys;
  a.tape = tape;
  a.tw = emu_rollout_tape_words(scene);
  a.judge_rec = judge_rec;
  run_ev(a, E, false);
  return 0;
}

// cotix_eval_backward on the host
extern "C" int emu_eval_backward(void* scene, const float* saved_dyn, const uint32_t* saved_keys, const uint32_t* tape,
                                 const uint32_t* judge_rec, const float* geom, int gstride, int B, int n_nfe, int wfe,
                                 float dt, int stages, const cotix_judge* judge, const cotix_control* control,
                                 float* grad_control, float* grad_dyn0, float* grad_dv, int E) {
  EmuScene* s = static_cast<EmuScene*>(scene);
  if (!judge) return g_err = "the differentiable eval needs a judge", -1;
  if (!tape) return g_err = "the differentiable eval needs the tape", -1;
  if (!saved_dyn || !saved_keys || !judge_rec) return g_err = "null argument", -1;
  if (grad_control && !control) return g_err = "grad_control needs the control", -1;
  if (ev_scene_ok(s, stages)) return -1;
  if (B == 0 || n_nfe == 0 || wfe == 0) return 0;
  cxk::KArgs a{};
  const int nb = s->s.nb;
  if (cxk::pack_judge(judge, nb * 6, nb, a.judge, g_err) || cxk::pack_control(control, nb, a.ctl, g_err)) return -1;
  a.sc = &s->s;
  a.geom = geom;
  a.gstride = gstride;
  a.B = B;
  a.n_steps = n_nfe * wfe;
  a.nfe_len = wfe;
  a.dt = dt;
  a.stages = stages & ~COTIX_STAGE_BROADPHASE;
  a.save_dyn = const_cast<float*>(saved_dyn);
  a.save_keys = const_cast<uint32_t*>(saved_keys);
  a.tape = const_cast<uint32_t*>(tape);
  a.tw = emu_rollout_tape_words(scene);
  a.judge_rec = const_cast<uint32_t*>(judge_rec);
  a.grad_control = grad_control;
  a.grad_dyn = grad_dyn0;
  a.grad_action = grad_dv;
  run_ev(a, E, true);
  return 0;
}
