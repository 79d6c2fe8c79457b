// cotix_plan.h -- which instantiation of the fused kernel a launch runs.
//
// Host only (no HIP runtime: the library's launcher, the kernel translation
// units and the host emulation all include it).  Two things live here and
// nowhere else:
//   the kernel list: what cotix_step_kernel.hip compiles for each
//     envs-per-wave tiling EW -- the translation unit instantiates exactly
//     these entries and launches by looking a key up in them;
//   the plan: plan_launch(), a pure function from a scene, its variant, the
//     launch's arguments and the device to the kernel (family and key), its
//     grid, block and LDS bytes.  A specialization or a two-wave form is used
//     if and only if its kernel is in the list, else the plan falls back.
#pragma once
#include <algorithm>
#include <cstddef>

#include "cotix_kernel.h"

namespace cxl {
// waves per workgroup: WPB (one per SIMD of a CU) -- or, for a scene whose
// tiles do not fit the LDS four at a time, 2 or 1 (each wave still owns its
// own tile, so the bits do not depend on it)
constexpr int WPB = 4;
// the hardware's LDS per CU
constexpr size_t LDS_CAP = 160 * 1024;

// ---------------------------------------------------------------------------
// the kernel list.  ews: the tilings an entry is compiled for, as the sum of
// their EW (1, 2, 4, 8 are their own bits)
// ---------------------------------------------------------------------------
struct StepKey {  // step_kernel<EW, fnset, mode, spec, gp>
  int fnset, mode, spec;
  int gp;  // the backward's gradient level: 0 none, 1 the body parameters, 2 the shape geometry (cxk::gpar_on)
  int ews;
};
struct HelpKey {  // step_help_kernel<fnset, spec, sdefer, l1>
  int fnset, spec;
  bool sdefer, l1;
  int ews;
};
struct SplitKey {  // bwd_split_kernel<nb, spec>
  int nb, spec;
  int ews;
};
constexpr int F_AN = cxk::FNS_ANALYTIC, F_PP = F_AN | cxk::FNS_CONVEX, F_AP = F_PP | cxk::FNS_AABB_POLY,
              F_ALL = F_AP | cxk::FNS_CIRCLE_POLY;
constexpr int EW_ALL = 1 | 2 | 4 | 8;
constexpr StepKey STEP_KERNELS[] = {
    // generic, every tiling: the step program per contact-function set, the
    // other programs (1 rollout forward, 2 backward re-play, 3 eval with a
    // judge / control, 4 tape backward; 5 / 6 below) analytic or full
    {F_AN, 0, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_PP, 0, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_AP, 0, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 0, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_AN, 1, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 1, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_AN, 2, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 2, cxk::SPEC_GENERIC, 0, EW_ALL},  // polygon scenes (the host rejects circle x polygon contacts)
    {F_AN, 3, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 3, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_AN, 4, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 4, cxk::SPEC_GENERIC, 0, EW_ALL},
    // the backward with the body parameters' gradient (KArgs::grad_params)
    {F_AN, 2, cxk::SPEC_GENERIC, 1, EW_ALL},
    {F_ALL, 2, cxk::SPEC_GENERIC, 1, EW_ALL},
    {F_AN, 4, cxk::SPEC_GENERIC, 1, EW_ALL},
    {F_ALL, 4, cxk::SPEC_GENERIC, 1, EW_ALL},
    // the backward with the shape geometry's gradient (KArgs::grad_geom; with
    // the parameters' where both are asked for).  Generic only: the analytic
    // scenes' register chain is selected by the body count inside phase G
    // 
    {F_AN, 2, cxk::SPEC_GENERIC, 2, EW_ALL},
    {F_ALL, 2, cxk::SPEC_GENERIC, 2, EW_ALL},
    {F_AN, 4, cxk::SPEC_GENERIC, 2, EW_ALL},
    {F_ALL, 4, cxk::SPEC_GENERIC, 2, EW_ALL},
    // the differentiable eval: the eval that also saves (5) and its tape backward (6)
    {F_AN, 5, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 5, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_AN, 6, cxk::SPEC_GENERIC, 0, EW_ALL},
    {F_ALL, 6, cxk::SPEC_GENERIC, 0, EW_ALL},
    // the reference scenes' step programs at 4 and 2 envs per wave, either PRNG layout
    {F_AN, 0, cxk::SPEC_ROBOCUP, 0, 2 | 4},
    {F_AN, 0, cxk::SPEC_ROBOCUP_PART, 0, 2 | 4},
    {F_PP, 0, cxk::SPEC_LUNAR, 0, 2 | 4},
    {F_PP, 0, cxk::SPEC_LUNAR_PART, 0, 2 | 4},
    // the default tiling: RoboCup's other programs (the re-play backward,
    // mode 2, is the tape backward's check: generic only) ...
    {F_AN, 1, cxk::SPEC_ROBOCUP, 0, 4},
    {F_AN, 3, cxk::SPEC_ROBOCUP, 0, 4},
    {F_AN, 4, cxk::SPEC_ROBOCUP, 0, 4},
    // ... the box world's step and rollout programs (finite_scene, grad_box) ...
    {F_AN, 0, cxk::SPEC_BOX, 0, 4},
    {F_AN, 1, cxk::SPEC_BOX, 0, 4},
    {F_AN, 4, cxk::SPEC_BOX, 0, 4},
    // ... and their tape backward with the body parameters' gradient
    {F_AN, 4, cxk::SPEC_ROBOCUP, 1, 4},
    {F_AN, 4, cxk::SPEC_BOX, 1, 4},
    // ... and their differentiable eval
    {F_AN, 5, cxk::SPEC_ROBOCUP, 0, 4},
    {F_AN, 6, cxk::SPEC_ROBOCUP, 0, 4},
    {F_AN, 5, cxk::SPEC_BOX, 0, 4},
    {F_AN, 6, cxk::SPEC_BOX, 0, 4},
};
// the step program with a key-window helper wave per env group, without and
// with the level-1 key ring: RoboCup's specialization
constexpr HelpKey HELP_KERNELS[] = {
    {F_AN, cxk::SPEC_ROBOCUP, true, false, 4},
    {F_AN, cxk::SPEC_ROBOCUP, true, true, 4},
};
// the tape backward at two waves per env group.  The specializations only:
// with the header's dimensions as run-time values the two roles' registers
// exceed 256 VGPRs and spill (the generic scenes keep mode 4).  The box
// world's split form is emulation-tested but not compiled: measured slower
// than its one-wave mode 4, 0.55 against 0.42 ms per 64-step backward (DESIGN
// section 13)
constexpr SplitKey SPLIT_KERNELS[] = {
    {5, cxk::SPEC_ROBOCUP, 4},
};

constexpr bool same_kernel(const StepKey& a, const StepKey& b) {
  return a.fnset == b.fnset && a.mode == b.mode && a.spec == b.spec && a.gp == b.gp;
}
constexpr bool same_kernel(const HelpKey& a, const HelpKey& b) {
  return a.fnset == b.fnset && a.spec == b.spec && a.sdefer == b.sdefer && a.l1 == b.l1;
}
constexpr bool same_kernel(const SplitKey& a, const SplitKey& b) { return a.nb == b.nb && a.spec == b.spec; }
// the key's index in its list where it is compiled for `ew`, else -1 (the
// key's own ews is not read)
template <class K, size_t N>
constexpr int kernel_index(const K (&list)[N], int ew, const K& k) {
  for (size_t i = 0; i < N; ++i)
    if ((list[i].ews & ew) != 0 && same_kernel(list[i], k)) return (int)i;
  return -1;
}
constexpr bool compiled(int ew, const StepKey& k) { return kernel_index(STEP_KERNELS, ew, k) >= 0; }
constexpr bool compiled(int ew, const HelpKey& k) { return kernel_index(HELP_KERNELS, ew, k) >= 0; }
constexpr bool compiled(int ew, const SplitKey& k) { return kernel_index(SPLIT_KERNELS, ew, k) >= 0; }

// ---------------------------------------------------------------------------
// tilings
// ---------------------------------------------------------------------------
// waves per workgroup of a tiling: WPB, or for a scene whose tiles do not fit
// four at a time 2, then 1 -- a workgroup of one wave holds one tile and the
// tables; 0: not even that fits (the scene's hard cap)
inline int scene_wpb(const cxk::SceneHdr& s, int ew) {
  for (int w : {WPB, 2, 1})
    if (cxk::lds_bytes(s, w, ew) <= LDS_CAP) return w;
  return 0;
}
// the default tiling of a scene: 4 envs per wave (the measured best), else
// the largest of 2, 1 whose workgroup of WPB waves fits the LDS, else one env
// per wave in workgroups of 2 or 1 waves; 0: none fits
inline int lds_default_ew(const cxk::SceneHdr& s) {
#ifdef COTIX_EW4_ONLY
  return cxk::lds_bytes(s, WPB, 4) <= LDS_CAP ? 4 : 0;
#else
  for (int ew : {4, 2, 1})
    if (cxk::lds_bytes(s, WPB, ew) <= LDS_CAP) return ew;
  return scene_wpb(s, 1) ? 1 : 0;
#endif
}

// ---------------------------------------------------------------------------
// what a wave program admits (the host emulation runs the two-wave forms on
// every scene these admit, also where the library launches another kernel)
// ---------------------------------------------------------------------------
// the step program with a key helper: 4 envs per wave, the analytic program,
// more than one key window (cxk::KeyHelper)
inline bool key_helper_may_run(int fnset, int ew, int n_steps) {
  return ew == 4 && n_steps > cxk::KWIN && cxk::launch_fnset(fnset, 0) == cxk::FNS_ANALYTIC;
}
// the tape backward at two waves per env group (cxk::run_backward_split)
inline bool split_bwd_may_run(const cxk::SceneHdr& s, int fnset, int ew, const cxk::KArgs& a) {
  return a.tape != nullptr && ew == 4 && cxk::launch_fnset(fnset, 4) == cxk::FNS_ANALYTIC &&
         cxk::split_bwd_ok<4>(a, cxk::make_ctx<4>(s));
}

// ---------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------
// the kernel family; the step families' values are cotix_scene_last_step_form's
enum : int { FAM_STEP = 0, FAM_HELP = 1, FAM_HELP_L1 = 2, FAM_SPLIT = 3 };
struct Variant {  // cotix_scene_set_variant
  int envs_per_wave, specialize;
};
struct Device {
  int cus;             // compute units (0: unknown)
  bool key_helper_on;  // COTIX_KEY_HELPER
  bool split_bwd_on;   // COTIX_SPLIT_BWD
};
struct LaunchPlan {
  int family, ew, wpb;
  // the key: fnset, mode, spec, gp of step_kernel; fnset, spec, sdefer of the
  // helper forms (l1: the family); nb, spec of bwd_split_kernel
  int fnset, mode, spec, nb;
  int gp;  // StepKey::gp
  bool sdefer;
  unsigned grid, block;
  size_t lds;
  const char* error;  // the launch cannot run (nullptr: it can)
};
constexpr StepKey step_key(const LaunchPlan& p) { return {p.fnset, p.mode, p.spec, p.gp, 0}; }
constexpr HelpKey help_key(const LaunchPlan& p) { return {p.fnset, p.spec, p.sdefer, p.family == FAM_HELP_L1, 0}; }
constexpr SplitKey split_key(const LaunchPlan& p) { return {p.nb, p.spec, 0}; }

// sc: the scene's header and tables; fnset: its contact-function mask; a: the
// launch's arguments (sc / sh are not read); mode 0 step, 1 rollout forward,
// 2 backward re-play, 3 eval with a judge / control, 4 tape backward, 5 the
// eval that also saves, 6 its tape backward (one wave per env group: the
// split form does not carry the control's gradient)
inline LaunchPlan plan_launch(const cxk::SceneDev& sc, int fnset, Variant v, const cxk::KArgs& a, int mode,
                              Device dev) {
  LaunchPlan p{};
  p.ew = v.envs_per_wave;
  p.wpb = scene_wpb(sc, p.ew);
  if (p.wpb == 0) {  // (checked at create / set_variant)
    p.error = "scene too large for the LDS tile";
    return p;
  }
  p.fnset = cxk::launch_fnset(fnset, mode);  // the contact-function program for this scene
  p.mode = mode;
  p.nb = sc.nb;
  p.gp = a.grad_geom != nullptr ? 2 : a.grad_params != nullptr ? 1 : 0;
  // scene specialization (compile-time dimensions; reference scenes, whose
  // tiles always fit WPB to a workgroup)
  const int spec = v.specialize && p.wpb == WPB ? cxk::spec_of(sc) : cxk::SPEC_GENERIC;
  p.spec = spec;
  // the two-wave forms: workgroups of 2 * WPB waves over WPB env groups of 4
  p.grid = (unsigned)((a.B + WPB * 4 - 1) / (WPB * 4));
  p.block = 2 * WPB * 64;
  // the tape backward at two waves per env group where the scene allows it
  // and two tiles per group fit (the same bits).  A launch that asks for the
  // body parameters' or the shape geometry's gradient runs the one-wave mode 4
  // (the consumer chain does not carry them)
  if (mode == 4 && dev.split_bwd_on && p.gp == 0 && p.wpb == WPB && split_bwd_may_run(sc, fnset, p.ew, a) &&
      cxk::lds_bytes(sc, 2 * WPB, 4) <= LDS_CAP && compiled(4, split_key(p))) {
    p.family = FAM_SPLIT;
    p.lds = cxk::lds_bytes(sc, 2 * WPB, 4);
    return p;
  }
  // the step program with a key-window helper wave per env group where the
  // launch has more than one key window (the same bits)
  if (mode == 0 && dev.key_helper_on && p.wpb == WPB && key_helper_may_run(fnset, p.ew, a.n_steps) &&
      cxk::help_lds_bytes<4>(sc, WPB) <= LDS_CAP) {
    // with the level-1 key ring (cxk::KeyL1) where the scan is the fused one
    // that reads it, the ring fits, and its LDS costs the launch no residency:
    // a CU holds two of these workgroups by its registers (__launch_bounds__
    // of 512 threads) and LDS_CAP / lds by its LDS, and the launch needs no
    // more than its workgroups over the CUs
    const size_t lds0 = cxk::help_lds_bytes<4>(sc, WPB);
    // (and the speculative draw ring: the L1 kernels carry both)
    const size_t lds1 = cxk::help_l1_lds_bytes<4>(sc, WPB, cxk::key_l1_keys(sc, sc.hot), true);
    const cxk::Ctx c4 = cxk::make_ctx<4>(sc);
    const int need = dev.cus > 0 ? ((int)p.grid + dev.cus - 1) / dev.cus : 2;
    const int res0 = std::min<int>(2, (int)(LDS_CAP / lds0)), res1 = std::min<int>(2, (int)(LDS_CAP / lds1));
    const bool l1 = (a.stages & COTIX_STAGE_COLLIDER) && c4.nl > 0 && cxk::scan_fused<4>(c4) && lds1 <= LDS_CAP &&
                    res1 >= std::min(res0, need);
    // run_wave's SDEFER, as step_kernel's mode 0 has it for these scenes
    p.sdefer = spec == cxk::SPEC_ROBOCUP || spec == cxk::SPEC_ROBOCUP_PART;
    p.family = l1 ? FAM_HELP_L1 : FAM_HELP;
    if (compiled(4, help_key(p))) {
      p.lds = l1 ? lds1 : lds0;
      return p;
    }
    p.sdefer = false;
  }
  // step_kernel: the scene's specialization where this program of it is
  // compiled for this tiling, else the generic kernel
  p.family = FAM_STEP;
  if (!compiled(p.ew, step_key(p))) p.spec = cxk::SPEC_GENERIC;
  if (!compiled(p.ew, step_key(p))) p.error = "no kernel is compiled for this launch";
  p.grid = (unsigned)((a.B + p.wpb * p.ew - 1) / (p.wpb * p.ew));
  p.block = p.wpb * 64;
  p.lds = cxk::lds_bytes(sc, p.wpb, p.ew);
  return p;
}
}  // namespace cxl
