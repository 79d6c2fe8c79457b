// cotix_step_kernel.hip -- the fused step kernel (gfx950) for ONE envs-per-wave
// tiling: compiled once per EW with -DCOTIX_EW=N (see cotix_launch.h), the
// instantiations cotix_plan.h lists for that EW; the phase programs live in
// cotix_kernel.h, design notes there and in DESIGN.md.
#include <hip/hip_runtime.h>

#include <array>
#include <utility>

#include "../../include/cotix_amd.h"
#include "cotix_device.h"
#include "cotix_kernel.h"
#include "cotix_launch.h"

#ifndef COTIX_EW
#error "compile with -DCOTIX_EW=1|2|4|8"
#endif

using cxk::SceneDev;

namespace {

// ---------------------------------------------------------------------------
// the fused step kernel: WPB independent waves per workgroup, EW envs per wave
// ---------------------------------------------------------------------------
using cxl::WPB;
#ifdef COTIX_PHASE_PROF
__device__ unsigned long long g_phase_cycles[cxk::PH_COUNT];
// per-wave timeline of the last launch (s_memrealtime, 100 MHz, chip-wide):
// entry, state loaded (before the workgroup barrier), after the barrier, end
// (after the stores completed) -- tools/k1_stamps.py
constexpr int STAMP_WAVES = 4096;
__device__ unsigned long long g_stamps[STAMP_WAVES * 4];
#define CXK_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memrealtime()
#else
#define CXK_STAMP(v) ((void)0)
#endif
// one phase on this lane, then wave-local ordering before the next phase.
// staged(ph, fetch, mid, finish): a phase of three stages whose per-lane
// state S passes from the first to the last in registers, every lane's
// stage before every lane's next (lockstep: nothing on the GPU, an order
// point of the host emulation's fibers); the emulation's HostRun is this
struct WaveRun {
  int lane;
  template <class S, class F1, class F2, class F3>
  __device__ __forceinline__ void staged(int ph, F1 fetch, F2 mid, F3 finish) const {
    (*this)(ph, [&](int l) {
      S s;
      fetch(l, s);
      cxk::lockstep();
      mid(l);
      cxk::lockstep();
      finish(l, s);
    });
  }
#ifdef COTIX_PHASE_PROF
  unsigned long long* acc;  // per-phase cycle accumulators (registers after inlining); set by every kernel
  __device__ __forceinline__ WaveRun(int l, unsigned long long* a) : lane(l), acc(a) {}
  template <class F>
  __device__ __forceinline__ void operator()(int ph, F f) const {
    const unsigned long long t0 = clock64();
    f(lane);
    cxk::wave_sync();
    acc[ph] += clock64() - t0;
  }
#elif defined(COTIX_ASM_MARKERS)  // tooling: phase markers in the ISA (tools/isa_phases.py)
  template <class F>
  __device__ __forceinline__ void operator()(int ph, F f) const {
    asm volatile(";#PHASE_BEGIN %0" ::"s"(ph));
    f(lane);
    cxk::wave_sync();
    asm volatile(";#PHASE_END %0" ::"s"(ph));
  }
#else
  // lockstep: the wave-uniform reads between phases precede the phase (a
  // no-op on the GPU, an order point of the host emulation's fibers)
  template <class F>
  __device__ __forceinline__ void operator()(int, F f) const {
    cxk::lockstep();
    f(lane);
    cxk::wave_sync();
  }
#endif
};
// a wave's phase runner and, in the phase-profile build, its per-phase cycle
// accumulators: flushed to g_phase_cycles by lane 0 of the waves that ran phases
#ifdef COTIX_PHASE_PROF
struct PhaseAcc {
  unsigned long long acc[cxk::PH_COUNT];
  __device__ __forceinline__ WaveRun run(int lane) {
    for (int q = 0; q < cxk::PH_COUNT; ++q) acc[q] = 0ull;
    return WaveRun{lane, acc};
  }
  __device__ __forceinline__ void flush(bool on) const {
    if (on)
      for (int q = 0; q < cxk::PH_COUNT; ++q) atomicAdd(&g_phase_cycles[q], acc[q]);
  }
};
#else
struct PhaseAcc {
  __device__ __forceinline__ WaveRun run(int lane) const { return WaveRun{lane}; }
  __device__ __forceinline__ void flush(bool) const {}
};
#endif
// MODE 0: step, 1: rollout forward (saves + return, + tape), 2: rollout
// backward re-playing the forward, 3: eval with the device judge / control
// (cotix_eval), 4: rollout backward from the forward's tape, 5: the eval
// that also saves (cotix_eval_rollout: run_wave ESAVE), 6: its tape backward
// (cotix_eval_backward: run_wave_backward_tape EV);
// SPEC: scene specialization (cxk::SPEC_*, compile-time dimensions);
// GP (MODE 2 and 4): the backward with the body parameters' gradient (1,
// KArgs::grad_params) or the shape geometry's (2, KArgs::grad_geom; with the
// parameters' where both are given) -- instantiations of their own, so a
// launch that does not ask for them runs the kernels it ran before
template <int EW, int FNSET, int MODE, int SPEC = cxk::SPEC_GENERIC, int GP = 0>
__global__ __launch_bounds__(WPB * 64) void step_kernel(cxk::KArgs a) {
  extern __shared__ uint32_t lds[];
  CXK_STAMP(st0);
  const SceneDev* sc = a.sc;
  const cxk::SceneHdr sh = cxk::spec_hdr<SPEC>(a.sh);  // a constant for SPEC > 0
  const int nhot = sh.nhot;
  // waves in this workgroup: WPB, or 2 / 1 for scenes whose tiles do not fit
  // four at a time (generic kernel only: the specializations are the
  // reference scenes, which fit, and keep their folded constants)
  const int nw = SPEC != cxk::SPEC_GENERIC ? WPB : (int)blockDim.x >> 6;
  constexpr int HC = 16;
  const int nt = nw * 64;
  for (int base = 0; base < nhot; base += HC * nt) {
    uint32_t r[HC];
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * nt + (int)threadIdx.x;
      r[k] = i < nhot ? sc->hot[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * nt + (int)threadIdx.x;
      if (i < nhot) lds[i] = r[k];
    }
  }
  const cxk::Ctx c = cxk::make_ctx<EW>(sh);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int env0 = (blockIdx.x * nw + wave) * EW;
  uint32_t* wbase = lds + nhot + wave * (c.L.S * EW + c.W.words);
  const cxk::Tile<EW> t{wbase, lds, wbase + c.L.S * EW};
  // the forward programs load the wave's state before the barrier: it writes
  // only the wave's own tile (disjoint from the tables), so its global reads
  // overlap the table copy's (a launch's fixed cost, K = 1 RL loops)
  if (MODE != 2 && MODE != 4 && MODE != 6 && env0 < a.B) {
    if (MODE == 3 || MODE == 5)
      cxk::ph_load_fwd<EW, false, true>(a, c, t, env0, lane);
    else
      cxk::ph_load_fwd<EW, MODE == 1>(a, c, t, env0, lane);
  }
#ifdef COTIX_PHASE_PROF
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
  CXK_STAMP(st1);
  __syncthreads();
  CXK_STAMP(st2);
  if (env0 >= a.B) return;  // whole wave idle (after the only workgroup barrier)
  PhaseAcc pa;
  const WaveRun run = pa.run(lane);
  if (MODE == 6)
    cxk::run_wave_backward_tape<EW, FNSET, 0, true>(a, c, t, env0, run);
  else if (MODE == 5)
    cxk::run_wave<EW, FNSET, false, true, false, true>(a, c, t, env0, run, true);
  else if (MODE == 4)
    cxk::run_wave_backward_tape<EW, FNSET, GP>(a, c, t, env0, run);
  else if (MODE == 2)
    cxk::run_wave_backward<EW, FNSET, GP>(a, c, t, env0, run);
  else if (MODE == 3)
    cxk::run_wave<EW, FNSET, false, true>(a, c, t, env0, run, true);
  else
    cxk::run_wave<EW, FNSET, MODE == 1, false,
                  MODE == 0 && (SPEC == cxk::SPEC_ROBOCUP || SPEC == cxk::SPEC_ROBOCUP_PART)>(a, c, t, env0, run, true);
  pa.flush(lane == 0);
#ifdef COTIX_PHASE_PROF
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  CXK_STAMP(st3);
  const int gw = (int)blockIdx.x * nw + wave;
  if (lane == 0 && gw < STAMP_WAVES) {
    g_stamps[4 * gw] = st0;
    g_stamps[4 * gw + 1] = st1;
    g_stamps[4 * gw + 2] = st2;
    g_stamps[4 * gw + 3] = st3;
  }
#endif
}

#if COTIX_EW == 4
// the tape backward at two waves per env group (cxk::run_backward_split):
// waves g and g + WPB of the workgroup are env group g's producer and
// consumer (one SIMD each pair), the group's two tiles are the LDS regions of
// those two waves.  The workgroup barrier waits for LDS only: the producer's
// prefetch reads (two steps ahead) and the consumer's gradient stores stay in
// flight across it.
CX_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int NB, int SPEC>
__global__ __launch_bounds__(2 * WPB * 64) void bwd_split_kernel(cxk::KArgs a) {
  constexpr int EW = 4;
  extern __shared__ uint32_t lds[];
  const SceneDev* sc = a.sc;
  const cxk::SceneHdr sh = cxk::spec_hdr<SPEC>(a.sh);
  const int nhot = sh.nhot;
  constexpr int HC = 8, NT = 2 * WPB * 64;
  for (int base = 0; base < nhot; base += HC * NT) {
    uint32_t r[HC];
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * NT + (int)threadIdx.x;
      r[k] = i < nhot ? sc->hot[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * NT + (int)threadIdx.x;
      if (i < nhot) lds[i] = r[k];
    }
  }
  const cxk::Ctx c = cxk::make_ctx<EW>(sh);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = wave % WPB, role = wave < WPB ? 1 : 2;
  const int env0 = (blockIdx.x * WPB + grp) * EW;
  // the group's two tiles are its two waves' regions; each wave keeps its own scratch
  const int rw = c.L.S * EW + c.W.words;
  uint32_t* r0 = lds + nhot + grp * rw;
  uint32_t* r1 = lds + nhot + (grp + WPB) * rw;
  uint32_t* ws = (role == 1 ? r0 : r1) + c.L.S * EW;
  const cxk::Tile<EW> t0{r0, lds, ws}, t1{r1, lds, ws};
  __syncthreads();
  PhaseAcc pa;
  const WaveRun run = pa.run(lane);
  cxk::run_backward_split<EW, NB>(a, c, t0, t1, env0, run, role, [] { lds_barrier(); });
  pa.flush(lane == 0 && env0 < a.B);
}
// the step program with a key-window helper wave per env group
// (cxk::KeyHelper): waves g < WPB step env group g, wave g + WPB computes its
// key windows; LDS: the tables, WPB wave regions (tile + scratch, stride rounded
// to a multiple of EW words), then WPB helper window buffers
struct GpuKeyHelp {
  static constexpr bool on = true;
  int kwalt;
  __device__ __forceinline__ void bar() const { lds_barrier(); }
};
// L1: the helper also fills the level-1 key ring (cxk::KeyL1): WPB rings
// follow the window buffers, and the workgroup passes cxk::key_l1_barriers
// spec: and the speculative draw words (cxk::scan_spec_fill): WPB draw rings
// follow the key rings
struct GpuKeyHelpL1 {
  static constexpr bool on = true;
  static constexpr bool l1 = true;
  static constexpr int spec = cxk::SCAN_M;
  int kwalt;
  int l1o;
  int spo;
  __device__ __forceinline__ void bar() const { lds_barrier(); }
};
template <int FNSET, int SPEC, bool SDEFER, bool L1 = false>
__global__ __launch_bounds__(2 * WPB * 64) void step_help_kernel(cxk::KArgs a) {
  constexpr int EW = 4;
  extern __shared__ uint32_t lds[];
  const SceneDev* sc = a.sc;
  const cxk::SceneHdr sh = cxk::spec_hdr<SPEC>(a.sh);
  const int nhot = sh.nhot;
  constexpr int HC = 8, NT = 2 * WPB * 64;
  for (int base = 0; base < nhot; base += HC * NT) {
    uint32_t r[HC];
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * NT + (int)threadIdx.x;
      r[k] = i < nhot ? sc->hot[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const int i = base + k * NT + (int)threadIdx.x;
      if (i < nhot) lds[i] = r[k];
    }
  }
  const cxk::Ctx c = cxk::make_ctx<EW>(sh);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = wave % WPB;
  const bool stepper = wave < WPB;
  const int env0 = (blockIdx.x * WPB + grp) * EW;
  const int rw = cxk::help_region_words<EW>(c), hw = cxk::KWIN * c.L.kww * EW;
  uint32_t* um = lds + nhot + grp * rw;
  uint32_t* hb = lds + nhot + WPB * rw + grp * hw;
  const cxk::Tile<EW> tm{um, lds, um + c.L.S * EW};
  if (stepper && env0 < a.B) cxk::ph_load_fwd<EW, false>(a, c, tm, env0, lane);
  __syncthreads();
  PhaseAcc pa;
  const WaveRun run = pa.run(lane);
  const int nbar = L1 ? cxk::key_l1_barriers(a) : cxk::keys_on(a) ? cxk::key_helper_windows(a) : 0;
  if (env0 >= a.B) {  // an idle wave keeps the barrier count
    for (int q = 0; q < nbar; ++q) lds_barrier();
    return;
  }
  if constexpr (L1) {
    const int nk1 = cxk::key_l1_keys(sh, lds);
    const int l1o = (int)(lds + nhot + WPB * (rw + hw) + grp * cxk::key_l1_ring_words<EW>(nk1) - um) / EW;
    const int spo = (int)(lds + nhot + WPB * (rw + hw + cxk::key_l1_ring_words<EW>(nk1)) +
                          grp * cxk::scan_spec_ring_words<EW>(sh) - um) / EW;
    if (stepper) {
      // the step wave's instructions issue ahead of its helper's on their
      // SIMD: the launch is the step waves' dependent chain (measured: 701.7
      // -> 706.8 M env-steps/s, profiles/key_l1_ab_*.json)
      __builtin_amdgcn_s_setprio(2);
      const GpuKeyHelpL1 help{(int)(hb - um) / EW - c.L.kw, l1o, spo};
      cxk::run_wave<EW, FNSET, false, false, SDEFER>(a, c, tm, env0, run, true, help);
    } else {
      cxk::KeyL1<EW> h;
      h.kh.tm = tm;
      h.kh.th = cxk::Tile<EW>{hb - c.L.kw * EW, lds, nullptr};
      h.kh.env0 = env0;
      h.l1o = l1o;
      h.nk1 = nk1;
      h.sm = cxk::SCAN_M;
      h.spo = spo;
      for (int q = 0; q < nbar; ++q) {
        cxk::key_l1_next<EW>(a, c, h, run);
        lds_barrier();
      }
    }
  } else if (stepper) {
    const GpuKeyHelp help{(int)(hb - um) / EW - c.L.kw};
    cxk::run_wave<EW, FNSET, false, false, SDEFER>(a, c, tm, env0, run, true, help);
  } else {
    cxk::KeyHelper<EW> h;
    h.tm = tm;
    h.th = cxk::Tile<EW>{hb - c.L.kw * EW, lds, nullptr};
    h.env0 = env0;
    if (nbar > 0) cxk::key_helper_init<EW>(a, c, h, run);
    for (int q = 0; q < nbar; ++q) {
      cxk::key_helper_next<EW>(a, c, h, run);
      lds_barrier();
    }
  }
  pa.flush(lane == 0 && stepper);  // the step waves' phases (the helper's K work overlaps them)
}
#endif

// ---------------------------------------------------------------------------
// the kernels of this tiling: one function pointer per entry of cotix_plan.h's
// lists (null where the entry is not compiled for this EW, and then not
// instantiated), in the lists' order
// ---------------------------------------------------------------------------
using KernelFn = void (*)(cxk::KArgs);
template <int EW, size_t I>
constexpr KernelFn step_fn() {
  constexpr cxl::StepKey k = cxl::STEP_KERNELS[I];
  if constexpr ((k.ews & EW) != 0)
    return &step_kernel<EW, k.fnset, k.mode, k.spec, k.gp>;
  else
    return nullptr;
}
template <int EW, size_t... I>
constexpr std::array<KernelFn, sizeof...(I)> step_fns(std::index_sequence<I...>) {
  return {step_fn<EW, I>()...};
}
#if COTIX_EW == 4
template <size_t... I>
constexpr std::array<KernelFn, sizeof...(I)> help_fns(std::index_sequence<I...>) {
  return {&step_help_kernel<cxl::HELP_KERNELS[I].fnset, cxl::HELP_KERNELS[I].spec, cxl::HELP_KERNELS[I].sdefer,
                            cxl::HELP_KERNELS[I].l1>...};
}
template <size_t... I>
constexpr std::array<KernelFn, sizeof...(I)> split_fns(std::index_sequence<I...>) {
  return {&bwd_split_kernel<cxl::SPLIT_KERNELS[I].nb, cxl::SPLIT_KERNELS[I].spec>...};
}
#endif
template <class K, size_t N>
KernelFn kernel_of(const K (&list)[N], const std::array<KernelFn, N>& fns, const K& key) {
  const int i = cxl::kernel_index(list, COTIX_EW, key);
  return i < 0 ? nullptr : fns[i];
}

}  // namespace

// the plan's kernel launched as planned; a key that is not in this tiling's
// table is an error (the plan has already fallen back)
#define CXL_NAME2(n) launch_ew##n
#define CXL_NAME(n) CXL_NAME2(n)
hipError_t cxl::CXL_NAME(COTIX_EW)(const cxl::LaunchPlan& p, const cxk::KArgs& ka, hipStream_t st) {
  static constexpr auto STEP = step_fns<COTIX_EW>(std::make_index_sequence<std::size(cxl::STEP_KERNELS)>{});
  KernelFn fn = nullptr;
  if (p.ew != COTIX_EW || p.error != nullptr) return hipErrorInvalidValue;
  if (p.family == cxl::FAM_STEP) fn = kernel_of(cxl::STEP_KERNELS, STEP, cxl::step_key(p));
#if COTIX_EW == 4
  static constexpr auto HELP = help_fns(std::make_index_sequence<std::size(cxl::HELP_KERNELS)>{});
  static constexpr auto SPLIT = split_fns(std::make_index_sequence<std::size(cxl::SPLIT_KERNELS)>{});
  if (p.family == cxl::FAM_HELP || p.family == cxl::FAM_HELP_L1)
    fn = kernel_of(cxl::HELP_KERNELS, HELP, cxl::help_key(p));
  if (p.family == cxl::FAM_SPLIT) fn = kernel_of(cxl::SPLIT_KERNELS, SPLIT, cxl::split_key(p));
#endif
  if (fn == nullptr) return hipErrorInvalidValue;
  cxk::KArgs a = ka;
  void* args[] = {&a};
  return hipLaunchKernel(reinterpret_cast<const void*>(fn), dim3(p.grid), dim3(p.block), args, p.lds, st);
}

#ifdef COTIX_PHASE_PROF
// profiling build only: per-phase cycles summed over waves since the last call (then reset)
extern "C" int cotix_phase_cycles(unsigned long long* out, int n) {
  unsigned long long h[cxk::PH_COUNT] = {};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase_cycles), sizeof(h)) != hipSuccess) return -1;
  unsigned long long z[cxk::PH_COUNT] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)) != hipSuccess) return -1;
  for (int q = 0; q < n && q < cxk::PH_COUNT; ++q) out[q] = h[q];
  // then the 8 sub-phase timers (CXK_SUB_T1)
  unsigned long long sub[8] = {};
  if (hipMemcpyFromSymbol(sub, HIP_SYMBOL(cxk::g_sub_cycles), sizeof(sub)) != hipSuccess) return -1;
  unsigned long long z8[8] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(cxk::g_sub_cycles), z8, sizeof(z8)) != hipSuccess) return -1;
  unsigned long long dsub[4] = {};  // GJK timer of cotix_device.h in slot 4
  if (hipMemcpyFromSymbol(dsub, HIP_SYMBOL(cx::g_dev_sub), sizeof(dsub)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(cx::g_dev_sub), z8, sizeof(dsub)) != hipSuccess) return -1;
  sub[4] = dsub[0];  // GJK
  sub[5] = dsub[1];  // EPA
  for (int q = 0; q < 8 && cxk::PH_COUNT + q < n; ++q) out[cxk::PH_COUNT + q] = sub[q];
  return cxk::PH_COUNT + 8 < n ? cxk::PH_COUNT + 8 : n;
}
// profiling build only: the last launch's per-wave timeline (g_stamps), n words
extern "C" int cotix_phase_stamps(unsigned long long* out, int n) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const int m = n < STAMP_WAVES * 4 ? n : STAMP_WAVES * 4;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * m) != hipSuccess) return -1;
  return m;
}
#endif
