// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// host emulation of the differentiable eval (cotix_emu_evalgrad.cpp
// emu_eval_rollout / emu_eval_backward).
// usage: evalgrad_asan_driver IN OUT.  IN: int32 header (nb np B n_nfe wfe
// stages G gstride E), f32 dt, the scene (body parameters, part body / type /
// vertex count), the geometry, the state, the keys, then the bytes of a
// cotix_judge and a cotix_control.  Every array the two entry points write is
// sized exactly (an access past it is the sanitizer's to find).
// OUT: dyn, keys, err, reward, finished, judge_rec, grad_control, grad_dyn0,
// grad_dv.  The forward must also equal emu_eval's bits (exit 6).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cotix_amd.h"

extern "C" {
int emu_scene_create(int, const float*, int, const int*, const int*, const int*, void**);
int emu_rollout_tape_words(void*);
int emu_eval(void*, float*, uint32_t*, uint32_t*, const float*, int, int, int, int, float, int, const cotix_judge*,
             const cotix_control*, const float*, int, float*, uint32_t*, int, const float*, uint32_t*, float*, int);
int emu_eval_rollout(void*, float*, uint32_t*, uint32_t*, const float*, int, int, int, int, float, int,
                     const cotix_judge*, const cotix_control*, float*, uint32_t*, float*, uint32_t*, uint32_t*,
                     uint32_t*, int);
int emu_eval_backward(void*, const float*, const uint32_t*, const uint32_t*, const uint32_t*, const float*, int, int,
                      int, int, float, int, const cotix_judge*, const cotix_control*, float*, float*, float*, int);
const char* emu_last_error(void);
int emu_scene_destroy(void*);
}

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
  fwrite(v.data(), sizeof(T), v.size(), f);
}
static bool same(const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k) {
    const bool na = a[k] != a[k], nb = b[k] != b[k];
    if (na != nb || (!na && memcmp(&a[k], &b[k], 4) != 0)) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> h;
  std::vector<float> dtv;
  if (!rd(f, h, 9) || !rd(f, dtv, 1)) return 3;
  const int nb = h[0], np = h[1], B = h[2], nfe = h[3], wfe = h[4], stages = h[5], G = h[6], gs = h[7], E = h[8];
  const float dt = dtv[0];
  const int T = nfe * wfe;
  std::vector<float> par, geom, dyn;
  std::vector<int32_t> pb, pt, pn;
  std::vector<uint32_t> keys;
  cotix_judge judge;
  cotix_control control;
  if (!rd(f, par, nb * 4) || !rd(f, pb, np) || !rd(f, pt, np) || !rd(f, pn, np)) return 3;
  if (!rd(f, geom, gs ? (size_t)B * gs : (size_t)G) || !rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, keys, 2 * (size_t)B))
    return 3;
  if (fread(&judge, sizeof(judge), 1, f) != 1 || fread(&control, sizeof(control), 1, f) != 1) return 3;
  fclose(f);
  void* sc = nullptr;
  if (emu_scene_create(nb, par.data(), np, pb.data(), pt.data(), pn.data(), &sc)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 4;
  }
  // the plain eval on a copy
  std::vector<float> d0 = dyn, r0(B, 0.0f);
  std::vector<uint32_t> k0 = keys, e0(B, 0u), f0(B, 0u);
  if (emu_eval(sc, d0.data(), k0.data(), e0.data(), geom.data(), gs, B, nfe, wfe, dt, stages, &judge, &control, nullptr,
               0, r0.data(), f0.data(), 0, nullptr, nullptr, nullptr, E)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 5;
  }
  const size_t B4 = (size_t)(B + 3) / 4 * 4;  // saved rows in env blocks of 4 (cxk::row_at)
  std::vector<uint32_t> err(B, 0u), fin(B, 0u), sk((size_t)T * B * 2),
      tape((size_t)T * emu_rollout_tape_words(sc) * B4, 0x7FBADBADu), rec((size_t)(T + 1) * B, 0xFFFFFFFFu);
  std::vector<float> rw(B, 0.0f), sd((size_t)T * nb * 6 * B4);
  if (emu_eval_rollout(sc, dyn.data(), keys.data(), err.data(), geom.data(), gs, B, nfe, wfe, dt, stages, &judge,
                       &control, rw.data(), fin.data(), sd.data(), sk.data(), tape.data(), rec.data(), E)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 5;
  }
  if (!same(dyn, d0) || keys != k0 || err != e0 || !same(rw, r0) || fin != f0) {
    fprintf(stderr, "saving eval forward != eval\n");
    return 6;
  }
  std::vector<float> gc((size_t)26 * B, -7.0f), gd((size_t)nb * 6 * B, -7.0f), gv((size_t)T * B * 2, -7.0f);
  if (emu_eval_backward(sc, sd.data(), sk.data(), tape.data(), rec.data(), geom.data(), gs, B, nfe, wfe, dt, stages,
                        &judge, &control, gc.data(), gd.data(), gv.data(), E)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 5;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, dyn);
  wr(o, keys);
  wr(o, err);
  wr(o, rw);
  wr(o, fin);
  wr(o, rec);
  wr(o, gc);
  wr(o, gd);
  wr(o, gv);
  fclose(o);
  emu_scene_destroy(sc);
  return 0;
}
