// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// host emulation's backward with the shape geometry's gradient
// (cotix_emu_gradg.cpp emu_rollout_backward_geom).
// usage: gradg_asan_driver IN OUT.  IN: asan_driver.cpp's mode-1 input
// (int32 header nb np B T stages G gstride mode E action_body, the scene, the
// geometry, the state, the keys, the actions, the return weights).
// OUT: ret, grad_action, grad_dyn0, grad_geom of the backward from the
// forward's tape; the re-play backward must give the same bits (exit 6),
// grad_action / grad_dyn0 those of the backward without grad_geom (exit 7), and
// the backward that also asks for grad_params the same grad_geom (exit 8).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int emu_scene_create(int, const float*, int, const int*, const int*, const int*, void**);
int emu_rollout_tape_words(void*);
int emu_rollout(void*, float*, uint32_t*, uint32_t*, const float*, int, int, int, float, int, const float*, int,
                const float*, float*, float*, uint32_t*, uint32_t*, int);
int emu_rollout_backward(void*, const float*, const uint32_t*, const uint32_t*, const float*, int, int, int, float, int,
                         const float*, int, const float*, float*, float*, int);
int emu_rollout_backward_geom(void*, const float*, const uint32_t*, const uint32_t*, const float*, int, int, int,
                              float, int, const float*, int, const float*, float*, float*, float*, float*, int);
int emu_geom_part_words(void*);
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
// bit for bit, NaN where the other has NaN (payloads aside)
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
  if (!rd(f, h, 10)) return 3;
  const int nb = h[0], np = h[1], B = h[2], T = h[3], stages = h[4], G = h[5], gs = h[6], E = h[8], ab = h[9];
  std::vector<float> par, geom, dyn, act, rw;
  std::vector<int32_t> pb, pt, pn;
  std::vector<uint32_t> keys;
  if (!rd(f, par, nb * 4) || !rd(f, pb, np) || !rd(f, pt, np) || !rd(f, pn, np)) return 3;
  if (!rd(f, geom, gs ? (size_t)B * gs : (size_t)G) || !rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, keys, 2 * (size_t)B))
    return 3;
  if (!rd(f, act, (size_t)T * B * 2) || !rd(f, rw, nb * 6)) return 3;
  fclose(f);
  void* sc = nullptr;
  if (emu_scene_create(nb, par.data(), np, pb.data(), pt.data(), pn.data(), &sc)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 4;
  }
  std::vector<uint32_t> err(B, 0u);
  const size_t B4 = (size_t)(B + 3) / 4 * 4;  // saved rows in env blocks of 4 (cxk::row_at)
  std::vector<float> ret(B, 0.0f), sd((size_t)T * nb * 6 * B4);
  std::vector<uint32_t> sk((size_t)T * B * 2), tape((size_t)T * emu_rollout_tape_words(sc) * B4, 0x7FBADBADu);
  emu_rollout(sc, dyn.data(), keys.data(), err.data(), geom.data(), gs, B, T, 1e-2f, stages, act.data(), ab, rw.data(),
              ret.data(), sd.data(), sk.data(), tape.data(), E);
  // exactly sized outputs (an access past grad_geom's GW * B words is the sanitizer's to find)
  const size_t na = (size_t)T * B * 2, nd = (size_t)nb * 6 * B, npar = (size_t)nb * 4 * B,
               ng = (size_t)emu_geom_part_words(sc) * B;
  std::vector<float> ga(na), gd(nd), gg(ng, -7.0f), ra(na), rd_(nd), rg(ng, -7.0f), pa(na), pd(nd), qa(na), qd(nd),
      qp(npar, -7.0f), qg(ng, -7.0f);
  if (emu_rollout_backward_geom(sc, sd.data(), sk.data(), tape.data(), geom.data(), gs, B, T, 1e-2f, stages, act.data(),
                                ab, rw.data(), ga.data(), gd.data(), nullptr, gg.data(), E) ||
      emu_rollout_backward_geom(sc, sd.data(), sk.data(), nullptr, geom.data(), gs, B, T, 1e-2f, stages, act.data(), ab,
                                rw.data(), ra.data(), rd_.data(), nullptr, rg.data(), E) ||
      emu_rollout_backward_geom(sc, sd.data(), sk.data(), tape.data(), geom.data(), gs, B, T, 1e-2f, stages, act.data(),
                                ab, rw.data(), qa.data(), qd.data(), qp.data(), qg.data(), E) ||
      emu_rollout_backward(sc, sd.data(), sk.data(), tape.data(), geom.data(), gs, B, T, 1e-2f, stages, act.data(), ab,
                           rw.data(), pa.data(), pd.data(), E)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 5;
  }
  if (!same(ga, ra) || !same(gd, rd_) || !same(gg, rg)) {
    fprintf(stderr, "tape backward != re-play backward\n");
    return 6;
  }
  if (!same(ga, pa) || !same(gd, pd)) {
    fprintf(stderr, "grad_action / grad_dyn0 change with grad_geom\n");
    return 7;
  }
  if (!same(gg, qg) || !same(ga, qa) || !same(gd, qd)) {
    fprintf(stderr, "grad_geom changes with grad_params\n");
    return 8;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, ret);
  wr(o, ga);
  wr(o, gd);
  wr(o, gg);
  fclose(o);
  emu_scene_destroy(sc);
  return 0;
}
