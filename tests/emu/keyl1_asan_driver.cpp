// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// host emulation's step program with the level-1 key ring
// (cotix_emu_keyl1.cpp emu_step_keyl1).
// usage: keyl1_asan_driver IN OUT.  IN: int32 header nb np B T stages G
// gstride mode E action_body, the scene, the geometry, the state (also the
// restart state), the keys, the actions [T][B][2].
// OUT: dyn, keys, err, resets, chosen, cells after one launch of T steps, in
// exactly sized buffers; the barrier counts are checked inside (exit 5).
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int emu_scene_create(int, const float*, int, const int*, const int*, const int*, void**);
int emu_step_keyl1(void*, float*, uint32_t*, uint32_t*, const float*, int, int, int, float, int, const float*, int,
                   const float*, uint32_t*, int32_t*, int32_t*);
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> h;
  if (!rd(f, h, 10)) return 3;
  const int nb = h[0], np = h[1], B = h[2], T = h[3], stages = h[4], G = h[5], gs = h[6], ab = h[9];
  std::vector<float> par, geom, dyn, act;
  std::vector<int32_t> pb, pt, pn;
  std::vector<uint32_t> keys;
  if (!rd(f, par, nb * 4) || !rd(f, pb, np) || !rd(f, pt, np) || !rd(f, pn, np)) return 3;
  if (!rd(f, geom, gs ? (size_t)B * gs : (size_t)G) || !rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, keys, 2 * (size_t)B))
    return 3;
  if (!rd(f, act, (size_t)T * B * 2)) return 3;
  fclose(f);
  void* sc = nullptr;
  if (emu_scene_create(nb, par.data(), np, pb.data(), pt.data(), pn.data(), &sc)) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 4;
  }
  const std::vector<float> reset = dyn;
  std::vector<uint32_t> err(B, 0u), resets(B, 0u);
  std::vector<int32_t> chosen((size_t)T * nb * B, -7), cells((size_t)T * nb * nb * B, -7);
  if (emu_step_keyl1(sc, dyn.data(), keys.data(), err.data(), geom.data(), gs, B, T, 1e-2f, stages, act.data(), ab,
                     reset.data(), resets.data(), chosen.data(), cells.data())) {
    fprintf(stderr, "%s\n", emu_last_error());
    return 5;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, dyn);
  wr(o, keys);
  wr(o, err);
  wr(o, resets);
  wr(o, chosen);
  wr(o, cells);
  fclose(o);
  emu_scene_destroy(sc);
  return 0;
}
