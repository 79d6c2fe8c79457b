// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// range-sensor gradients' host checker (cotix_raygrad_host.cpp raygrad_host).
// usage: raygrad_asan_driver IN OUT.  IN: int32 header np nb B G gstride R
// sensor_body follow_angle ignore_mask gw want_dyn want_geom, the part table
// (body, kind, nv, goff: np each), sensor f32 [3] (ox, oy, max_range), dirs f32
// [R][2], dyn f32 [nb][6][B], the geometry (G words, or B rows of gstride),
// g_dist f32 [B][R].  OUT: g_dyn f32 [nb][6][B] when want_dyn, then g_geom f32
// [gw][B] when want_geom, from exactly sized buffers.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int raygrad_host(int, const int*, const int*, const int*, const int*, const float*, const float*, int, int,
                            const float*, int, int, unsigned, const float*, int, int, int, const float*, float*,
                            float*);

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> h, body, kind, nv, goff;
  if (!rd(f, h, 12)) return 3;
  const int np = h[0], nb = h[1], B = h[2], G = h[3], gs = h[4], R = h[5], gw = h[9];
  if (np < 0 || nb < 0 || B <= 0 || G < 0 || gs < 0 || R <= 0 || gw < 0 || (!h[10] && !h[11])) return 3;
  std::vector<float> sensor, dirs, dyn, geom, gdist;
  if (!rd(f, body, np) || !rd(f, kind, np) || !rd(f, nv, np) || !rd(f, goff, np) || !rd(f, sensor, 3)) return 3;
  if (!rd(f, dirs, 2 * (size_t)R) || !rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, geom, gs ? (size_t)B * gs : (size_t)G) ||
      !rd(f, gdist, (size_t)B * R))
    return 3;
  fclose(f);
  std::vector<float> g_dyn(h[10] ? (size_t)nb * 6 * B : 0), g_geom(h[11] ? (size_t)gw * B : 0);
  if (raygrad_host(np, body.data(), kind.data(), nv.data(), goff.data(), dyn.data(), geom.data(), gs, B, sensor.data(),
                   h[6], h[7], (unsigned)h[8], dirs.data(), R, nb, gw, gdist.data(), h[10] ? g_dyn.data() : nullptr,
                   h[11] ? g_geom.data() : nullptr))
    return 5;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  if (!g_dyn.empty()) fwrite(g_dyn.data(), sizeof(float), g_dyn.size(), o);
  if (!g_geom.empty()) fwrite(g_geom.data(), sizeof(float), g_geom.size(), o);
  fclose(o);
  return 0;
}
