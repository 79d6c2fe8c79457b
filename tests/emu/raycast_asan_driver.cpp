// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// range sensor's host checker (cotix_raycast_host.cpp raycast_host).
// usage: raycast_asan_driver IN OUT.  IN: int32 header np nb B G gstride R
// sensor_body follow_angle ignore_mask want_hit, the part table (body, kind,
// nv, goff: np each), sensor f32 [3] (ox, oy, max_range), dirs f32 [R][2],
// dyn f32 [nb][6][B], the geometry (G words, or B rows of gstride).
// OUT: dist f32 [B][R], then hit u8 [B][R] when want_hit, from exactly sized buffers.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int raycast_host(int, const int*, const int*, const int*, const int*, const float*, const float*, int, int,
                            const float*, int, int, unsigned, const float*, int, float*, unsigned char*);

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
  if (!rd(f, h, 10)) return 3;
  const int np = h[0], nb = h[1], B = h[2], G = h[3], gs = h[4], R = h[5];
  if (np < 0 || nb < 0 || B <= 0 || G < 0 || gs < 0 || R <= 0) return 3;
  std::vector<float> sensor, dirs, dyn, geom;
  if (!rd(f, body, np) || !rd(f, kind, np) || !rd(f, nv, np) || !rd(f, goff, np) || !rd(f, sensor, 3)) return 3;
  if (!rd(f, dirs, 2 * (size_t)R) || !rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, geom, gs ? (size_t)B * gs : (size_t)G))
    return 3;
  fclose(f);
  std::vector<float> dist((size_t)B * R);
  std::vector<unsigned char> hit(h[9] ? (size_t)B * R : 0);
  if (raycast_host(np, body.data(), kind.data(), nv.data(), goff.data(), dyn.data(), geom.data(), gs, B, sensor.data(),
                   h[6], h[7], (unsigned)h[8], dirs.data(), R, dist.data(), h[9] ? hit.data() : nullptr))
    return 5;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(dist.data(), sizeof(float), dist.size(), o);
  if (!hit.empty()) fwrite(hit.data(), 1, hit.size(), o);
  fclose(o);
  return 0;
}
