// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// rasterizer's host checker (cotix_raster_host.cpp raster_host).
// usage: raster_asan_driver IN OUT.  IN: int32 header np nb B G gstride W H
// channels follow_body follow_angle, the part table (body, kind, nv, goff:
// np each), cam f32 [4], dyn f32 [nb][6][B], the geometry (G words, or B rows
// of gstride), the palette (3 * (nb + 1) bytes when channels == 3).
// OUT: the image, from an exactly sized buffer.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int raster_host(int, const int*, const int*, const int*, const int*, const float*, const float*, int, int,
                           const float*, int, int, int, int, int, const unsigned char*, unsigned char*);

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
  const int np = h[0], nb = h[1], B = h[2], G = h[3], gs = h[4], W = h[5], H = h[6], ch = h[7];
  if (np < 0 || nb < 0 || B <= 0 || G < 0 || gs < 0 || W <= 0 || H <= 0 || (ch != 1 && ch != 3)) return 3;
  std::vector<float> cam, dyn, geom;
  std::vector<unsigned char> pal;
  if (!rd(f, body, np) || !rd(f, kind, np) || !rd(f, nv, np) || !rd(f, goff, np) || !rd(f, cam, 4)) return 3;
  if (!rd(f, dyn, (size_t)nb * 6 * B) || !rd(f, geom, gs ? (size_t)B * gs : (size_t)G)) return 3;
  if (ch == 3 && !rd(f, pal, 3 * (size_t)(nb + 1))) return 3;
  fclose(f);
  std::vector<unsigned char> image((size_t)B * ch * W * H);
  if (raster_host(np, body.data(), kind.data(), nv.data(), goff.data(), dyn.data(), geom.data(), gs, B, cam.data(),
                  h[8], h[9], W, H, ch, ch == 3 ? pal.data() : nullptr, image.data()))
    return 5;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(image.data(), 1, image.size(), o);
  fclose(o);
  return 0;
}
