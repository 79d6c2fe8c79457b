// TEST INFRASTRUCTURE ONLY: the host checker of cotix_rasterize -- a plain
// loop over envs and pixels around the per-part and per-pixel functions of
// parallax_amd/csrc/cotix_raster.h (the code the gfx950 kernel runs), built
// with the kernel's floating-point flags (tests/emu/raster.mk).
#include <vector>

#include "../../parallax_amd/csrc/cotix_raster.h"

// part table: body / kind (0 circle, 1 AABB, 2 polygon) / nv / goff per part,
// in draw order; dyn f32 [n_bodies][6][B]; geom shared (gstride 0) or one row
// per env; cam = (cx, cy, half_w, half_h); palette: 3 bytes per id (NULL: ids).
// image u8 [B][H][W] (channels 1) or [B][3][H][W].  Returns 0, or -1 on a bad size.
extern "C" int raster_host(int np, const int* body, const int* kind, const int* nv, const int* goff,
                           const float* dyn, const float* geom, int gstride, int B, const float* cam,
                           int follow_body, int follow_angle, int W, int H, int channels,
                           const unsigned char* palette, unsigned char* image) {
  if (np < 0 || np > cxk::MAXRP || B <= 0 || W <= 0 || H <= 0 || (channels != 1 && channels != 3)) return -1;
  if ((channels == 3) != (palette != nullptr)) return -1;
  cxk::RasterParts rp{};
  rp.np = np;
  for (int p = 0; p < np; ++p) {
    rp.body[p] = body[p];
    rp.kind[p] = kind[p];
    rp.nv[p] = nv[p];
    rp.goff[p] = goff[p];
    const unsigned char* c = palette ? palette + 3 * (body[p] + 1) : nullptr;
    rp.val[p] = c ? (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 : (uint32_t)(body[p] + 1);
  }
  rp.bg = palette ? (uint32_t)palette[0] | (uint32_t)palette[1] << 8 | (uint32_t)palette[2] << 16 : 0u;
  const cxk::RasterCam rc{cam[0], cam[1], cam[2], cam[3], follow_body, follow_angle};
  std::vector<float> words((size_t)cxk::MAXRP * cxk::RASTER_PW);
  const size_t plane = (size_t)W * H;
  for (int g = 0; g < B; ++g) {
    for (int p = 0; p < np; ++p)
      cxk::raster_part_words(dyn, B, geom, gstride, body[p], kind[p], nv[p], goff[p], g,
                             words.data() + (size_t)cxk::RASTER_PW * p);
    float fr[4];
    cxk::raster_frame(dyn, B, rc, g, fr);
    for (int j = 0; j < H; ++j)
      for (int i = 0; i < W; ++i) {
        const cx::v2 pt = cxk::raster_point(rc, W, H, i, j, fr[0], fr[1], fr[2], fr[3]);
        uint32_t val;
        cxk::raster_pixels<1>(rp, words.data(), &pt, &val);
        for (int ch = 0; ch < channels; ++ch)
          image[((size_t)g * channels + ch) * plane + (size_t)j * W + i] = (unsigned char)(val >> (8 * ch) & 255u);
      }
  }
  return 0;
}
