// TEST INFRASTRUCTURE ONLY: the host checker of cotix_raycast -- a plain loop
// over envs and rays around the per-part and per-ray functions of
// parallax_amd/csrc/cotix_raycast.h (the code the gfx950 kernel runs), built
// with the kernel's floating-point flags (tests/emu/raycast.mk).
#include <vector>

#include "../../parallax_amd/csrc/cotix_raycast.h"

// part table: body / kind (0 circle, 1 AABB, 2 polygon) / nv / goff per part,
// in scene order (every part: the ignored bodies' are left out here, as the
// library's entry does); dyn f32 [n_bodies][6][B]; geom shared (gstride 0) or
// one row per env; sensor = (ox, oy, max_range); dirs f32 [R][2].
// dist f32 [B][R], hit u8 [B][R] or NULL.  Returns 0, or -1 on a bad size.
extern "C" int raycast_host(int np, const int* body, const int* kind, const int* nv, const int* goff,
                            const float* dyn, const float* geom, int gstride, int B, const float* sensor,
                            int sensor_body, int follow_angle, unsigned ignore_mask, const float* dirs, int R,
                            float* dist, unsigned char* hit) {
  if (np < 0 || np > cxk::MAXRP || B <= 0 || R <= 0) return -1;
  cxk::RasterParts rp{};
  for (int p = 0; p < np; ++p) {
    if (body[p] < 32 && (ignore_mask >> body[p] & 1u) != 0u) continue;
    rp.body[rp.np] = body[p];
    rp.kind[rp.np] = kind[p];
    rp.nv[rp.np] = nv[p];
    rp.goff[rp.np] = goff[p];
    rp.val[rp.np] = (uint32_t)(body[p] + 1);
    ++rp.np;
  }
  const cxk::RaySensor rs{sensor_body, follow_angle, sensor[0], sensor[1], sensor[2]};
  std::vector<float> words((size_t)cxk::MAXRP * cxk::RASTER_PW);
  for (int g = 0; g < B; ++g) {
    for (int p = 0; p < rp.np; ++p)
      cxk::raster_part_words(dyn, B, geom, gstride, rp.body[p], rp.kind[p], rp.nv[p], rp.goff[p], g,
                             words.data() + (size_t)cxk::RASTER_PW * p);
    float fr[4];
    cxk::ray_frame(dyn, B, rs, g, fr);
    for (int k = 0; k < R; ++k) {
      const cx::v2 d = cxk::ray_dir(rs, fr[0], fr[1], dirs[2 * k], dirs[2 * k + 1]);
      float t;
      uint32_t id;
      cxk::ray_cast(rp, words.data(), cx::v2{fr[2], fr[3]}, d, rs.max_range, &t, &id);
      dist[(size_t)g * R + k] = t;
      if (hit) hit[(size_t)g * R + k] = (unsigned char)id;
    }
  }
  return 0;
}
