// TEST INFRASTRUCTURE ONLY: the host checker of cotix_raycast_backward -- a
// plain loop over envs, rays and output slots around the per-part, per-ray and
// per-slot functions of parallax_amd/csrc/cotix_raycast_grad.h (the code the
// gfx950 kernel runs), built with the kernel's floating-point flags
// (tests/emu/raygrad.mk).
#include <vector>

#include "../../parallax_amd/csrc/cotix_raycast_grad.h"

namespace {
// the visible parts, as the library's entry builds them
int visible_parts(int np, const int* body, const int* kind, const int* nv, const int* goff, unsigned ignore_mask,
                  cxk::RasterParts* rp) {
  if (np < 0 || np > cxk::MAXRP) return -1;
  *rp = cxk::RasterParts{};
  for (int p = 0; p < np; ++p) {
    if (body[p] < 32 && (ignore_mask >> body[p] & 1u) != 0u) continue;
    rp->body[rp->np] = body[p];
    rp->kind[rp->np] = kind[p];
    rp->nv[rp->np] = nv[p];
    rp->goff[rp->np] = goff[p];
    rp->val[rp->np] = (uint32_t)(body[p] + 1);
    ++rp->np;
  }
  return 0;
}
}  // namespace

// The arguments of raycast_host (cotix_raycast_host.cpp), then nb bodies, gw
// geometry words, the cotangent g_dist f32 [B][R] and the outputs g_dyn f32
// [nb][6][B] and g_geom f32 [gw][B] (either may be NULL).  Returns 0, or -1 on a
// bad size.
extern "C" int raygrad_host(int np, const int* body, const int* kind, const int* nv, const int* goff,
                            const float* dyn, const float* geom, int gstride, int B, const float* sensor,
                            int sensor_body, int follow_angle, unsigned ignore_mask, const float* dirs, int R, int nb,
                            int gw, const float* g_dist, float* g_dyn, float* g_geom) {
  cxk::RasterParts rp;
  if (visible_parts(np, body, kind, nv, goff, ignore_mask, &rp) || B <= 0 || R <= 0 || nb < 0 ||
      nb > cxk::RG_MAXBODIES || gw < 0 || gw > cxk::RG_MAXGW)
    return -1;
  const cxk::RaySensor rs{sensor_body, follow_angle, sensor[0], sensor[1], sensor[2]};
  std::vector<float> words((size_t)cxk::MAXRP * cxk::RASTER_PW), pf((size_t)cxk::MAXRP * 2);
  std::vector<int> inv((size_t)cxk::MAXRP * cx::MAXV), meta((size_t)cxk::MAXRP * 4);
  std::vector<float> rec((size_t)R * cxk::RG_REC);
  const int nb3 = 3 * nb, slots = nb3 + gw;
  for (int g = 0; g < B; ++g) {
    for (int p = 0; p < rp.np; ++p) {
      cxk::raster_part_words(dyn, B, geom, gstride, rp.body[p], rp.kind[p], rp.nv[p], rp.goff[p], g,
                             words.data() + (size_t)cxk::RASTER_PW * p);
      cxk::raygrad_part(dyn, B, geom, gstride, rp.body[p], rp.kind[p], rp.nv[p], rp.goff[p], g, pf.data() + 2 * p,
                        inv.data() + (size_t)cx::MAXV * p, meta.data() + 4 * p);
    }
    float fr[4];
    cxk::ray_frame(dyn, B, rs, g, fr);
    const float* lgeom = geom + (gstride ? (size_t)g * gstride : (size_t)0);
    for (int k = 0; k < R; ++k)
      cxk::raygrad_record(rp, words.data(), pf.data(), inv.data(), meta.data(), lgeom, rs, fr, dirs[2 * k],
                          dirs[2 * k + 1], g_dist[(size_t)g * R + k], rec.data() + (size_t)cxk::RG_REC * k);
    for (int s = 0; s < slots; ++s) {
      float acc = 0.0f;
      for (int k = 0; k < R; ++k)
        acc = cxk::raygrad_accumulate(rec.data() + (size_t)cxk::RG_REC * k, s, nb3, rs.body, acc);
      cxk::raygrad_store(s, nb3, B, g, acc, g_dyn, g_geom);
    }
    if (g_dyn)
      for (int b = 0; b < nb; ++b)
        for (int r : {2, 3, 5}) g_dyn[((size_t)b * 6 + r) * B + g] = 0.0f;
  }
  return 0;
}

// The winner-reporting cast alone: dist f32 [B][R] and hit u8 [B][R] as
// raycast_host writes them, from ray_cast_win, and (optionally) part / feat
// i32 [B][R]: the winning visible part (-1: none) and its edge or circle root.
extern "C" int raywin_host(int np, const int* body, const int* kind, const int* nv, const int* goff, const float* dyn,
                           const float* geom, int gstride, int B, const float* sensor, int sensor_body,
                           int follow_angle, unsigned ignore_mask, const float* dirs, int R, float* dist,
                           unsigned char* hit, int* part, int* feat) {
  cxk::RasterParts rp;
  if (visible_parts(np, body, kind, nv, goff, ignore_mask, &rp) || B <= 0 || R <= 0) return -1;
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
      const cxk::RayWin w = cxk::ray_cast_win(rp, words.data(), cx::v2{fr[2], fr[3]}, d, rs.max_range);
      dist[(size_t)g * R + k] = w.t;
      hit[(size_t)g * R + k] = (unsigned char)w.id;
      if (part) part[(size_t)g * R + k] = w.part;
      if (feat) feat[(size_t)g * R + k] = w.feat;
    }
  }
  return 0;
}

// The restated rank against cx::order_clockwise: n polygons of nv vertices,
// xy f32 [n][nv][2] (world vertices, before the sort).  sorted f32 [n][nv][2] =
// cx::order_clockwise's; gathered f32 [n][nv][2] = vertex k stored at
// poly_rank's rank[k]; rank i32 [n][nv].
extern "C" int rayrank_host(int n, int nv, const float* xy, float* sorted, float* gathered, int* rank) {
  if (n < 0 || nv < 1 || nv > cx::MAXV) return -1;
  for (int i = 0; i < n; ++i) {
    cx::Poly q;
    for (int k = 0; k < cx::MAXV; ++k) {
      q.x[k] = k < nv ? xy[((size_t)i * nv + k) * 2] : 0.0f;
      q.y[k] = k < nv ? xy[((size_t)i * nv + k) * 2 + 1] : 0.0f;
    }
    const cx::Poly r = cx::order_clockwise(q, nv);
    int rk[cx::MAXV];
    cxk::poly_rank(q, nv, rk);
    for (int k = 0; k < nv; ++k) {
      sorted[((size_t)i * nv + k) * 2] = r.x[k];
      sorted[((size_t)i * nv + k) * 2 + 1] = r.y[k];
      rank[(size_t)i * nv + k] = rk[k];
      if (rk[k] < 0 || rk[k] >= nv) return -1;
      gathered[((size_t)i * nv + rk[k]) * 2] = q.x[k];
      gathered[((size_t)i * nv + rk[k]) * 2 + 1] = q.y[k];
    }
  }
  return 0;
}
