// cotix_raycast.h -- range-sensor observations: a fan of rays cast from every
// env on the device (cotix_raycast).  Included by
// cotix_step.hip (the gfx950 kernel) and by the tests' host checker
// (tests/emu/cotix_raycast_host.cpp), which runs the same per-part and per-ray
// functions in a plain loop.
//
// Semantics (every operation one f32 operation rounded on its own;
// cross(u, v) = u.x*v.y - v.x*u.y as in cx::edge_vs_edge, dot as cx::dot):
//   o, d = (ox, oy), dirs[k]                                 no body
//        = (ox, oy) + position(body), dirs[k]                follow_angle == 0
//        = Transformer(position, angle).forward_vector((ox, oy)),
//          (c*x + (-sn)*y, sn*x + c*y)                       follow_angle == 1
//   edge (e0, e1) of an AABB / polygon, in cx::cvx_edge's order, with
//   s = e1 - e0, w = e0 - o:  c = cross(d, s), t = cross(w, s) / c,
//   u = cross(w, d) / c; a crossing at t when c != 0, 0 <= t <= max_range,
//   0 <= u <= 1 (edge_vs_edge with the ray as the first edge)
//   circle (r, cen), m = o - cen:  a = dot(d, d), b = dot(m, d),
//   q = dot(m, m) - r*r, sq = sqrt(b*b - a*q), t0 = (-b - sq) / a,
//   t1 = (-b + sq) / a, t = t0 >= 0 ? t0 : t1; a crossing when 0 <= t <= max_range
//   dist = the smallest t over the parts in scene order and their edges in
//   order (a later crossing replaces an earlier one only when strictly nearer),
//   hit = 1 + that part's body; max_range and 0 where nothing is crossed.
// World parts are raster_part_words' (cotix_raster.h).  Consequences, by design:
//   * boundary crossings, not entries: a ray that starts inside a shape reports
//     where it leaves it;
//   * a NaN makes every comparison false: a NaN vertex removes the edges that
//     touch it, a body with a NaN pose is invisible, and a sensor on a body with
//     a NaN pose reports max_range, 0 on every ray;
//   * a ray parallel to an edge (c == 0) does not cross it;
//   * directions are never renormalised (distances are in units of |d|), and
//     there is no culling of any kind.
#pragma once
#include "cotix_raster.h"

namespace cxk {

constexpr int MAXRAYS = 1024;
struct RaySensor {
  int body, follow_angle;  // body -1: fixed in the world
  float ox, oy, max_range;
};

// the sensor of env g: fr = (cos, sin, origin x, origin y)
CX_DEV void ray_frame(const float* dyn, int B, const RaySensor& rs, int g, float* fr) {
  fr[0] = 1.0f;
  fr[1] = 0.0f;
  fr[2] = rs.ox;
  fr[3] = rs.oy;
  if (rs.body < 0) return;
  float c, sn, px, py;
  body_frame(dyn, B, rs.body, g, &c, &sn, &px, &py);
  if (!rs.follow_angle) {
    fr[2] = rs.ox + px;
    fr[3] = rs.oy + py;
    return;
  }
  // HomogenuousTransformer.forward_vector (cotix/_geometry_utils.py:134-138), as raster_point
  const float x = rs.ox, y = rs.oy;
  const float t0 = (c * x + (-sn) * y) + px * 1.0f, t1 = (sn * x + c * y) + py * 1.0f;
  const float t2 = (0.0f * x + 0.0f * y) + 1.0f * 1.0f;
  fr[0] = c;
  fr[1] = sn;
  fr[2] = t0 / t2;
  fr[3] = t1 / t2;
}

// the world direction of the table's (x, y)
CX_DEV cx::v2 ray_dir(const RaySensor& rs, float c, float sn, float x, float y) {
  if (!rs.follow_angle) return cx::v2{x, y};
  return cx::v2{c * x + (-sn) * y, sn * x + c * y};
}

CX_DEV float ray_cross(cx::v2 u, cx::v2 v) { return u.x * v.y - v.x * u.y; }

// the nearest crossing of one world part by the ray o + t d, 0 <= t <=
// max_range; +inf when it has none.  kind and n are uniform over a wave; the
// conditions of an edge are selects.
CX_DEV float ray_vs_shape(const cx::Shape& s, cx::v2 o, cx::v2 d, float max_range) {
  float best = cx::finf();
  if (s.kind == cx::KIND_CIRCLE) {
    const float r = s.w[0];
    const cx::v2 m = cx::sub(o, cx::v2{s.w[1], s.w[2]});
    const float a = cx::dot(d, d), b = cx::dot(m, d), q = cx::dot(m, m) - r * r;
    const float disc = b * b - a * q;
    const float sq = __builtin_sqrtf(disc);
    const float t0 = (-b - sq) / a, t1 = (-b + sq) / a;
    const float t = t0 >= 0.0f ? t0 : t1;
    return (t >= 0.0f && t <= max_range) ? t : best;
  }
  const int cnt = cx::cvx_count(s);
  const cx::v2 last = s.kind == cx::KIND_AABB ? cx::v2{0.0f, 0.0f} : cx::vert(s, s.n - 1);
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k)
    if (k < cnt) {
      cx::v2 e0, e1;
      cx::cvx_edge(s, k, last, &e0, &e1);
      const cx::v2 sv = cx::sub(e1, e0), w = cx::sub(e0, o);
      const float c = ray_cross(d, sv);
      const float t = ray_cross(w, sv) / c, u = ray_cross(w, d) / c;
      const bool ok = (c != 0.0f) & (t >= 0.0f) & (t <= max_range) & (u >= 0.0f) & (u <= 1.0f) & (t < best);
      best = ok ? t : best;
    }
  return best;
}

// one ray against the parts in scene order: *dist, *id = the nearest crossing
// and 1 + its body (rp.val), or max_range and 0
CX_DEV void ray_cast(const RasterParts& rp, const float* words, cx::v2 o, cx::v2 d, float max_range, float* dist,
                     uint32_t* id) {
  float best = cx::finf();
  uint32_t hit = 0u;
  for (int p = 0; p < rp.np; ++p) {
    const cx::Shape s = raster_shape(rp.kind[p], rp.nv[p], words + RASTER_PW * p);
    const float t = ray_vs_shape(s, o, d, max_range);
    const bool nearer = t < best;
    best = nearer ? t : best;
    hit = nearer ? rp.val[p] : hit;
  }
  *dist = hit != 0u ? best : max_range;
  *id = hit;
}

#if defined(__HIP__) || defined(__HIPCC__)
// One wave per env, four envs per workgroup: lane p builds world part p into
// LDS and the wave's last lane the sensor's frame; one barrier, taken by every
// thread; then lane l takes rays l, l + 64, ...: the part words are LDS
// broadcasts (one address per wave), the direction comes from global memory,
// best / hit stay in registers, and a wave's stores are contiguous.
constexpr int RAY_BLOCK = 256, RAY_EPB = RAY_BLOCK / 64;
__global__ __launch_bounds__(RAY_BLOCK) void raycast_kernel(const float* dyn, int B, const float* geom, int gstride,
                                                            RasterParts rp, RaySensor rs, const float* dirs, int R,
                                                            float* dist, unsigned char* hit) {
  static_assert(MAXRP < 64, "a lane per part and one for the frame");
  __shared__ float s_words[RAY_EPB][MAXRP * RASTER_PW];
  __shared__ float s_frame[RAY_EPB][4];
  const int e = threadIdx.x / 64, l = threadIdx.x % 64;
  const long long gl = (long long)blockIdx.x * RAY_EPB + e;
  const bool live = gl < (long long)B;
  const int g = (int)gl;
  if (live && l < rp.np)
    raster_part_words(dyn, B, geom, gstride, rp.body[l], rp.kind[l], rp.nv[l], rp.goff[l], g,
                      &s_words[e][RASTER_PW * l]);
  if (live && l == 63) ray_frame(dyn, B, rs, g, s_frame[e]);
  __syncthreads();
  if (!live) return;
  const float c = s_frame[e][0], sn = s_frame[e][1];
  const cx::v2 o{s_frame[e][2], s_frame[e][3]};
  const size_t row = (size_t)g * R;
  for (int k = l; k < R; k += 64) {
    const cx::v2 d = ray_dir(rs, c, sn, dirs[2 * k], dirs[2 * k + 1]);
    float t;
    uint32_t id;
    ray_cast(rp, s_words[e], o, d, rs.max_range, &t, &id);
    dist[row + k] = t;
    if (hit) hit[row + k] = (unsigned char)id;
  }
}
#endif

}  // namespace cxk
