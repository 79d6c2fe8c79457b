// cotix_raycast_grad.h -- range-sensor gradients: the vector-Jacobian product
// of cotix_raycast's distances with respect to every body's pose and every
// geometry word (cotix_raycast_backward).  Included by
// cotix_step.hip (the gfx950 kernel) and by the tests' host checker
// (tests/emu/cotix_raygrad_host.cpp), which runs the same per-part, per-ray and
// per-slot functions in a plain loop.  cotix_raycast.h is included, not changed.
//
// Semantics.  With dist[g][k] of cotix_raycast.h and a cotangent g_dist[g][k],
// the outputs are sum_k g_dist[g][k] * d dist[g][k] / d x for x = every body's
// (px, py, angle) and every word of the env's local geometry.  The derivative
// is that of the executed branch (the rule of parallax_amd/rollout.py):
//   * the winning crossing is held fixed -- the part, and its edge or its
//     circle root t0 / t1 -- and is found by re-casting with the forward's own
//     comparisons (ray_cast_win below: the same passes, the same tie rule);
//   * order_clockwise's permutation is held fixed: the cotangent of a sorted
//     world vertex goes to the stored vertex it came from (poly_rank below);
//     nothing flows through the sort keys, the mean or atan2;
//   * with (c, sn) of body_frame, d c = -sn d angle and d sn = c d angle; the
//     divisions by t2 == 1 of forward_vector are the identity;
//   * a ray that crosses nothing (hit == 0) and a ray whose cotangent is +-0
//     contribute nothing: both are selects, never multiplications, so a NaN or
//     inf cotangent on a miss reaches no word;
//   * the sensor's body receives the cotangent of o and, with follow_angle,
//     that of d through its own frame; a body that is both the sensor's and
//     the one crossed gets both contributions;
//   * AABBs and circles do not depend on the angle: their angle gradient is 0;
//   * dirs, the sensor's offset and max_range are not differentiated.
// Per ray, every operation one f32 operation rounded on its own, g = g_dist:
//   edge (e0, e1), s = e1 - e0, w = e0 - o, c = cross(d, s), t = cross(w, s) / c:
//     gN = g / c, gc = -(gN * t)
//     g_w = (gN*s.y, -(gN*s.x)),  g_d = (gc*s.y, -(gc*s.x))
//     g_s = (-(gN*w.y) - gc*d.y, gN*w.x + gc*d.x)
//     g_e0 = g_w - g_s, g_e1 = g_s, g_o = -g_w
//   circle (r, cen), m = o - cen, a, b, q, sq as the forward's, t = (-b + sg*sq) / a
//   with sg = -1 (root t0) or +1 (root t1):
//     ga0 = g / a, g_sq = sg*ga0, g_disc = g_sq / (2*sq)
//     g_b = -ga0 + (2*b)*g_disc, g_a = -(ga0*t) - q*g_disc, g_q = -(a*g_disc)
//     g_m = m*(2*g_q) + d*g_b, g_d = m*g_b + d*(2*g_a), g_o = g_m, g_cen = -g_m
//     g_r = ((2*r) / (2*sq)) * (a*g_sq)   (-(2*r)*g_q in this association: a ray
//     from the circle's own centre with a == 1 has sq == r and returns g exactly)
//   a world vertex v = (c*x - sn*y + px, sn*x + c*y + py) of the stored (x, y):
//     g_x = c*gv.x + sn*gv.y, g_y = (-sn)*gv.x + c*gv.y, g_p = gv,
//     g_angle = gv.x*(-(sn*x) - c*y) + gv.y*(c*x - sn*y)
//   (the sensor's o and d with follow_angle: the same, with the offset and
//   the table's direction in place of (x, y); o first, then d).
// The record of a ray (RG_REC words) holds the sensor body's (g_px, g_py,
// g_angle), the crossed body's, and at most four (geometry word, value) pairs:
//   circle:  (goff, g_r), (goff+1, g_cen.x), (goff+2, g_cen.y)
//   AABB:    the edge's two corners share one stored coordinate word; that word
//            gets g_e0's component + g_e1's (in this order), the other two
//            words one component each: three pairs, in the order of the words
//            of (e0.x, e0.y, e1.x, e1.y) with the second mention dropped
//   polygon: (x of e0's stored vertex, g_x), (y, g_y), then e1's
// The crossed body's (g_px, g_py, g_angle) is e0's contribution + e1's.
//
// Reduction.  Output slot s is a pose word (s = 3*body + 0 / 1 / 2 for px, py,
// angle; s < 3*n_bodies) or geometry word s - 3*n_bodies.  Each slot is the sum
// of its records' addends in ascending ray index starting from +0.0f
// (raygrad_accumulate); within one ray, the sensor's contribution comes before
// the crossed body's, and the pairs in record order.  No atomics anywhere: the
// result is reproducible and equals the host checker's loop bit for bit.
#pragma once
#include "cotix_raycast.h"

namespace cxk {

constexpr int RG_REC = 16;                      // words per ray record
constexpr int RG_MAXBODIES = 16;                // COTIX_MAX_STATE_WORDS / 6
constexpr int RG_MAXGW = MAXRP * RASTER_PW;     // 512 geometry words
constexpr int RG_MAXSLOTS = RG_MAXGW + 3 * RG_MAXBODIES;
// record words: 0..2 the sensor body's (px, py, angle) cotangent, 3 meta (bit 0:
// the ray contributes, bits 8..: the crossed body), 4..6 the crossed body's, 7
// unused, 8..11 geometry word indices (-1: none), 12..15 their values
struct RayWin {
  float t;
  int part, feat;  // the winning part (index into RasterParts; -1: none); its edge, or circle root 0 / 1
  uint32_t id;
};

// ray_vs_shape with the winning feature: the same passes and comparisons
CX_DEV float ray_vs_shape_win(const cx::Shape& s, cx::v2 o, cx::v2 d, float max_range, int* feat) {
  float best = cx::finf();
  *feat = 0;
  if (s.kind == cx::KIND_CIRCLE) {
    const float r = s.w[0];
    const cx::v2 m = cx::sub(o, cx::v2{s.w[1], s.w[2]});
    const float a = cx::dot(d, d), b = cx::dot(m, d), q = cx::dot(m, m) - r * r;
    const float disc = b * b - a * q;
    const float sq = __builtin_sqrtf(disc);
    const float t0 = (-b - sq) / a, t1 = (-b + sq) / a;
    const float t = t0 >= 0.0f ? t0 : t1;
    *feat = t0 >= 0.0f ? 0 : 1;
    return (t >= 0.0f && t <= max_range) ? t : best;
  }
  const int cnt = cx::cvx_count(s);
  const cx::v2 last = s.kind == cx::KIND_AABB ? cx::v2{0.0f, 0.0f} : cx::vert(s, s.n - 1);
  int f = 0;
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
      f = ok ? k : f;
    }
  *feat = f;
  return best;
}

// ray_cast with the winner: t and id are ray_cast's *dist and *id, bit for bit
CX_DEV RayWin ray_cast_win(const RasterParts& rp, const float* words, cx::v2 o, cx::v2 d, float max_range) {
  float best = cx::finf();
  uint32_t hit = 0u;
  int part = -1, feat = 0;
  for (int p = 0; p < rp.np; ++p) {
    const cx::Shape s = raster_shape(rp.kind[p], rp.nv[p], words + RASTER_PW * p);
    int f;
    const float t = ray_vs_shape_win(s, o, d, max_range, &f);
    const bool nearer = t < best;
    best = nearer ? t : best;
    hit = nearer ? rp.val[p] : hit;
    part = nearer ? p : part;
    feat = nearer ? f : feat;
  }
  return RayWin{hit != 0u ? best : max_range, hit != 0u ? part : -1, feat, hit};
}

// The stable rank of cx::order_clockwise, restated (cotix_device.h is the fused
// kernels' and stays as it is): vertex k of q goes to sorted position rank[k]
// = #{j : key_j < key_k} + #{j < k : not key_k < key_j}, key = atan2 about the
// sequential mean, NaN -> 4.  rank[0 .. n) is a permutation of 0 .. n-1.
CX_DEV void poly_rank(const cx::Poly& q, int n, int* rank) {
  float sx = 0.0f, sy = 0.0f;
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k)
    if (k < n) {
      sx = sx + q.x[k];
      sy = sy + q.y[k];
    }
  const float fn = (float)n;
  const float mx = sx / fn, my = sy / fn;
  float key[cx::MAXV];
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k) {
    key[k] = 0.0f;
    if (k < n) {
      const float a = cx::atan2_32(q.y[k] - my, q.x[k] - mx);
      key[k] = cx::isn(a) ? 4.0f : a;
    }
  }
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < cx::MAXV; ++j)
      if (j != k && j < n) r += (j < k ? !(key[k] < key[j]) : (key[j] < key[k])) ? 1 : 0;
    rank[k] = r;
  }
}

// the world vertices of a polygon before the sort (raster_part_words' arithmetic)
CX_DEV cx::Poly poly_world(const float* lg, int n, float c, float sn, float px, float py) {
  cx::Poly q;
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k) {
    q.x[k] = 0.0f;
    q.y[k] = 0.0f;
    if (k < n) {
      const float x = lg[2 * k], y = lg[2 * k + 1];
      const float t0 = (c * x + (-sn) * y) + px * 1.0f, t1 = (sn * x + c * y) + py * 1.0f;
      const float t2 = (0.0f * x + 0.0f * y) + 1.0f * 1.0f;
      q.x[k] = t2 == 1.0f ? t0 : cx::qnan();
      q.y[k] = t2 == 1.0f ? t1 : cx::qnan();
    }
  }
  return q;
}

// what the backward keeps of part p of env g besides its world words: pf = the
// body's (cos, sin), inv[i] = the stored vertex of sorted vertex i (MAXV
// entries; the identity for a circle or an AABB) and meta = (kind, n, goff,
// body): the part table where a lane can index it by its own winner
CX_DEV void raygrad_part(const float* dyn, int B, const float* geom, int gstride, int body, int kind, int n, int goff,
                         int g, float* pf, int* inv, int* meta) {
  meta[0] = kind;
  meta[1] = n;
  meta[2] = goff;
  meta[3] = body;
  const float* lg = geom + (gstride ? (size_t)g * gstride : (size_t)0) + goff;
  float c, sn, px, py;
  body_frame(dyn, B, body, g, &c, &sn, &px, &py);
  pf[0] = c;
  pf[1] = sn;
#pragma unroll
  for (int k = 0; k < cx::MAXV; ++k) inv[k] = k;
  if (kind != cx::KIND_POLY) return;
  const cx::Poly q = poly_world(lg, n, c, sn, px, py);
  int rank[cx::MAXV];
  poly_rank(q, n, rank);
#pragma unroll
  for (int i = 0; i < cx::MAXV; ++i) {
    int j = i;
#pragma unroll
    for (int k = 0; k < cx::MAXV; ++k) j = (k < n && rank[k] == i) ? k : j;
    inv[i] = j;
  }
}

CX_DEV void raygrad_empty(float* rec) {
  uint32_t* u = reinterpret_cast<uint32_t*>(rec);  // words 3 and 8..11 are only ever touched as integers
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k != 3) rec[k] = 0.0f;
  u[3] = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    u[8 + k] = 0xffffffffu;
    rec[12 + k] = 0.0f;
  }
}

// the cotangent of (x, y) -> (c*x - sn*y + px, sn*x + c*y + py) with respect to the angle
CX_DEV float raygrad_turn(float c, float sn, float x, float y, cx::v2 gv) {
  return gv.x * (-(sn * x) - c * y) + gv.y * (c * x - sn * y);
}

// The record of one ray.  words / pf / inv / meta: the parts of the env as built by
// raster_part_words and raygrad_part (RASTER_PW, 2, MAXV and 4 entries per part);
// lgeom: the env's local geometry row; fr: ray_frame's; (x, y): the table's
// direction; g: the ray's cotangent.
CX_DEV void raygrad_record(const RasterParts& rp, const float* words, const float* pf, const int* inv,
                           const int* meta, const float* lgeom, const RaySensor& rs, const float* fr, float x,
                           float y, float g, float* rec) {
  raygrad_empty(rec);
  const cx::v2 o{fr[2], fr[3]};
  const cx::v2 d = ray_dir(rs, fr[0], fr[1], x, y);
  const RayWin win = ray_cast_win(rp, words, o, d, rs.max_range);
  if (win.part < 0 || g == 0.0f) return;  // a miss, or a +-0 cotangent: nothing, whatever g holds
  const int p = win.part, kind = meta[4 * p], goff = meta[4 * p + 2];
  const float* w = words + RASTER_PW * p;
  uint32_t* u = reinterpret_cast<uint32_t*>(rec);
  cx::v2 g_o, g_d;
  if (kind == cx::KIND_CIRCLE) {
    const float r = w[0];
    const cx::v2 m = cx::sub(o, cx::v2{w[1], w[2]});
    const float a = cx::dot(d, d), b = cx::dot(m, d), q = cx::dot(m, m) - r * r;
    const float sq = __builtin_sqrtf(b * b - a * q);
    const float sg = win.feat == 0 ? -1.0f : 1.0f;
    const float ga0 = g / a, g_sq = sg * ga0, g_disc = g_sq / (2.0f * sq);
    const float g_b = -ga0 + (2.0f * b) * g_disc, g_a = -(ga0 * win.t) - q * g_disc, g_q = -(a * g_disc);
    const float tq = 2.0f * g_q;
    const cx::v2 g_m{m.x * tq + d.x * g_b, m.y * tq + d.y * g_b};
    const float ta = 2.0f * g_a;
    g_d = cx::v2{m.x * g_b + d.x * ta, m.y * g_b + d.y * ta};
    g_o = g_m;
    rec[4] = -g_m.x;
    rec[5] = -g_m.y;
    rec[6] = 0.0f;
    u[8] = (uint32_t)goff;
    u[9] = (uint32_t)(goff + 1);
    u[10] = (uint32_t)(goff + 2);
    rec[12] = ((2.0f * r) / (2.0f * sq)) * (a * g_sq);
    rec[13] = -g_m.x;
    rec[14] = -g_m.y;
  } else {
    // the winning edge's corners, in cx::cvx_edge's order: word indices within the part
    const int k = win.feat, n = meta[4 * p + 1];
    int ix0, iy0, ix1, iy1;
    if (kind == cx::KIND_AABB) {
      const int k1 = (k + 1) & 3;
      ix0 = (k == 0 || k == 1) ? 2 : 0;
      iy0 = (k == 0 || k == 3) ? 3 : 1;
      ix1 = (k1 == 0 || k1 == 1) ? 2 : 0;
      iy1 = (k1 == 0 || k1 == 3) ? 3 : 1;
    } else {
      const int k1 = k == 0 ? n - 1 : k - 1;
      ix0 = 2 * k;
      iy0 = 2 * k + 1;
      ix1 = 2 * k1;
      iy1 = 2 * k1 + 1;
    }
    const cx::v2 e0{w[ix0], w[iy0]}, e1{w[ix1], w[iy1]};
    const cx::v2 sv = cx::sub(e1, e0), wv = cx::sub(e0, o);
    const float c = ray_cross(d, sv);
    const float gN = g / c, gc = -(gN * win.t);
    const cx::v2 g_w{gN * sv.y, -(gN * sv.x)};
    const cx::v2 g_s{-(gN * wv.y) - gc * d.y, gN * wv.x + gc * d.x};
    g_d = cx::v2{gc * sv.y, -(gc * sv.x)};
    g_o = cx::v2{-g_w.x, -g_w.y};
    const cx::v2 g0 = cx::sub(g_w, g_s), g1 = g_s;
    rec[4] = g0.x + g1.x;
    rec[5] = g0.y + g1.y;
    rec[6] = 0.0f;
    if (kind == cx::KIND_AABB) {
      // even edges share x (one x word, two y words), odd edges share y
      if (ix0 == ix1) {
        u[8] = (uint32_t)(goff + ix0);
        u[9] = (uint32_t)(goff + iy0);
        u[10] = (uint32_t)(goff + iy1);
        rec[12] = g0.x + g1.x;
        rec[13] = g0.y;
        rec[14] = g1.y;
      } else {
        u[8] = (uint32_t)(goff + ix0);
        u[9] = (uint32_t)(goff + iy0);
        u[10] = (uint32_t)(goff + ix1);
        rec[12] = g0.x;
        rec[13] = g0.y + g1.y;
        rec[14] = g1.x;
      }
    } else {
      const float c_ = pf[2 * p], sn = pf[2 * p + 1];
      const int j0 = inv[cx::MAXV * p + k], j1 = inv[cx::MAXV * p + (k == 0 ? n - 1 : k - 1)];
      const float* lg = lgeom + goff;
      const float x0 = lg[2 * j0], y0 = lg[2 * j0 + 1], x1 = lg[2 * j1], y1 = lg[2 * j1 + 1];
      u[8] = (uint32_t)(goff + 2 * j0);
      u[9] = (uint32_t)(goff + 2 * j0 + 1);
      u[10] = (uint32_t)(goff + 2 * j1);
      u[11] = (uint32_t)(goff + 2 * j1 + 1);
      rec[12] = c_ * g0.x + sn * g0.y;
      rec[13] = (-sn) * g0.x + c_ * g0.y;
      rec[14] = c_ * g1.x + sn * g1.y;
      rec[15] = (-sn) * g1.x + c_ * g1.y;
      rec[6] = raygrad_turn(c_, sn, x0, y0, g0) + raygrad_turn(c_, sn, x1, y1, g1);
    }
  }
  u[3] = 1u | (uint32_t)meta[4 * p + 3] << 8;
  if (rs.body < 0) return;
  rec[0] = g_o.x;
  rec[1] = g_o.y;
  if (rs.follow_angle) rec[2] = raygrad_turn(fr[0], fr[1], rs.ox, rs.oy, g_o) + raygrad_turn(fr[0], fr[1], x, y, g_d);
}

// one record's addends to output slot `slot` (nb3 = 3 * n_bodies), after acc
CX_DEV float raygrad_accumulate(const float* rec, int slot, int nb3, int sensor_body, float acc) {
  const uint32_t* u = reinterpret_cast<const uint32_t*>(rec);
  const uint32_t meta = u[3];
  const bool on = (meta & 1u) != 0u;
  if (slot < nb3) {
    const int body = slot / 3, comp = slot - 3 * body;
    const float sv = comp == 0 ? rec[0] : (comp == 1 ? rec[1] : rec[2]);
    const float bv = comp == 0 ? rec[4] : (comp == 1 ? rec[5] : rec[6]);
    acc = (on && body == sensor_body) ? acc + sv : acc;
    acc = (on && body == (int)(meta >> 8)) ? acc + bv : acc;
    return acc;
  }
  const uint32_t wd = (uint32_t)(slot - nb3);
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = (on && u[8 + k] == wd) ? acc + rec[12 + k] : acc;
  return acc;
}

// slot s of env g: where it is stored (pose slots: rows 0, 1 and 4 of the body)
CX_DEV void raygrad_store(int slot, int nb3, int B, int g, float v, float* g_dyn, float* g_geom) {
  if (slot < nb3) {
    const int body = slot / 3, comp = slot - 3 * body;
    if (g_dyn) g_dyn[((size_t)body * 6 + (comp == 2 ? 4 : comp)) * B + g] = v;
  } else if (g_geom) {
    g_geom[(size_t)(slot - nb3) * B + g] = v;
  }
}

#if defined(__HIP__) || defined(__HIPCC__)
// One wave per env, four envs per workgroup, as raycast_kernel.  Lane p builds
// world part p, its body's (cos, sin) and its inverse rank into LDS, the
// wave's last lane the sensor's frame, and every lane zeroes its slots'
// accumulators; one barrier.  Rays then go in chunks of 64, one per lane: a
// lane re-casts its ray (the part words are LDS broadcasts) and stores its
// record to LDS; after a barrier lane j walks the chunk's 64 records in ray
// order for each of its slots j, j + 64, ... (every lane reads the same record
// word: a broadcast), the running sums living in LDS words only lane j touches;
// a second barrier frees the records for the next chunk.  Chunks ascend, so
// each word's total order is ascending ray index.  Every thread, live or not,
// runs the same number of chunks (n_rays is the launch's) and takes every
// barrier: the four waves share nothing else.  At the end every slot is stored
// once and the velocity rows get their zeros.
constexpr int RG_BLOCK = 256, RG_EPB = RG_BLOCK / 64;
__global__ __launch_bounds__(RG_BLOCK) void raycast_grad_kernel(const float* dyn, int B, const float* geom,
                                                                int gstride, RasterParts rp, RaySensor rs,
                                                                const float* dirs, int R, const float* g_dist,
                                                                int nb, int gw, float* g_dyn, float* g_geom) {
  static_assert(MAXRP < 64, "a lane per part and one for the frame");
  __shared__ float s_words[RG_EPB][MAXRP * RASTER_PW];
  __shared__ float s_pf[RG_EPB][MAXRP * 2];
  __shared__ int s_inv[RG_EPB][MAXRP * cx::MAXV];
  __shared__ int s_meta[RG_EPB][MAXRP * 4];
  __shared__ float s_frame[RG_EPB][4];
  __shared__ __attribute__((aligned(16))) float s_rec[RG_EPB][64 * RG_REC];
  __shared__ float s_acc[RG_EPB][RG_MAXSLOTS];
  const int e = threadIdx.x / 64, l = threadIdx.x % 64;
  const long long gl = (long long)blockIdx.x * RG_EPB + e;
  const bool live = gl < (long long)B;
  const int g = live ? (int)gl : 0;
  const int nb3 = 3 * nb, slots = nb3 + gw;  // slots <= RG_MAXSLOTS: the entry point's check
  if (live && l < rp.np) {
    raster_part_words(dyn, B, geom, gstride, rp.body[l], rp.kind[l], rp.nv[l], rp.goff[l], g,
                      &s_words[e][RASTER_PW * l]);
    raygrad_part(dyn, B, geom, gstride, rp.body[l], rp.kind[l], rp.nv[l], rp.goff[l], g, &s_pf[e][2 * l],
                 &s_inv[e][cx::MAXV * l], &s_meta[e][4 * l]);
  }
  if (live && l == 63) ray_frame(dyn, B, rs, g, s_frame[e]);
  for (int s = l; s < slots; s += 64) s_acc[e][s] = 0.0f;
  __syncthreads();
  const float* lgeom = geom + (gstride ? (size_t)g * gstride : (size_t)0);
  const size_t row = (size_t)g * R;
  for (int k0 = 0; k0 < R; k0 += 64) {
    const int k = k0 + l;
    float* rec = &s_rec[e][RG_REC * l];
    if (live && k < R)
      raygrad_record(rp, s_words[e], s_pf[e], s_inv[e], s_meta[e], lgeom, rs, s_frame[e], dirs[2 * k],
                     dirs[2 * k + 1], g_dist[row + k], rec);
    else
      raygrad_empty(rec);
    __syncthreads();
    if (live)
      for (int s = l; s < slots; s += 64) {
        float acc = s_acc[e][s];
        for (int j = 0; j < 64; ++j) acc = raygrad_accumulate(&s_rec[e][RG_REC * j], s, nb3, rs.body, acc);
        s_acc[e][s] = acc;
      }
    __syncthreads();
  }
  if (!live) return;
  for (int s = l; s < slots; s += 64) raygrad_store(s, nb3, B, g, s_acc[e][s], g_dyn, g_geom);
  if (g_dyn)
    for (int s = l; s < nb3; s += 64) {  // the velocity rows 2, 3 and 5
      const int body = s / 3, comp = s - 3 * body;
      g_dyn[((size_t)body * 6 + (comp == 2 ? 5 : 2 + comp)) * B + g] = 0.0f;
    }
}
#endif

}  // namespace cxk
