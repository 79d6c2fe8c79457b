// cotix_raster.h -- pixel observations: every env's filled bodies rasterized
// on the device (cotix_rasterize).  Included by
// cotix_step.hip (the gfx950 kernel) and by the tests' host checker
// (tests/emu/cotix_raster_host.cpp), which runs the same per-part and
// per-pixel functions in a plain loop.
//
// Semantics (every operation one f32 operation rounded on its own):
//   u   = float(2 i + 1 - W) / float(W)          pixel column i
//   v   = float(H - (2 j + 1)) / float(H)        pixel row j, row 0 at the top
//   loc = (cam.cx + u * cam.half_w, cam.cy + v * cam.half_h)
//   p   = loc | loc + position(follow_body) | Transformer(position, angle).forward_vector(loc)
//   id  = 1 + b of the last body b, in scene order, with a part whose world
//         shape contains(p) (cx::shape_contains: the reference's point tests,
//         eps included); 0 where no part does
// World parts are render_part_env's (cotix_body.h): circle position + shift,
// AABB lower / upper + shift, polygon forward_vector of every vertex then
// order_clockwise.  No culling: Polygon.contains is "all edge signs equal", so
// a degenerate polygon contains points far from it.
#pragma once
#include "cotix_body.h"
#include "cotix_device.h"

namespace cxk {

constexpr int RASTER_PW = 2 * cx::MAXV;  // words per world part (cx::Shape::w)
struct RasterCam {
  float cx, cy, hw, hh;
  int follow_body, follow_angle;
};
// the scene's parts in draw order, with the byte(s) a hit writes: val = 1 +
// body (ids) or the body's palette entry r | g << 8 | b << 16 (RGB); bg: no hit
struct RasterParts {
  int np;
  int body[MAXRP], kind[MAXRP], nv[MAXRP], goff[MAXRP];
  uint32_t val[MAXRP];
  uint32_t bg;
};

// part p of env g in world coordinates, as the RASTER_PW words of a cx::Shape
// (the arithmetic of render_part_env; unused words 0)
CX_DEV void raster_part_words(const float* dyn, int B, const float* geom, int gstride, int body, int kind, int n,
                              int goff, int g, float* o) {
  const float* lg = geom + (gstride ? (size_t)g * gstride : (size_t)0) + goff;
  float c, sn, px, py;
  body_frame(dyn, B, body, g, &c, &sn, &px, &py);
#pragma unroll
  for (int k = 0; k < RASTER_PW; ++k) o[k] = 0.0f;
  if (kind == cx::KIND_CIRCLE) {  // Circle.transform: position + shift (:37-41); words r, cx, cy
    o[0] = lg[0];
    o[1] = lg[1] + px;
    o[2] = lg[2] + py;
  } else if (kind == cx::KIND_AABB) {  // lower/upper + shift (:113-117)
    o[0] = lg[0] + px;
    o[1] = lg[1] + py;
    o[2] = lg[2] + px;
    o[3] = lg[3] + py;
  } else {  // forward_vector of every vertex, then order_clockwise (Polygon.transform, :181-187)
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
    const cx::Poly v = cx::order_clockwise(q, n);
#pragma unroll
    for (int k = 0; k < cx::MAXV; ++k)
      if (k < n) {
        o[2 * k] = v.x[k];
        o[2 * k + 1] = v.y[k];
      }
  }
}

// the followed body's frame (cos, sin, px, py) of env g; unused without one
CX_DEV void raster_frame(const float* dyn, int B, const RasterCam& cam, int g, float* fr) {
  fr[0] = 1.0f;
  fr[1] = 0.0f;
  fr[2] = 0.0f;
  fr[3] = 0.0f;
  if (cam.follow_body >= 0) body_frame(dyn, B, cam.follow_body, g, &fr[0], &fr[1], &fr[2], &fr[3]);
}

// the world point of pixel (column i, row j)
CX_DEV cx::v2 raster_point(const RasterCam& cam, int W, int H, int i, int j, float c, float sn, float px, float py) {
  const float u = (float)(2 * i + 1 - W) / (float)W;
  const float v = (float)(H - (2 * j + 1)) / (float)H;
  const float x = cam.cx + u * cam.hw, y = cam.cy + v * cam.hh;
  if (cam.follow_body < 0) return cx::v2{x, y};
  if (!cam.follow_angle) return cx::v2{x + px, y + py};
  // HomogenuousTransformer.forward_vector (cotix/_geometry_utils.py:134-138)
  const float t0 = (c * x + (-sn) * y) + px * 1.0f, t1 = (sn * x + c * y) + py * 1.0f;
  const float t2 = (0.0f * x + 0.0f * y) + 1.0f * 1.0f;
  return cx::v2{t0 / t2, t1 / t2};
}

// a world part's words as a cx::Shape: only the words its kind reads
CX_DEV cx::Shape raster_shape(int kind, int n, const float* w) {
  cx::Shape s;
  s.kind = kind;
  s.n = n;
#pragma unroll
  for (int k = 0; k < RASTER_PW; ++k) s.w[k] = 0.0f;
  if (kind == cx::KIND_POLY) {
#pragma unroll
    for (int k = 0; k < cx::MAXV; ++k)
      if (k < n) {
        s.w[2 * k] = w[2 * k];
        s.w[2 * k + 1] = w[2 * k + 1];
      }
  } else {
    s.w[0] = w[0];
    s.w[1] = w[1];
    s.w[2] = w[2];
    if (kind == cx::KIND_AABB) s.w[3] = w[3];
  }
  return s;
}

// NP pixels against the parts in draw order: the last hit's value per pixel
template <int NP>
CX_DEV void raster_pixels(const RasterParts& rp, const float* words, const cx::v2* p, uint32_t* val) {
#pragma unroll
  for (int k = 0; k < NP; ++k) val[k] = rp.bg;
  for (int t = 0; t < rp.np; ++t) {
    const cx::Shape s = raster_shape(rp.kind[t], rp.nv[t], words + RASTER_PW * t);
    const uint32_t pv = rp.val[t];
#pragma unroll
    for (int k = 0; k < NP; ++k) val[k] = cx::shape_contains(s, p[k]) ? pv : val[k];
  }
}

#if defined(__HIP__) || defined(__HIPCC__)
// One group of GROUP lanes (a wave, or the workgroup's four) per env: lane p
// builds world part p into LDS and the last lane the followed body's frame,
// one barrier, then every lane takes 4 horizontally adjacent pixels at a time
// (pixel quad q of the row-major image: bytes 4 q .. 4 q + 3 of a plane), reads
// the part words as LDS broadcasts and writes one 32-bit word per plane.
constexpr int RASTER_BLOCK = 256;
template <int GROUP>
__global__ __launch_bounds__(RASTER_BLOCK) void raster_kernel(const float* dyn, int B, const float* geom, int gstride,
                                                              RasterParts rp, RasterCam cam, int W, int H,
                                                              int channels, unsigned char* image) {
  constexpr int EPB = RASTER_BLOCK / GROUP;
  static_assert(GROUP % 64 == 0 && GROUP > MAXRP, "whole waves per env; a lane per part and one for the frame");
  __shared__ float s_words[EPB][MAXRP * RASTER_PW];
  __shared__ float s_frame[EPB][4];
  const int e = threadIdx.x / GROUP, l = threadIdx.x % GROUP;
  const long long gl = (long long)blockIdx.x * EPB + e;
  const bool live = gl < (long long)B;
  const int g = (int)gl;
  if (live && l < rp.np)
    raster_part_words(dyn, B, geom, gstride, rp.body[l], rp.kind[l], rp.nv[l], rp.goff[l], g,
                      &s_words[e][RASTER_PW * l]);
  if (live && l == GROUP - 1) raster_frame(dyn, B, cam, g, s_frame[e]);
  __syncthreads();
  if (!live) return;
  const float c = s_frame[e][0], sn = s_frame[e][1], px = s_frame[e][2], py = s_frame[e][3];
  const int w4 = W >> 2, nq = w4 * H;
  const size_t plane = (size_t)W * H;
  uint32_t* out = reinterpret_cast<uint32_t*>(image + (size_t)g * channels * plane);
  for (int q = l; q < nq; q += GROUP) {
    const int j = q / w4, i0 = (q - j * w4) * 4;
    cx::v2 p[4];
    uint32_t val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = raster_point(cam, W, H, i0 + k, j, c, sn, px, py);
    raster_pixels<4>(rp, s_words[e], p, val);
    if (channels == 1) {
      out[q] = (val[0] & 255u) | (val[1] & 255u) << 8 | (val[2] & 255u) << 16 | val[3] << 24;
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        out[ch * (plane >> 2) + q] = (val[0] >> (8 * ch) & 255u) | (val[1] >> (8 * ch) & 255u) << 8 |
                                     (val[2] >> (8 * ch) & 255u) << 16 | (val[3] >> (8 * ch) & 255u) << 24;
    }
  }
}
#endif

}  // namespace cxk
