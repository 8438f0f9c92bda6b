// The front end of a sensor frame (include/gsr.h, gsr_frame_undistort / gsr_frame_pyramid): a distorted RGB-D frame becomes an
// ideal pinhole image with a validity mask, and that image a pyramid whose levels have exact intrinsics
// (scene_utils.cameras.scaled_camera).  Both kernels stream: almost no arithmetic per byte, so what counts is bytes moved.
//
//   k_frame_undistort   one thread per TARGET pixel, a workgroup = 64 x 4 pixels: every wave writes 64 consecutive floats of one row
//                       per plane (256-B stores).  The reads are a gather, but a smooth one - neighbouring lanes read neighbouring
//                       source pixels, the four taps of a lane share cache lines with its neighbours' - so the source crosses the
//                       memory bus about once: ~16 B read and 20 B written per pixel with depth.
//   k_frame_pyramid     a workgroup owns a 32 x 32 block of level 0, each of its 256 threads loads one 2 x 2 quad of the five planes
//                       (8-byte loads when the width is even and the planes are 8-byte aligned) and forms the level-1 pixel; levels
//                       2 and 3 are reduced from LDS by 64 and 16 of the threads.  Level 0 is read once for all levels:
//                       20 B read and 20 (1/4 + 1/16 + 1/64) B written per level-0 pixel.  Block origins are multiples of 32, so a
//                       quad of any level never straddles two workgroups.
//
// Every result is a fixed sequence of separately rounded float32 operations, in the order include/gsr.h states:
// tests/frames_reference.py restates them in numpy, bit for bit for both kernels.  No atomics, nothing read back.
#include "gsr_common.h"

// No implicit fma contraction in this file (as in preprocess.hip, exchange.hip and image.hip), and plain operators: the __f*_rn
// intrinsics are inline functions of plain operators that carry the default contraction flags wherever they are called, so
// "fx * xd + cx" built from them came out as one v_fma_f32 - under this pragma or not.
#pragma clang fp contract(off)

namespace {

struct GsrUndistortArgs {
  int Ws, Hs, W, H;
  float fx, fy, cx, cy;       // source K
  float fxt, fyt, cxt, cyt;   // target K
  float k1, k2, p1, p2, k3;
};

template <bool IDENTITY, bool DEPTH>
__global__ __launch_bounds__(256) void k_frame_undistort(GsrUndistortArgs a, const float* __restrict__ src_color,
                                                         const float* __restrict__ src_depth, float* __restrict__ color,
                                                         float* __restrict__ depth, float* __restrict__ mask) {
  const int u = (int)(blockIdx.x * 64u + threadIdx.x), v = (int)(blockIdx.y * 4u + threadIdx.y);
  if (u >= a.W || v >= a.H) return;
  float us, vs;
  if (IDENTITY) {
    us = (float)u;
    vs = (float)v;
  } else {
    const float x = ((float)u - a.cxt) / a.fxt, y = ((float)v - a.cyt) / a.fyt;
    const float x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
    const float rho = 1.0f + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
    const float xd = (x * rho + (2.0f * a.p1) * xy) + a.p2 * (r2 + 2.0f * x2);
    const float yd = (y * rho + a.p1 * (r2 + 2.0f * y2)) + (2.0f * a.p2) * xy;
    us = a.fx * xd + a.cx;
    vs = a.fy * yd + a.cy;
  }
  const size_t plane = (size_t)a.H * a.W, pix = (size_t)v * a.W + u;
  // (a NaN coordinate fails every comparison: outside)
  const bool inside = us >= 0.0f && us <= (float)(a.Ws - 1) && vs >= 0.0f && vs <= (float)(a.Hs - 1);
  if (!inside) {
    color[pix] = 0.0f;
    color[plane + pix] = 0.0f;
    color[2 * plane + pix] = 0.0f;
    if (DEPTH) depth[pix] = 0.0f;
    mask[pix] = 0.0f;
    return;
  }
  // 0 <= us <= Ws - 1 from here on: floor and ceil are pixel indices of the source, and so is floor(us + 0.5)
  const float x0f = floorf(us), y0f = floorf(vs);
  const float ax = us - x0f, ay = vs - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const int x1 = x0 + (ax > 0.0f ? 1 : 0), y1 = y0 + (ay > 0.0f ? 1 : 0);
  const size_t splane = (size_t)a.Hs * a.Ws;
  const size_t r0 = (size_t)y0 * a.Ws, r1 = (size_t)y1 * a.Ws;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float* __restrict__ s = src_color + ch * splane;
    const float c00 = s[r0 + x0], c01 = s[r0 + x1], c10 = s[r1 + x0], c11 = s[r1 + x1];
    const float top = c00 + ax * (c01 - c00);
    const float bot = c10 + ax * (c11 - c10);
    color[ch * plane + pix] = top + ay * (bot - top);
  }
  if (DEPTH) {
    const int xn = (int)floorf(us + 0.5f), yn = (int)floorf(vs + 0.5f);
    depth[pix] = src_depth[(size_t)yn * a.Ws + xn];
  }
  mask[pix] = 1.0f;
}

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------
#define PYR_PLANES 5      // colour 0..2, depth, mask

struct GsrPyramidArgs {
  int W[4], H[4];         // sizes of levels 0 .. 3 (0 beyond `levels`)
  int levels;
  float band1;            // 1 + depth_band, rounded once
  const float* color;
  const float* depth;
  const float* mask;
  float* color_out[3];
  float* depth_out[3];
  float* mask_out[3];
};

__device__ __forceinline__ float pyr_color(float a, float b, float c, float d) {
  return ((a + b) + (c + d)) * 0.25f;
}

// the mean of the valid (> 0 and finite) readings within the band of the smallest valid one, summed in the order a, b, c, d
__device__ __forceinline__ float pyr_depth(float a, float b, float c, float d, float band1) {
  const float big = __builtin_inff();
  const float m = fminf(fminf(a > 0.0f ? a : big, b > 0.0f ? b : big), fminf(c > 0.0f ? c : big, d > 0.0f ? d : big));
  if (!(m < big)) return 0.0f;      // no valid reading: none > 0, or only +inf ones
  // (a product that overflows takes every finite reading, and still no +inf one: +inf never enters a mean)
  const float lim = fminf(m * band1, 3.402823466e+38f);
  float sum = 0.0f, n = 0.0f;
  if (a > 0.0f && a <= lim) { sum = sum + a; n += 1.0f; }
  if (b > 0.0f && b <= lim) { sum = sum + b; n += 1.0f; }
  if (c > 0.0f && c <= lim) { sum = sum + c; n += 1.0f; }
  if (d > 0.0f && d <= lim) { sum = sum + d; n += 1.0f; }
  return sum / n;                    // (n >= 1: the smallest reading is within its own band)
}

__device__ __forceinline__ float pyr_mask(float a, float b, float c, float d) {
  return (a == 1.0f && b == 1.0f && c == 1.0f && d == 1.0f) ? 1.0f : 0.0f;
}

template <bool VEC>
__device__ __forceinline__ void pyr_load2(const float* __restrict__ p, float& lo, float& hi) {
  if (VEC) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    lo = v.x;
    hi = v.y;
  } else {
    lo = p[0];
    hi = p[1];
  }
}

// one quad of plane `k` held in LDS (side `S` of the finer level's block) -> the coarser pixel
template <int S>
__device__ __forceinline__ float pyr_reduce(const float (*s)[S][S], int k, int y, int x, float band1) {
  const float a = s[k][2 * y][2 * x], b = s[k][2 * y][2 * x + 1], c = s[k][2 * y + 1][2 * x], d = s[k][2 * y + 1][2 * x + 1];
  return k < 3 ? pyr_color(a, b, c, d) : (k == 3 ? pyr_depth(a, b, c, d, band1) : pyr_mask(a, b, c, d));
}

__device__ __forceinline__ void pyr_store(const GsrPyramidArgs& g, int level /*1..3*/, int X, int Y, const float* v) {
  const int W = g.W[level], H = g.H[level];
  const size_t plane = (size_t)W * H, pix = (size_t)Y * W + X;
  float* __restrict__ co = g.color_out[level - 1];
  co[pix] = v[0];
  co[plane + pix] = v[1];
  co[2 * plane + pix] = v[2];
  if (g.depth) g.depth_out[level - 1][pix] = v[3];
  if (g.mask) g.mask_out[level - 1][pix] = v[4];
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_frame_pyramid(GsrPyramidArgs g) {
  __shared__ float s1[PYR_PLANES][16][16];
  __shared__ float s2[PYR_PLANES][8][8];
  const int t = (int)threadIdx.x, qx = t & 15, qy = t >> 4;
  const int X1 = (int)blockIdx.x * 16 + qx, Y1 = (int)blockIdx.y * 16 + qy;
  float v[PYR_PLANES] = {0.f, 0.f, 0.f, 0.f, 0.f};
  // level 1 from global memory: the quad (2 X1 .. 2 X1 + 1, 2 Y1 .. 2 Y1 + 1) lies inside level 0 whenever (X1, Y1) lies inside level 1
  const bool in1 = X1 < g.W[1] && Y1 < g.H[1];
  if (in1) {
    const int W0 = g.W[0];
    const size_t plane0 = (size_t)W0 * g.H[0], top = (size_t)(2 * Y1) * W0 + 2 * X1;
    float a, b, c, d;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      pyr_load2<VEC>(g.color + ch * plane0 + top, a, b);
      pyr_load2<VEC>(g.color + ch * plane0 + top + W0, c, d);
      v[ch] = pyr_color(a, b, c, d);
    }
    if (g.depth) {
      pyr_load2<VEC>(g.depth + top, a, b);
      pyr_load2<VEC>(g.depth + top + W0, c, d);
      v[3] = pyr_depth(a, b, c, d, g.band1);
    }
    if (g.mask) {
      pyr_load2<VEC>(g.mask + top, a, b);
      pyr_load2<VEC>(g.mask + top + W0, c, d);
      v[4] = pyr_mask(a, b, c, d);
    }
    pyr_store(g, 1, X1, Y1, v);
  }
  if (g.levels < 2) return;         // (uniform over the launch)
#pragma unroll
  for (int k = 0; k < PYR_PLANES; k++) s1[k][qy][qx] = v[k];      // (zeros outside level 1: never part of a quad that is kept)
  __syncthreads();
  // level 2: 8 x 8 per workgroup, the first wave
  const int x2 = t & 7, y2 = (t >> 3) & 7;
  const int X2 = (int)blockIdx.x * 8 + x2, Y2 = (int)blockIdx.y * 8 + y2;
  if (t < 64) {
#pragma unroll
    for (int k = 0; k < PYR_PLANES; k++) v[k] = pyr_reduce<16>(s1, k, y2, x2, g.band1);
    if (X2 < g.W[2] && Y2 < g.H[2]) pyr_store(g, 2, X2, Y2, v);
    if (g.levels >= 3) {
#pragma unroll
      for (int k = 0; k < PYR_PLANES; k++) s2[k][y2][x2] = v[k];
    }
  }
  if (g.levels < 3) return;
  __syncthreads();
  // level 3: 4 x 4 per workgroup
  if (t < 16) {
    const int x3 = t & 3, y3 = t >> 2;
    const int X3 = (int)blockIdx.x * 4 + x3, Y3 = (int)blockIdx.y * 4 + y3;
#pragma unroll
    for (int k = 0; k < PYR_PLANES; k++) v[k] = pyr_reduce<8>(s2, k, y3, x3, g.band1);
    if (X3 < g.W[3] && Y3 < g.H[3]) pyr_store(g, 3, X3, Y3, v);
  }
}

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

inline bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; i++)
    if (!(fabsf(p[i]) <= 3.0e38f)) return false;
  return true;
}

}  // namespace

extern "C" int gsr_frame_undistort(int32_t src_w, int32_t src_h, const float* src_color, const float* src_depth,
                                   const float* src_K, const float* dist, int32_t w, int32_t h, const float* K, float* color,
                                   float* depth, float* mask, void* stream) {
  if (!src_color || !src_K || !dist || !color || !mask || (src_depth && !depth) || src_w < 1 || src_h < 1 || w < 1 || h < 1 ||
      (int64_t)src_w * src_h > 0x3FFFFFFF || (int64_t)w * h > 0x3FFFFFFF) {
    gsr_set_error("frame_undistort: bad arguments (source %d x %d, target %d x %d)", (int)src_w, (int)src_h, (int)w, (int)h);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const float* Kt = K ? K : src_K;
  if (!finite_all(src_K, 4) || !finite_all(Kt, 4) || !finite_all(dist, 5) || !(src_K[0] > 0.f) || !(src_K[1] > 0.f) ||
      !(Kt[0] > 0.f) || !(Kt[1] > 0.f)) {
    gsr_set_error("frame_undistort: intrinsics or distortion coefficients not finite, or a focal length <= 0");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  GsrUndistortArgs a;
  a.Ws = src_w; a.Hs = src_h; a.W = w; a.H = h;
  a.fx = src_K[0]; a.fy = src_K[1]; a.cx = src_K[2]; a.cy = src_K[3];
  a.fxt = Kt[0]; a.fyt = Kt[1]; a.cxt = Kt[2]; a.cyt = Kt[3];
  a.k1 = dist[0]; a.k2 = dist[1]; a.p1 = dist[2]; a.p2 = dist[3]; a.k3 = dist[4];
  bool identity = true;
  for (int i = 0; i < 5; i++) identity = identity && dist[i] == 0.f;
  for (int i = 0; i < 4; i++) identity = identity && Kt[i] == src_K[i];
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), block(64, 4);
  if (identity && src_depth)
    GSR_LAUNCH("frame_undistort", (k_frame_undistort<true, true>), grid, block, 0, st, a, src_color, src_depth, color, depth, mask);
  else if (identity)
    GSR_LAUNCH("frame_undistort", (k_frame_undistort<true, false>), grid, block, 0, st, a, src_color, src_depth, color, depth, mask);
  else if (src_depth)
    GSR_LAUNCH("frame_undistort", (k_frame_undistort<false, true>), grid, block, 0, st, a, src_color, src_depth, color, depth, mask);
  else
    GSR_LAUNCH("frame_undistort", (k_frame_undistort<false, false>), grid, block, 0, st, a, src_color, src_depth, color, depth, mask);
  return gsr_launch_status("frame_undistort launch");
}

extern "C" int gsr_frame_pyramid(int32_t w, int32_t h, int32_t levels, const float* color, const float* depth, const float* mask,
                                 float depth_band, float* const* color_out, float* const* depth_out, float* const* mask_out,
                                 void* stream) {
  if (levels < 1 || levels > 3 || w < 1 || h < 1 || (int64_t)w * h > 0x3FFFFFFF || !color || !color_out || (depth && !depth_out) ||
      (mask && !mask_out) || !(depth_band >= 0.f) || !(depth_band <= 3.0e38f)) {
    gsr_set_error("frame_pyramid: bad arguments (%d x %d, %d levels)", (int)w, (int)h, (int)levels);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if ((w >> levels) < 1 || (h >> levels) < 1) {
    gsr_set_error("frame_pyramid: level %d of a %d x %d image has no pixels", (int)levels, (int)w, (int)h);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  GsrPyramidArgs g;
  g.levels = levels;
  g.band1 = 1.0f + depth_band;
  g.color = color; g.depth = depth; g.mask = mask;
  g.W[0] = w; g.H[0] = h;
  for (int l = 1; l <= 3; l++) {
    g.W[l] = l <= levels ? g.W[l - 1] / 2 : 0;
    g.H[l] = l <= levels ? g.H[l - 1] / 2 : 0;
    const bool on = l <= levels;
    g.color_out[l - 1] = on ? color_out[l - 1] : nullptr;
    g.depth_out[l - 1] = on && depth ? depth_out[l - 1] : nullptr;
    g.mask_out[l - 1] = on && mask ? mask_out[l - 1] : nullptr;
    if (on && (!g.color_out[l - 1] || (depth && !g.depth_out[l - 1]) || (mask && !g.mask_out[l - 1]))) {
      gsr_set_error("frame_pyramid: output of level %d is NULL", l);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  // one workgroup per 32 x 32 block of level 0 that holds a level-1 pixel
  const dim3 grid((unsigned)((g.W[1] + 15) / 16), (unsigned)((g.H[1] + 15) / 16)), block(256);
  const bool vec = (w & 1) == 0 && aligned8(color) && aligned8(depth) && aligned8(mask);
  if (vec)
    GSR_LAUNCH("frame_pyramid", k_frame_pyramid<true>, grid, block, 0, st, g);
  else
    GSR_LAUNCH("frame_pyramid", k_frame_pyramid<false>, grid, block, 0, st, g);
  return gsr_launch_status("frame_pyramid launch");
}
