// odometry.hip - dense frame-to-frame RGB-D odometry on the pixel grid: the hybrid photometric + depth term of Steinbruecker et
// al. 2011 / Park et al. 2017 (what Open3D offers as compute_rgbd_odometry with the hybrid Jacobian).  The image-grid sibling of
// the coloured ICP of registration.hip: the same 6-unknown Gauss-Newton step, the same summation and the same final kernel
// (gsr_block_sum_store, k_gn6_final of solve6_common.h), and the association by projection instead of by search.
//
// gsr_odometry_prepare: ONE launch, a workgroup = a 32 x 8 tile of pixels.  Every thread forms the intensity and the validated
//   depth of its pixel (and, 340 cells over 256 threads, of the one-pixel halo) into two LDS planes; the centre cells are written
//   out, and with `grad_out` the four Sobel planes are taken from LDS.  All float32, every operation rounded on its own
//   (tests/odometry_reference.py restates it in numpy, bit for bit).  Invalid pixels are NaN and spread into the gradients by IEEE
//   arithmetic alone: no validity branch in the stencil.  12 + 4 (+ 4 mask) B read, 8 + 16 B written per pixel.
//
// gsr_odometry_update: <= 256 workgroups over fixed slices of the row-major pixel index; per source pixel the warp, the tests, the
//   two residuals and their Jacobians in float64 in the order include/gsr.h states, 30 float64 sums per thread, gsr_block_sum
//   (a fixed butterfly, the wave sums in order), one row of partials per workgroup; then the shared final kernel: one workgroup adds
//   the rows and one thread solves and composes, into a copy that reaches T only with status 0 and `apply`.  No float atomics, nothing read back, no allocation.  Two source planes are streamed and six target
//   planes gathered per pixel; the gather is smooth (neighbouring lanes read neighbouring target pixels).
#include "gsr_common.h"
#include "solve6_common.h"

// No implicit fma contraction in this file, and plain operators (see frames.hip): every product and sum below is rounded on its
// own, which is what lets a numpy restatement give the same n, the same association and, for prepare, the same bits.
#pragma clang fp contract(off)

#define GSR_ODO_TILE_W 32
#define GSR_ODO_TILE_H 8
#define GSR_ODO_H 3                                // n, sum r_D^2, sum r_I^2 (both unweighted)
#define GSR_ODO_SUMS (GSR_ODO_H + GSR_GN6_TERMS)   // ... J^T r [6], upper triangle of J^T J [21]
// (the workspace: gn_ws(.., GSR_ODO_SUMS, false) of solve6_common.h - the rows of partial sums, no shift)

namespace {

inline bool odo_bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)w * h > 0x3FFFFFFF; }

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_odometry_prepare(int w, int h, uint32_t tiles_x, const float* __restrict__ color,
                                                          const float* __restrict__ depth, const float* __restrict__ mask,
                                                          float depth_min, float depth_max, float* __restrict__ intensity_out,
                                                          float* __restrict__ depth_out, float* __restrict__ grad_out) {
  __shared__ float sI[GSR_ODO_TILE_H + 2][GSR_ODO_TILE_W + 2], sD[GSR_ODO_TILE_H + 2][GSR_ODO_TILE_W + 2];
  const float nan = __builtin_nanf("");
  const int x0 = (int)(blockIdx.x % tiles_x) * GSR_ODO_TILE_W, y0 = (int)(blockIdx.x / tiles_x) * GSR_ODO_TILE_H;
  const size_t plane = (size_t)w * h;
  for (int c = (int)threadIdx.x; c < (GSR_ODO_TILE_H + 2) * (GSR_ODO_TILE_W + 2); c += 256) {
    const int ly = c / (GSR_ODO_TILE_W + 2), lx = c % (GSR_ODO_TILE_W + 2);
    const int gx = x0 + lx - 1, gy = y0 + ly - 1;
    const bool centre = lx >= 1 && lx <= GSR_ODO_TILE_W && ly >= 1 && ly <= GSR_ODO_TILE_H;
    if (!grad_out && !centre) continue;      // (the source frame: no stencil, no halo)
    float I = nan, D = nan;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t pix = (size_t)gy * w + gx;
      const bool seen = !mask || mask[pix] == 1.0f;
      if (seen) {
        I = ((color[pix] + color[plane + pix]) + color[2 * plane + pix]) / 3.0f;
        const float d = depth[pix];
        if (knn_finite(d) && d > depth_min && d <= depth_max) D = d;
      }
      if (centre) {
        intensity_out[pix] = I;
        depth_out[pix] = D;
      }
    }
    sI[ly][lx] = I;
    sD[ly][lx] = D;
  }
  if (!grad_out) return;      // (uniform over the launch)
  __syncthreads();
  const int tx = (int)threadIdx.x % GSR_ODO_TILE_W, ty = (int)threadIdx.x / GSR_ODO_TILE_W;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= w || y >= h) return;
  const size_t pix = (size_t)y * w + x;
  float g[4] = {nan, nan, nan, nan};
  if (x > 0 && y > 0 && x < w - 1 && y < h - 1) {      // (inside: all nine taps are pixels of the image, and cells of this tile)
    const int lx = tx + 1, ly = ty + 1;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const float (*s)[GSR_ODO_TILE_W + 2] = k == 0 ? sI : sD;
      const float a = s[ly - 1][lx - 1], b = s[ly - 1][lx], c = s[ly - 1][lx + 1];
      const float d = s[ly][lx - 1], f = s[ly][lx + 1];
      const float p = s[ly + 1][lx - 1], q = s[ly + 1][lx], r = s[ly + 1][lx + 1];
      g[2 * k] = (((c - a) + 2.0f * (f - d)) + (r - p)) * 0.125f;
      g[2 * k + 1] = (((p - a) + 2.0f * (q - b)) + (r - c)) * 0.125f;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) grad_out[k * plane + pix] = g[k];
}

// ---- update -------------------------------------------------------------------------------------------------------------------------
struct GsrOdoArgs {
  int w, h;
  double fx, fy, cx, cy;
  double sqrt_d, sqrt_i;      // sqrt(lambda), sqrt(1 - lambda)
  double depth_diff_max;
};

__device__ __forceinline__ bool odo_finite(double v) { return fabs(v) < (double)KNN_INF; }

// per workgroup: s[0] = n, s[1] = sum r_D^2 (0 with lambda = 0), s[2] = sum r_I^2 (0 with lambda = 1), s[3..8] = J^T r, s[9..29] =
// J^T J rows 0 .. 5 from the diagonal on, r and J over both residuals
__global__ __launch_bounds__(256) void k_odometry_partial(GsrOdoArgs A, const float* __restrict__ src_intensity,
                                                          const float* __restrict__ src_depth,
                                                          const float* __restrict__ tgt_intensity,
                                                          const float* __restrict__ tgt_depth, const float* __restrict__ tgt_grad,
                                                          const double* __restrict__ T_dev, double* __restrict__ part) {
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = T_dev[i];
  const uint32_t N = (uint32_t)A.w * (uint32_t)A.h;      // (<= 2^30 - 1)
  const size_t plane = (size_t)N;
  const double wmax = (double)(A.w - 1), hmax = (double)(A.h - 1);
  double s[GSR_ODO_SUMS];
#pragma unroll
  for (int a = 0; a < GSR_ODO_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < N; i += gridDim.x * 256u) {
    const float df = src_depth[i], isf = src_intensity[i];
    if (!(knn_finite(df) && knn_finite(isf))) continue;
    const double d = (double)df, x = (double)(i % (uint32_t)A.w), y = (double)(i / (uint32_t)A.w);
    const double P[3] = {d * ((x - A.cx) / A.fx), d * ((y - A.cy) / A.fy), d};
    double Q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) Q[k] = ((T[4 * k] * P[0] + T[4 * k + 1] * P[1]) + T[4 * k + 2] * P[2]) + T[4 * k + 3];
    if (!(odo_finite(Q[2]) && Q[2] > 0.0)) continue;
    const double u = A.fx * (Q[0] / Q[2]) + A.cx, v = A.fy * (Q[1] / Q[2]) + A.cy;
    const double ui = floor(u + 0.5), vi = floor(v + 0.5);
    // (compared as doubles: NaN, +-inf and anything beyond an int fail here, before the conversion)
    if (!(ui >= 0.0 && ui <= wmax && vi >= 0.0 && vi <= hmax)) continue;
    const size_t j = (size_t)(uint32_t)vi * (uint32_t)A.w + (uint32_t)ui;      // (< N)
    const float dtf = tgt_depth[j], itf = tgt_intensity[j];
    const float g0 = tgt_grad[j], g1 = tgt_grad[plane + j], g2 = tgt_grad[2 * plane + j], g3 = tgt_grad[3 * plane + j];
    if (!(knn_finite(dtf) && knn_finite(itf) && knn_finite(g0) && knn_finite(g1) && knn_finite(g2) && knn_finite(g3))) continue;
    const double rD = (double)dtf - Q[2];
    if (!(fabs(rD) <= A.depth_diff_max)) continue;
    const double rI = (double)itf - (double)isf;
    const double a = A.fx / Q[2], b = A.fy / Q[2];
    // c = the residual's gradient with respect to Q: (g_x fx / Qz, g_y fy / Qz, -(c_0 Qx + c_1 Qy) / Qz [- 1 for the depth term])
    const double cD0 = (double)g2 * a, cD1 = (double)g3 * b;
    const double cD[3] = {cD0, cD1, -((cD0 * Q[0] + cD1 * Q[1]) / Q[2]) - 1.0};
    const double cI0 = (double)g0 * a, cI1 = (double)g1 * b;
    const double cI[3] = {cI0, cI1, -((cI0 * Q[0] + cI1 * Q[1]) / Q[2])};
    const double JD[6] = {A.sqrt_d * (Q[1] * cD[2] - Q[2] * cD[1]), A.sqrt_d * (Q[2] * cD[0] - Q[0] * cD[2]),
                          A.sqrt_d * (Q[0] * cD[1] - Q[1] * cD[0]), A.sqrt_d * cD[0], A.sqrt_d * cD[1], A.sqrt_d * cD[2]};
    const double JI[6] = {A.sqrt_i * (Q[1] * cI[2] - Q[2] * cI[1]), A.sqrt_i * (Q[2] * cI[0] - Q[0] * cI[2]),
                          A.sqrt_i * (Q[0] * cI[1] - Q[1] * cI[0]), A.sqrt_i * cI[0], A.sqrt_i * cI[1], A.sqrt_i * cI[2]};
    const double rd = A.sqrt_d * rD, ri = A.sqrt_i * rI;
    s[0] += 1.0;
    s[1] += A.sqrt_d > 0.0 ? rD * rD : 0.0;
    s[2] += A.sqrt_i > 0.0 ? rI * rI : 0.0;
    int o = 9;
#pragma unroll
    for (int p = 0; p < 6; p++) {
      s[3 + p] += JD[p] * rd + JI[p] * ri;
#pragma unroll
      for (int q = p; q < 6; q++) s[o++] += JD[p] * JD[q] + JI[p] * JI[q];
    }
  }
  gsr_block_sum_store(s, part);
}

// (the final kernel: k_gn6_final of solve6_common.h, about the origin - camera coordinates - and with the caller's `apply`)

inline bool finite_d(double v) { return fabs(v) <= 1.7e308; }      // false for NaN and +-inf

}  // namespace

extern "C" int gsr_odometry_prepare(int32_t w, int32_t h, const float* color, const float* depth, const float* mask,
                                    float depth_min, float depth_max, float* intensity_out, float* depth_out, float* grad_out,
                                    void* stream) {
  if (!color || !depth || !intensity_out || !depth_out || odo_bad_image(w, h) || depth_min != depth_min ||
      depth_max != depth_max || !(depth_max > depth_min)) {
    gsr_set_error("odometry_prepare: bad arguments (%d x %d, depth range (%g, %g])", (int)w, (int)h, (double)depth_min,
                  (double)depth_max);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const uint32_t tiles_x = ((uint32_t)w + GSR_ODO_TILE_W - 1) / GSR_ODO_TILE_W;
  const uint32_t tiles_y = ((uint32_t)h + GSR_ODO_TILE_H - 1) / GSR_ODO_TILE_H;
  // (w h < 2^30 and a tile covers at least min(w, 32) min(h, 8) of them: the product stays below 2^31)
  GSR_LAUNCH("odometry_prepare", k_odometry_prepare, dim3(tiles_x * tiles_y), dim3(256), 0, (hipStream_t)stream, (int)w, (int)h,
             tiles_x, color, depth, mask, depth_min, depth_max, intensity_out, depth_out, grad_out);
  return gsr_launch_status("odometry_prepare launch");
}

extern "C" size_t gsr_odometry_workspace_bytes(int32_t w, int32_t h) {
  (void)w;
  (void)h;      // (the partial sums of at most GSR_GN_BLOCKS workgroups: the size does not grow with the image)
  return gn_ws(nullptr, GSR_ODO_SUMS, false).total;
}

extern "C" int gsr_odometry_update(int32_t w, int32_t h, const double* K, const float* src_intensity, const float* src_depth,
                                   const float* tgt_intensity, const float* tgt_depth, const float* tgt_grad,
                                   double lambda_geometric, double depth_diff_max, int32_t apply, double* T_dev, double* stats_dev,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!K || !src_intensity || !src_depth || !tgt_intensity || !tgt_depth || !tgt_grad || !T_dev || !stats_dev || !workspace ||
      odo_bad_image(w, h)) {
    gsr_set_error("odometry_update: bad arguments (%d x %d, or a NULL pointer)", (int)w, (int)h);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!(finite_d(K[0]) && finite_d(K[1]) && finite_d(K[2]) && finite_d(K[3]) && K[0] > 0.0 && K[1] > 0.0) ||
      !(lambda_geometric >= 0.0 && lambda_geometric <= 1.0) || !(depth_diff_max > 0.0)) {
    gsr_set_error("odometry_update: bad arguments (K = %g %g %g %g: expected finite, fx, fy > 0; lambda_geometric = %g: expected "
                  "0 .. 1; depth_diff_max = %g: expected > 0)", K[0], K[1], K[2], K[3], lambda_geometric, depth_diff_max);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrGnWs ws = gn_ws(workspace, GSR_ODO_SUMS, false);
  if (!gsr_workspace_fits("odometry_update", workspace, workspace_bytes, ws.total)) return GSR_ERR_STATE_TOO_SMALL;
  GsrOdoArgs A;
  A.w = w; A.h = h;
  A.fx = K[0]; A.fy = K[1]; A.cx = K[2]; A.cy = K[3];
  A.sqrt_d = sqrt(lambda_geometric);
  A.sqrt_i = sqrt(1.0 - lambda_geometric);
  A.depth_diff_max = depth_diff_max;
  hipStream_t st = (hipStream_t)stream;
  double* part = ws.part;
  const uint32_t N = (uint32_t)w * (uint32_t)h, sblk = gn_partial_blocks(N);
  GSR_LAUNCH("odometry_partial", k_odometry_partial, dim3(sblk), dim3(256), 0, st, A, src_intensity, src_depth, tgt_intensity,
             tgt_depth, tgt_grad, (const double*)T_dev, part);
  GSR_LAUNCH("odometry_final", k_gn6_final<GSR_ODO_H>, dim3(1), dim3(256), 0, st, sblk, (double)N, (int)apply, (const double*)part,
             (const double*)nullptr, T_dev, stats_dev);
  return gsr_launch_status("odometry_update launch");
}
