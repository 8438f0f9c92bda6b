// cloud_image.hip - a LiDAR cloud seen by the colour camera: the step that joins the two sensors of a /Visual_Merged message
// (Image + Local_Map).  The cloud is projected into the image with a z-buffer and a square occlusion footprint - a sparse depth
// image, the row that won each pixel, which rows the camera sees, the image's colour for them - and the sparse depth is filled
// into a dense one with a foreground-preferring window.  The reference has the message field and no code for this step; the
// rules are this library's own and are stated in include/gsr.h (gsr_cloud_project, gsr_depth_densify).
//
// Project, data path.  k_cloud_clear fills the two per-pixel buffers of the workspace - zocc, uint32, the occlusion depth, and win,
// uint64, (z bits << 32) | row of the nearest candidate - with all ones, above every key, and zeroes the two counts.
// k_cloud_project takes 256 consecutive rows per workgroup: their 768 floats are one contiguous span, brought into LDS with
// coalesced dword loads and read back at stride 3 (coprime to the bank count: no conflicts); each lane transforms and projects
// its row, then lowers zocc over its footprint and win at its centre pixel.  Every atomic is preceded by a relaxed read of the
// word (device scope: it is served by the L2, where the atomics land) and skipped when that is already <= the lane's value: the
// minimum only ever falls, so an old value can only cause an atomic that was not needed, never lose one, and most of a dense
// scan's footprint traffic stays out of the L2's atomic units.
// k_cloud_resolve_points compares each candidate with the finished zocc (visible, colour, the two counts: one ballot per wave,
// one integer atomic per count and workgroup); k_cloud_resolve_pixels decodes win into depth and index, lane t at pixel
// p0 + t: full-wave contiguous loads and stores.  Integer atomics only.
//
// Densify.  A workgroup is a 32 x 8 pixel tile; the tile and a halo of `radius` (at most 48 x 24 floats) are staged in LDS, a
// pixel outside the image as 0 = no reading.  A wave is two tile rows of 32 consecutive LDS words each.  A tile whose staged
// window holds no reading writes zeros and leaves.
#include "gsr_common.h"

// Every rule is a sequence of separately rounded operations and the tests compare bits: no implicit fma contraction in this
// file, and plain operators instead of the __f*_rn intrinsics (see image.hip).
#pragma clang fp contract(off)

#define CLD_BLOCK 256
#define CLD_UNTOUCHED 0xFFFFFFFFu                        // above the bits of every positive float
#define CLD_NO_WINNER 0xFFFFFFFFFFFFFFFFull
#define DNS_TILE_W 32
#define DNS_TILE_H 8
#define DNS_LDS_W (DNS_TILE_W + 2 * GSR_DENSIFY_MAX_RADIUS)
#define DNS_LDS_H (DNS_TILE_H + 2 * GSR_DENSIFY_MAX_RADIUS)

struct CloudArgs {
  int32_t W, H;
  float fx, fy, cx, cy;
  double T[12];
  float z_near, z_far;
  int32_t r;
  float occ_scale;
  uint32_t N;
};

// "q = w2c p" of include/gsr.h: image.hip's dreg_apply, operation for operation
__device__ __forceinline__ float3 cld_apply(const double* T, float x, float y, float z) {
  float q[3];
  const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double a = T[4 * i] * dx + T[4 * i + 1] * dy;
    q[i] = (float)((a + T[4 * i + 2] * dz) + T[4 * i + 3]);
  }
  return make_float3(q[0], q[1], q[2]);
}
__device__ __forceinline__ bool cld_finite(float v) { return fabsf(v) < INFINITY; }      // (false for NaN)
__device__ __forceinline__ bool cld_takes_part(const CloudArgs& A, const float3& q) {
  return cld_finite(q.x) && cld_finite(q.y) && cld_finite(q.z) && q.z >= A.z_near && q.z <= A.z_far;
}
// floor(p + 0.5) clamped in float to [-(r + 1), S + r], then an int
__device__ __forceinline__ int cld_round(float p, int S, int r) {
  return (int)fminf(fmaxf(floorf((p + 0.5f)), -(float)(r + 1)), (float)(S + r));
}

__global__ __launch_bounds__(CLD_BLOCK) void k_cloud_clear(uint32_t n, uint32_t* __restrict__ zocc,
                                                           unsigned long long* __restrict__ win,
                                                           unsigned long long* __restrict__ count) {
  const uint32_t i = blockIdx.x * (uint32_t)CLD_BLOCK + threadIdx.x;
  if (i < 2u) count[i] = 0ull;
  if (i < n) {
    zocc[i] = CLD_UNTOUCHED;
    win[i] = CLD_NO_WINNER;
  }
}

__global__ __launch_bounds__(CLD_BLOCK) void k_cloud_project(const CloudArgs A, const float* __restrict__ points,
                                                             const float* __restrict__ mask, uint32_t* __restrict__ zocc,
                                                             unsigned long long* __restrict__ win, int32_t* __restrict__ pixel,
                                                             float* __restrict__ zout) {
  __shared__ float sh[3 * CLD_BLOCK];
  const uint32_t t = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * (size_t)(3 * CLD_BLOCK), total = 3 * (size_t)A.N;
#pragma unroll
  for (uint32_t k = 0; k < 3u; k++) {
    const size_t g = first + t + k * (uint32_t)CLD_BLOCK;
    sh[t + k * (uint32_t)CLD_BLOCK] = g < total ? points[g] : 0.f;
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * (uint32_t)CLD_BLOCK + t;
  if (i >= A.N) return;
  const float3 q = cld_apply(A.T, sh[3u * t], sh[3u * t + 1u], sh[3u * t + 2u]);
  if (!cld_takes_part(A, q)) {
    zout[i] = 0.f;
    pixel[i] = -1;
    return;
  }
  const float px = ((A.fx * (q.x / q.z)) + A.cx);
  const float py = ((A.fy * (q.y / q.z)) + A.cy);
  const int u = cld_round(px, A.W, A.r), v = cld_round(py, A.H, A.r);
  const uint32_t zb = __float_as_uint(q.z);
  const int x0 = u - A.r < 0 ? 0 : u - A.r, x1 = u + A.r > A.W - 1 ? A.W - 1 : u + A.r;
  const int y0 = v - A.r < 0 ? 0 : v - A.r, y1 = v + A.r > A.H - 1 ? A.H - 1 : v + A.r;
  for (int yy = y0; yy <= y1; yy++) {      // (empty when the footprint misses the image: x0 > x1 or y0 > y1)
    for (int xx = x0; xx <= x1; xx++) {
      uint32_t* cell = &zocc[(size_t)yy * A.W + xx];
      if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > zb) atomicMin(cell, zb);
    }
  }
  int32_t p = -1;
  if (u >= 0 && u < A.W && v >= 0 && v < A.H) {
    const int32_t at = v * A.W + u;
    if (!mask || mask[at] != 0.f) {
      p = at;
      const unsigned long long key = ((unsigned long long)zb << 32) | (unsigned long long)i;
      unsigned long long* cell = &win[at];
      if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(cell, key);
    }
  }
  zout[i] = q.z;
  pixel[i] = p;
}

// the bilinear sample of one channel plane at (tx, ty) between the four clamped taps: horizontal lerps, then the vertical one
__device__ __forceinline__ float cld_bilinear(const float* __restrict__ plane, int W, int xa, int xb, int ya, int yb, float tx,
                                              float ty) {
  const float a = plane[(size_t)ya * W + xa], b = plane[(size_t)ya * W + xb];
  const float c = plane[(size_t)yb * W + xa], d = plane[(size_t)yb * W + xb];
  const float top = (a + (tx * (b - a)));
  const float bot = (c + (tx * (d - c)));
  return (top + (ty * (bot - top)));
}

__global__ __launch_bounds__(CLD_BLOCK) void k_cloud_resolve_points(const CloudArgs A, const float* __restrict__ points,
                                                                    const float* __restrict__ image,
                                                                    const uint32_t* __restrict__ zocc,
                                                                    const int32_t* __restrict__ pixel, const float* __restrict__ zin,
                                                                    uint8_t* __restrict__ visible, float* __restrict__ colors,
                                                                    unsigned long long* __restrict__ count) {
  __shared__ uint32_t wave_cnt[2][CLD_BLOCK / GSR_WAVE];
  const uint32_t t = threadIdx.x;
  const uint32_t i = blockIdx.x * (uint32_t)CLD_BLOCK + t;
  bool cand = false, vis = false;
  if (i < A.N) {
    const int32_t p = pixel[i];
    cand = p >= 0;
    if (cand) vis = zin[i] <= (__uint_as_float(zocc[p]) * A.occ_scale);      // (a candidate lowered zocc[p] itself: never untouched)
    visible[i] = vis ? (uint8_t)1 : (uint8_t)0;
    if (vis && colors) {
      // the row's pixel position again, by the operations of k_cloud_project: the same bits
      const float3 q = cld_apply(A.T, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
      const float px = ((A.fx * (q.x / q.z)) + A.cx);
      const float py = ((A.fy * (q.y / q.z)) + A.cy);
      const float fx0 = floorf(px), fy0 = floorf(py);
      const float tx = (px - fx0), ty = (py - fy0);
      // (a visible row's centre pixel is inside the image: px in [-0.5, W - 0.5), the int conversions are exact)
      const int xl = (int)fx0, yl = (int)fy0;
      const int xa = xl < 0 ? 0 : xl, xb = xl + 1 > A.W - 1 ? A.W - 1 : xl + 1;
      const int ya = yl < 0 ? 0 : yl, yb = yl + 1 > A.H - 1 ? A.H - 1 : yl + 1;
      const size_t plane = (size_t)A.W * (size_t)A.H;
#pragma unroll
      for (int c = 0; c < 3; c++) colors[3 * (size_t)i + c] = cld_bilinear(image + c * plane, A.W, xa, xb, ya, yb, tx, ty);
    }
  }
  const uint32_t nv = (uint32_t)__popcll(__ballot(vis)), nc = (uint32_t)__popcll(__ballot(cand));
  if (gsr_lane() == 0) {
    wave_cnt[0][t >> 6] = nv;
    wave_cnt[1][t >> 6] = nc;
  }
  __syncthreads();
  if (t < 2u) {
    const uint32_t s = (wave_cnt[t][0] + wave_cnt[t][1]) + (wave_cnt[t][2] + wave_cnt[t][3]);
    if (s) atomicAdd(&count[t], (unsigned long long)s);
  }
}

__global__ __launch_bounds__(CLD_BLOCK) void k_cloud_resolve_pixels(uint32_t n, float occ_scale, const uint32_t* __restrict__ zocc,
                                                                    const unsigned long long* __restrict__ win,
                                                                    float* __restrict__ depth, int32_t* __restrict__ index) {
  const uint32_t p = blockIdx.x * (uint32_t)CLD_BLOCK + threadIdx.x;
  if (p >= n) return;
  const unsigned long long w = win[p];
  float d = 0.f;
  int32_t row = -1;
  if (w != CLD_NO_WINNER) {
    // the winner has the smallest z of the pixel's candidates and the test is monotone in z: if it fails, every candidate fails
    const float z = __uint_as_float((uint32_t)(w >> 32));
    if (z <= (__uint_as_float(zocc[p]) * occ_scale)) {
      d = z;
      row = (int32_t)(uint32_t)(w & 0xFFFFFFFFull);
    }
  }
  depth[p] = d;
  index[p] = row;
}

// ---- densify ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DNS_TILE_W* DNS_TILE_H) void k_depth_densify(int32_t W, int32_t H, uint32_t tiles_x, int32_t R,
                                                                          float band_scale, int32_t min_neighbors,
                                                                          const float* __restrict__ depth, float* __restrict__ dense,
                                                                          float* __restrict__ valid) {
  __shared__ float sh[DNS_LDS_H * DNS_LDS_W];
  const int t = (int)threadIdx.x;
  const uint32_t tile_y = blockIdx.x / tiles_x;
  const int tx0 = (int)(blockIdx.x - tile_y * tiles_x) * DNS_TILE_W, ty0 = (int)tile_y * DNS_TILE_H;
  const int lw = DNS_TILE_W + 2 * R, lh = DNS_TILE_H + 2 * R;      // the staged window, row stride lw
  int any = 0;
  for (int k = t; k < lw * lh; k += DNS_TILE_W * DNS_TILE_H) {
    const int ly = k / lw, lx = k - ly * lw;
    const int gx = tx0 - R + lx, gy = ty0 - R + ly;
    float d = 0.f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) d = depth[(size_t)gy * W + gx];
    sh[k] = d;
    any |= d > 0.f ? 1 : 0;
  }
  any = __syncthreads_or(any);
  const int lx = t & (DNS_TILE_W - 1), ly = t >> 5;
  const int x = tx0 + lx, y = ty0 + ly;
  if (x >= W || y >= H) return;
  const size_t at = (size_t)y * W + x;
  if (!any) {
    dense[at] = 0.f;
    valid[at] = 0.f;
    return;
  }
  const float own = sh[(ly + R) * lw + lx + R];
  if (own > 0.f) {
    dense[at] = own;
    valid[at] = 1.f;
    return;
  }
  float zn = INFINITY;
  for (int dy = 0; dy <= 2 * R; dy++) {
    const float* rowp = &sh[(ly + dy) * lw + lx];
    for (int dx = 0; dx <= 2 * R; dx++) {
      const float z = rowp[dx];
      if (z > 0.f && z < zn) zn = z;
    }
  }
  float out = 0.f, ok = 0.f;
  if (zn < INFINITY) {
    const float band = (zn * band_scale);
    float sw = 0.f, swz = 0.f;
    int cnt = 0;
    for (int dy = 0; dy <= 2 * R; dy++) {
      const float* rowp = &sh[(ly + dy) * lw + lx];
      const int ey = dy - R;
      for (int dx = 0; dx <= 2 * R; dx++) {
        const float z = rowp[dx];
        if (z > 0.f && z <= band) {      // (never the centre: its reading is not positive)
          const int ex = dx - R;
          const float w = (1.0f / (float)(ex * ex + ey * ey));
          sw = (sw + w);
          swz = (swz + (w * z));
          cnt++;
        }
      }
    }
    if (cnt >= min_neighbors) {
      out = (swz / sw);
      ok = 1.f;
    }
  }
  dense[at] = out;
  valid[at] = ok;
}

// the workspace of gsr_cloud_project: the occlusion z-buffer and the winner keys of the image
struct CloudWs {
  uint32_t* zocc;               // u32[W H]
  unsigned long long* win;      // u64[W H]
  size_t total;
};
static CloudWs cloud_ws(void* base, int32_t W, int32_t H) {
  GsrCarve c(base);
  CloudWs w;
  const size_t n = (size_t)(W < 1 ? 1 : W) * (size_t)(H < 1 ? 1 : H);
  w.zocc = c.take<uint32_t>(n);
  w.win = c.take<unsigned long long>(n);
  w.total = c.o;
  return w;
}

extern "C" {

size_t gsr_cloud_project_workspace_bytes(int32_t W, int32_t H) { return cloud_ws(nullptr, W, H).total; }

int gsr_cloud_project(const gsr_cloud_camera* cam, int64_t N, const float* points, const float* image, const float* mask,
                      float* depth, int32_t* index, int32_t* pixel, float* z, uint8_t* visible, float* colors, int64_t* count_dev,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!cam || !depth || !index || !count_dev || !workspace) {
    gsr_set_error("cloud_project: NULL cam / depth / index / count_dev / workspace");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (N < 0 || N > 0x3FFFFFFFll) {
    gsr_set_error("cloud_project: N = %lld outside [0, 2^30 - 1]", (long long)N);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (N > 0 && (!points || !pixel || !z || !visible)) {
    gsr_set_error("cloud_project: NULL points / pixel / z / visible with N = %lld", (long long)N);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (colors && !image) {
    gsr_set_error("cloud_project: colors without an image to take them from");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const gsr_cloud_camera& c = *cam;
  if (c.width < 1 || c.height < 1 || (long long)c.width * c.height > 0x3FFFFFFFll) {
    gsr_set_error("cloud_project: %d x %d outside [1, 2^30 - 1] pixels", (int)c.width, (int)c.height);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < 4; i++) {
    if (!(fabsf(c.K[i]) < INFINITY) || (i < 2 && !(c.K[i] > 0.f))) {
      gsr_set_error("cloud_project: intrinsics (fx, fy, cx, cy) must be finite, fx and fy positive");
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  for (int i = 0; i < 12; i++) {
    if (!(fabs(c.w2c[i]) < (double)INFINITY)) {
      gsr_set_error("cloud_project: w2c[%d] is not finite", i);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  if (!(c.z_near > 0.f) || !(c.z_near < c.z_far) || !(c.z_far < INFINITY)) {
    gsr_set_error("cloud_project: z_near = %g, z_far = %g (0 < z_near < z_far, finite)", (double)c.z_near, (double)c.z_far);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (c.footprint < 0 || c.footprint > GSR_CLOUD_MAX_FOOTPRINT) {
    gsr_set_error("cloud_project: footprint = %d outside [0, %d]", (int)c.footprint, GSR_CLOUD_MAX_FOOTPRINT);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!(c.occlusion_scale >= 1.f) || !(c.occlusion_scale < INFINITY)) {
    gsr_set_error("cloud_project: occlusion_scale = %g (finite, >= 1)", (double)c.occlusion_scale);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const CloudWs w = cloud_ws(workspace, c.width, c.height);
  if (!gsr_workspace_fits("cloud_project", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  CloudArgs A;
  A.W = c.width; A.H = c.height;
  A.fx = c.K[0]; A.fy = c.K[1]; A.cx = c.K[2]; A.cy = c.K[3];
  for (int i = 0; i < 12; i++) A.T[i] = c.w2c[i];
  A.z_near = c.z_near; A.z_far = c.z_far;
  A.r = c.footprint;
  A.occ_scale = c.occlusion_scale;
  A.N = (uint32_t)N;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t npix = (uint32_t)c.width * (uint32_t)c.height;
  const dim3 pix_grid((npix + CLD_BLOCK - 1u) / CLD_BLOCK), pt_grid((A.N + CLD_BLOCK - 1u) / CLD_BLOCK), block(CLD_BLOCK);
  unsigned long long* count = (unsigned long long*)count_dev;
  GSR_LAUNCH("cloud_project_clear", k_cloud_clear, pix_grid, block, 0, st, npix, w.zocc, w.win, count);
  if (A.N > 0u) {
    GSR_LAUNCH("cloud_project_splat", k_cloud_project, pt_grid, block, 0, st, A, points, mask, w.zocc, w.win, pixel, z);
    GSR_LAUNCH("cloud_project_resolve_points", k_cloud_resolve_points, pt_grid, block, 0, st, A, points, image,
               (const uint32_t*)w.zocc, (const int32_t*)pixel, (const float*)z, visible, colors, count);
  }
  GSR_LAUNCH("cloud_project_resolve_pixels", k_cloud_resolve_pixels, pix_grid, block, 0, st, npix, A.occ_scale,
             (const uint32_t*)w.zocc, (const unsigned long long*)w.win, depth, index);
  return gsr_launch_status("cloud_project launch");
}

int gsr_depth_densify(int32_t W, int32_t H, const float* depth, int32_t radius, float band_scale, int32_t min_neighbors,
                      float* dense, float* valid, void* stream) {
  if (!depth || !dense || !valid || W < 1 || H < 1 || (long long)W * H > 0x3FFFFFFFll) {
    gsr_set_error("depth_densify: bad arguments (NULL depth / dense / valid, or %d x %d outside [1, 2^30 - 1] pixels)", (int)W,
                  (int)H);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (radius < 1 || radius > GSR_DENSIFY_MAX_RADIUS || !(band_scale >= 1.f) || !(band_scale < INFINITY) || min_neighbors < 1) {
    gsr_set_error("depth_densify: radius = %d (1 .. %d), band_scale = %g (finite, >= 1), min_neighbors = %d (>= 1)", (int)radius,
                  GSR_DENSIFY_MAX_RADIUS, (double)band_scale, (int)min_neighbors);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  // one grid axis, tile rows major (W H <= 2^30 - 1: at most 2^30 - 1 tiles)
  const uint32_t tiles_x = (uint32_t)((W + DNS_TILE_W - 1) / DNS_TILE_W), tiles_y = (uint32_t)((H + DNS_TILE_H - 1) / DNS_TILE_H);
  GSR_LAUNCH("depth_densify", k_depth_densify, dim3(tiles_x * tiles_y), dim3(DNS_TILE_W * DNS_TILE_H), 0, (hipStream_t)stream, W, H,
             tiles_x, radius, band_scale, min_neighbors, depth, dense, valid);
  return gsr_launch_status("depth_densify launch");
}

}  // extern "C"
