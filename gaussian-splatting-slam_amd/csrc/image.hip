// image.hip - a sensor_msgs/Image byte buffer decoded on the device: what the reference's imgmsg_to_pli (scene/dataset_readers.py:
// 278-309) does on the host with numpy and PIL for rgb8 / bgr8 / mono8 - here with `step`, `is_bigendian`, the 16-bit, Bayer and
// depth encodings honoured and no JPEG in between; the registration of a depth image into the colour camera (librealsense's
// "align depth to colour"); and the inverse of the decode for publishing a render (train.py:80).  Rules: include/gsr.h.
//
// Decode, data path.  A workgroup of IMG_TILE_W = 256 threads takes IMG_TILE_W consecutive pixels of ONE row, one pixel per
// lane.  Their bytes are one contiguous span of the buffer; the workgroup brings it into LDS with coalesced dword loads - the
// span's start aligned down to the dword of its ADDRESS, a dword that would leave the buffer assembled from guarded byte loads, as
// pointcloud2.hip stages a chunk of points - and every lane picks its pixel's bytes out of LDS (two dword reads and a funnel
// shift per sample, whatever the alignment: 3-byte pixels at an odd address cost the same as aligned ones).  Each output plane
// is then written by lane t at x0 + t: full-wave contiguous stores.  Bayer stages three rows (y - 1, y, y + 1, reflected at the
// image's edge) with one pixel of halo on either side; the rows above and below are re-read by the neighbouring workgroups out of
// the L2 (a 1080p Bayer frame is 2 MB).  The span of a row segment is at most (IMG_TILE_W + 2) * 8 + 3 bytes: it always fits, so
// there is no second path.
//
// Depth registration.  k_dreg_clear fills the workspace (one uint32 per colour pixel) with IMG_UNTOUCHED and clears the status
// word; k_dreg_splat, one lane per depth pixel, projects the reading's two pixel corners and takes atomicMin of the bits of the
// centre's z' over the rectangle between them - positive floats order as their bits, so the result does not depend on the order
// of arrival; k_dreg_finalize turns IMG_UNTOUCHED into 0.  Integer atomics only.
#include "gsr_common.h"

// No implicit fma contraction in this file (as in preprocess.hip): every rule of include/gsr.h is a sequence of separately rounded
// operations, and the tests compare bits.  The __f*_rn / __d*_rn intrinsics do not give that - they are inline functions of plain
// operators that carry the default contraction flags, and "fx * q + cx" built from them comes out as one v_fma_f32 - so the
// arithmetic below is written with plain operators under this pragma, the point transform of rigid_common.h (same operation
// order) included: dreg_apply.
#pragma clang fp contract(off)

#define IMG_TILE_W 256                                   // pixels per workgroup = threads per workgroup (one row segment)
#define IMG_MAX_BPP 8                                    // rgba16 / bgra16
#define IMG_ROW_WORDS (((IMG_TILE_W + 2) * IMG_MAX_BPP + 3 + 3) / 4 + 2)      // a staged row: halo, misalignment, + the dword behind (img_fetch reads two)
#define IMG_UNTOUCHED 0xFFFFFFFFu                        // above the bits of every positive float
#define IMG_DREG_CAP 8                                   // columns / rows of a footprint

enum { IMG_COLOR = 0, IMG_BAYER = 1, IMG_DEPTH = 2 };

struct ImgArgs {
  const uint8_t* data;
  unsigned long long data_bytes;
  uint32_t base_mis;       // (address of data) & 3
  uint32_t W, H, step;
  uint32_t tiles_x;
  uint32_t bpp;            // bytes per pixel
  uint32_t bpc;            // bytes per channel: 1, 2 (4: 32FC1)
  uint32_t off[3];         // byte offset of r, g, b inside a pixel (colour)
  uint32_t rx, ry;         // Bayer: parity of the red site's column and row (blue sits on the other parity of both)
  int32_t be;
  float inv;               // 255 or 65535
  float scale, lo, hi;     // depth
  float* out;
};

struct ImgEnc {
  int mode;
  uint32_t nchan, bpc, ro, go, bo, rx, ry;
};

// the GSR_IMG_* code -> how the kernel reads it; false: no such code
static bool img_encoding(int32_t code, ImgEnc& E) {
  E.rx = E.ry = 0u;
  E.ro = E.go = E.bo = 0u;
  if (code >= GSR_IMG_RGB8 && code <= GSR_IMG_MONO16) {
    const int k = (code - GSR_IMG_RGB8) % 5;      // rgb, bgr, rgba, bgra, mono
    E.mode = IMG_COLOR;
    E.bpc = code >= GSR_IMG_RGB16 ? 2u : 1u;
    E.nchan = k == 4 ? 1u : k >= 2 ? 4u : 3u;
    if (k == 0 || k == 2) { E.ro = 0u; E.go = 1u; E.bo = 2u; }
    if (k == 1 || k == 3) { E.ro = 2u; E.go = 1u; E.bo = 0u; }
    return true;
  }
  if (code >= GSR_IMG_BAYER_RGGB8 && code <= GSR_IMG_BAYER_GRBG16) {
    const int k = (code - GSR_IMG_BAYER_RGGB8) % 4;      // rggb, bggr, gbrg, grbg: red at (0,0), (1,1), (0,1), (1,0)
    E.mode = IMG_BAYER;
    E.bpc = code >= GSR_IMG_BAYER_RGGB16 ? 2u : 1u;
    E.nchan = 1u;
    E.rx = (k == 1 || k == 3) ? 1u : 0u;
    E.ry = (k == 1 || k == 2) ? 1u : 0u;
    return true;
  }
  if (code == GSR_IMG_16UC1 || code == GSR_IMG_32FC1) {
    E.mode = IMG_DEPTH;
    E.bpc = code == GSR_IMG_16UC1 ? 2u : 4u;
    E.nchan = 1u;
    return true;
  }
  return false;
}

// 4 bytes from byte b of a staged row, little-endian; the bytes above a shorter sample are whatever follows in LDS (inside the
// array: IMG_ROW_WORDS has the room) - INVARIANT: img_sample masks them away
__device__ __forceinline__ uint32_t img_fetch(const uint32_t* sh, uint32_t b) {
  const uint32_t w = b >> 2;
  const unsigned long long two = ((unsigned long long)sh[w + 1u] << 32) | (unsigned long long)sh[w];
  return (uint32_t)(two >> ((b & 3u) * 8u));
}
// one 8- or 16-bit sample as an integer, the 16-bit word assembled in the message's byte order
__device__ __forceinline__ uint32_t img_sample(const uint32_t* sh, uint32_t b, uint32_t bpc, bool be) {
  const uint32_t w = img_fetch(sh, b);
  if (bpc == 1u) return w & 0xFFu;
  const uint32_t s = w & 0xFFFFu;
  return be ? ((s & 0xFFu) << 8) | (s >> 8) : s;
}

// pixels [p0, p0 + n) of row y -> sh; returns the LDS byte of pixel p0's first byte.  No byte outside the buffer is read.
__device__ __forceinline__ uint32_t img_stage(uint32_t* sh, const ImgArgs& A, uint32_t y, uint32_t p0, uint32_t n) {
  // in "virtual" offsets (buffer offset + base_mis) a multiple of 4 is an aligned address
  const unsigned long long b0 = (unsigned long long)y * A.step + (unsigned long long)p0 * A.bpp;
  const unsigned long long s0 = b0 + A.base_mis, a0 = s0 & ~3ull;
  const uint32_t staged = (uint32_t)(s0 - a0) + n * A.bpp;                       // <= 3 + (IMG_TILE_W + 2) * IMG_MAX_BPP
  const uint32_t ndw = (staged + 3u) >> 2;
  const unsigned long long lo = A.base_mis, hi = A.base_mis + A.data_bytes;      // valid virtual offsets: [lo, hi)
  const uint8_t* vbase = A.data - A.base_mis;                                    // virtual offset 0 (never dereferenced itself)
  for (uint32_t i = threadIdx.x; i < ndw; i += (uint32_t)IMG_TILE_W) {
    const unsigned long long vo = a0 + 4ull * i;
    uint32_t w = 0u;
    if (vo >= lo && vo + 4ull <= hi) {
      w = *reinterpret_cast<const uint32_t*>(vbase + vo);
    } else {      // the dword straddles an end of the buffer: only the bytes inside it are read
      for (uint32_t k = 0; k < 4u; k++)
        if (vo + k >= lo && vo + k < hi) w |= (uint32_t)vbase[vo + k] << (8u * k);
    }
    sh[i] = w;
  }
  return (uint32_t)(s0 - a0);
}

template <int MODE>
__global__ __launch_bounds__(IMG_TILE_W) void k_image_decode(const ImgArgs A) {
  __shared__ uint32_t sh[(MODE == IMG_BAYER ? 3 : 1) * IMG_ROW_WORDS];
  const uint32_t t = threadIdx.x;
  const uint32_t y = blockIdx.x / A.tiles_x;
  const uint32_t x0 = (blockIdx.x - y * A.tiles_x) * (uint32_t)IMG_TILE_W;
  const uint32_t m = A.W - x0 < (uint32_t)IMG_TILE_W ? A.W - x0 : (uint32_t)IMG_TILE_W;
  const bool be = A.be != 0;
  const size_t plane = (size_t)A.W * A.H, at = (size_t)y * A.W + x0 + t;

  if (MODE == IMG_BAYER) {
    // rows y - 1, y, y + 1 and columns x0 - 1 .. x0 + m, reflected without repeating the edge (-1 -> 1, W -> W - 2): the
    // reflected column always lies inside [p0, p1] (W >= 2), the reflected row is staged in the neighbour's place
    const uint32_t p0 = x0 > 0u ? x0 - 1u : 0u, p1 = x0 + m < A.W ? x0 + m : A.W - 1u;
    const uint32_t yu = y > 0u ? y - 1u : 1u, yd = y + 1u < A.H ? y + 1u : A.H - 2u;
    const uint32_t bu = img_stage(sh, A, yu, p0, p1 - p0 + 1u);
    const uint32_t bc = img_stage(sh + IMG_ROW_WORDS, A, y, p0, p1 - p0 + 1u);
    const uint32_t bd = img_stage(sh + 2 * IMG_ROW_WORDS, A, yd, p0, p1 - p0 + 1u);
    __syncthreads();
    if (t >= m) return;
    const uint32_t x = x0 + t;
    const uint32_t xl = (x > 0u ? x - 1u : 1u) - p0, xc = x - p0, xr = (x + 1u < A.W ? x + 1u : A.W - 2u) - p0;
    const uint32_t* su = sh;
    const uint32_t* sc = sh + IMG_ROW_WORDS;
    const uint32_t* sd = sh + 2 * IMG_ROW_WORDS;
#define IMG_TAP(row, base, col) img_sample(row, (base) + (col) * A.bpp, A.bpc, be)
    const uint32_t own = IMG_TAP(sc, bc, xc);
    const uint32_t horiz = IMG_TAP(sc, bc, xl) + IMG_TAP(sc, bc, xr);
    const uint32_t vert = IMG_TAP(su, bu, xc) + IMG_TAP(sd, bd, xc);
    const uint32_t diag = (IMG_TAP(su, bu, xl) + IMG_TAP(su, bu, xr)) + (IMG_TAP(sd, bd, xl) + IMG_TAP(sd, bd, xr));
#undef IMG_TAP
    const bool red_col = (x & 1u) == A.rx, red_row = (y & 1u) == A.ry;
    uint32_t sr, sg, sb, nr, ng, nb;
    if (red_col == red_row) {      // a red or a blue site: green on the four edge neighbours, the other colour on the diagonals
      sg = horiz + vert; ng = 4u;
      if (red_col) { sr = own; nr = 1u; sb = diag; nb = 4u; }
      else { sb = own; nb = 1u; sr = diag; nr = 4u; }
    } else {                       // a green site: the colour of its row left and right, the other one above and below
      sg = own; ng = 1u;
      if (red_row) { sr = horiz; sb = vert; }
      else { sr = vert; sb = horiz; }
      nr = nb = 2u;
    }
    A.out[at] = ((float)sr / ((float)nr * A.inv));      // (n * 255, n * 65535: exact)
    A.out[plane + at] = ((float)sg / ((float)ng * A.inv));
    A.out[2 * plane + at] = ((float)sb / ((float)nb * A.inv));
    return;
  }

  const uint32_t base = img_stage(sh, A, y, x0, m);
  __syncthreads();
  if (t >= m) return;
  const uint32_t b = base + t * A.bpp;
  if (MODE == IMG_COLOR) {
    A.out[at] = ((float)img_sample(sh, b + A.off[0], A.bpc, be) / A.inv);
    A.out[plane + at] = ((float)img_sample(sh, b + A.off[1], A.bpc, be) / A.inv);
    A.out[2 * plane + at] = ((float)img_sample(sh, b + A.off[2], A.bpc, be) / A.inv);
    return;
  }
  float d;
  if (A.bpc == 2u) {
    d = ((float)img_sample(sh, b, 2u, be) * A.scale);
  } else {
    const uint32_t w = img_fetch(sh, b);
    const float f = __uint_as_float(be ? __builtin_bswap32(w) : w);
    d = (f * A.scale);
    if (!(f > 0.f) || !(f < INFINITY)) d = 0.f;      // NaN, +-inf, <= 0 (-0 and negative denormals included)
  }
  if (!(d > 0.f) || !(d < INFINITY)) d = 0.f;        // (a product that left the range; raw 0)
  if (d < A.lo || d > A.hi) d = 0.f;
  A.out[at] = d;
}

// one dword of the interleaved rgb8 stream per lane: bytes 4 i .. 4 i + 3, byte e = channel e % 3 of pixel e / 3
__global__ __launch_bounds__(256) void k_image_encode_rgb8(uint32_t N, const float* __restrict__ img, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t total = 3u * N;      // (N <= 2^30 - 1: no overflow)
  if (4u * i >= total) return;
  uint32_t w = 0u, nb = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const uint32_t e = 4u * i + k;
    if (e >= total) break;
    const uint32_t p = e / 3u, c = e - 3u * p;
    float v = img[(size_t)c * N + p];
    v = (v != v) ? 0.f : fminf(fmaxf(v, 0.f), 1.f);
    w |= ((uint32_t)(int)(v * 255.0f) & 255u) << (8u * k);
    nb = k + 1u;
  }
  if (nb == 4u) {
    reinterpret_cast<uint32_t*>(out)[i] = w;
  } else {
    for (uint32_t k = 0; k < nb; k++) out[4u * i + k] = (uint8_t)(w >> (8u * k));
  }
}

// ---- depth registration ------------------------------------------------------------------------------------------------------------
struct DregArgs {
  int32_t Wd, Hd, Wc, Hc;
  float fxd, fyd, cxd, cyd, fxc, fyc, cxc, cyc;
  double T[12];      // rows 0 .. 2 of depth -> colour, row-major 3 x 4
};

// "q = T s" of include/gsr.h in the operation order of rigid_common.h's reg_apply - component i =
// (float)(((T[i,0] x + T[i,1] y) + T[i,2] z) + T[i,3]): three products and three sums, each rounded to float64 on its own, then
// one rounding to float32 - with nothing contracted (see the pragma above)
__device__ __forceinline__ float3 dreg_apply(const double* T, float x, float y, float z) {
  float q[3];
  const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double a = T[4 * i] * dx + T[4 * i + 1] * dy;
    q[i] = (float)((a + T[4 * i + 2] * dz) + T[4 * i + 3]);
  }
  return make_float3(q[0], q[1], q[2]);
}

__global__ __launch_bounds__(256) void k_dreg_clear(uint32_t n, uint32_t* __restrict__ buf, int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0u) status[0] = 0;
  if (i < n) buf[i] = IMG_UNTOUCHED;
}

struct DregCorner {
  float px, py, z;
};
// a point of the depth image's plane (uc, vc) with reading d -> its pixel in the colour camera and its z there
__device__ __forceinline__ DregCorner dreg_project(const DregArgs& A, float uc, float vc, float d) {
  const float x = (((uc - A.cxd) / A.fxd) * d);
  const float y = (((vc - A.cyd) / A.fyd) * d);
  const float3 q = dreg_apply(A.T, x, y, d);
  DregCorner c;
  c.px = ((A.fxc * (q.x / q.z)) + A.cxc);
  c.py = ((A.fyc * (q.y / q.z)) + A.cyc);
  c.z = q.z;
  return c;
}
__device__ __forceinline__ bool dreg_finite(float v) { return fabsf(v) < INFINITY; }      // (false for NaN)
// floor(p + 0.5) clamped in float to [-1, S], then an int
__device__ __forceinline__ int dreg_round(float p, int S) {
  return (int)fminf(fmaxf(floorf((p + 0.5f)), -1.0f), (float)S);
}

__global__ __launch_bounds__(256) void k_dreg_splat(const DregArgs A, const float* __restrict__ depth, uint32_t* __restrict__ buf,
                                                    int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint32_t)A.Wd * (uint32_t)A.Hd) return;
  const float d = depth[i];
  if (!(d > 0.f)) return;
  const uint32_t v = i / (uint32_t)A.Wd, u = i - v * (uint32_t)A.Wd;
  const float fu = (float)u, fv = (float)v;
  const DregCorner c = dreg_project(A, fu, fv, d);
  if (!(c.z > 0.f) || !dreg_finite(c.z)) return;
  const DregCorner a = dreg_project(A, (fu - 0.5f), (fv - 0.5f), d);
  const DregCorner b = dreg_project(A, (fu + 0.5f), (fv + 0.5f), d);
  if (!dreg_finite(a.px) || !dreg_finite(a.py) || !dreg_finite(b.px) || !dreg_finite(b.py)) return;
  const int ax = dreg_round(a.px, A.Wc), ay = dreg_round(a.py, A.Hc), bx = dreg_round(b.px, A.Wc), by = dreg_round(b.py, A.Hc);
  int x0 = ax < bx ? ax : bx, x1 = ax < bx ? bx : ax, y0 = ay < by ? ay : by, y1 = ay < by ? by : ay;
  x0 = x0 < 0 ? 0 : x0;                      // the part of the rectangle inside the image ...
  y0 = y0 < 0 ? 0 : y0;
  x1 = x1 > A.Wc - 1 ? A.Wc - 1 : x1;
  y1 = y1 > A.Hc - 1 ? A.Hc - 1 : y1;
  if (x0 > x1 || y0 > y1) return;
  bool cut = false;                          // ... and of that at most IMG_DREG_CAP columns and rows from its low corner
  if (x1 - x0 >= IMG_DREG_CAP) { x1 = x0 + IMG_DREG_CAP - 1; cut = true; }
  if (y1 - y0 >= IMG_DREG_CAP) { y1 = y0 + IMG_DREG_CAP - 1; cut = true; }
  if (cut) atomicOr(status, 1);
  const uint32_t zb = __float_as_uint(c.z);
  for (int yy = y0; yy <= y1; yy++)
    for (int xx = x0; xx <= x1; xx++) atomicMin(&buf[(size_t)yy * A.Wc + xx], zb);
}

__global__ __launch_bounds__(256) void k_dreg_finalize(uint32_t n, const uint32_t* __restrict__ buf, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t w = buf[i];
  out[i] = w == IMG_UNTOUCHED ? 0u : w;
}

extern "C" {

int gsr_image_decode(const gsr_image_layout* layout, const void* data, size_t data_bytes, float depth_scale, float depth_lo,
                     float depth_hi, float* out, void* stream) {
  if (!layout || !data || !out) {
    gsr_set_error("image_decode: NULL layout / data / out");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const gsr_image_layout& L = *layout;
  ImgEnc E;
  if (!img_encoding(L.encoding, E)) {
    gsr_set_error("image_decode: encoding = %d is no GSR_IMG_* code", (int)L.encoding);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const unsigned long long bpp = (unsigned long long)E.nchan * E.bpc, row_bytes = (unsigned long long)L.width * bpp;
  const unsigned long long n64 = (unsigned long long)L.width * (unsigned long long)L.height;
  if (n64 > 0x3FFFFFFFull) {
    gsr_set_error("image_decode: width * height = %llu above 2^30 - 1", n64);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (E.mode == IMG_BAYER && (L.width < 2u || L.height < 2u)) {
    gsr_set_error("image_decode: a Bayer image of %u x %u (at least 2 x 2)", L.width, L.height);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (E.mode == IMG_DEPTH && (!(depth_scale > 0.f) || !(depth_scale < INFINITY) || depth_lo != depth_lo || depth_hi != depth_hi)) {
    gsr_set_error("image_decode: depth_scale = %g (finite, > 0), depth_lo = %g, depth_hi = %g (no NaN)", (double)depth_scale,
                  (double)depth_lo, (double)depth_hi);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if ((unsigned long long)L.step < row_bytes ||
      (n64 > 0ull && (unsigned long long)(L.height - 1u) * L.step + row_bytes > (unsigned long long)data_bytes)) {
    gsr_set_error("image_decode: step = %u below width * bytes per pixel = %llu, or %llu bytes of data are too few", L.step,
                  row_bytes, (unsigned long long)data_bytes);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (n64 == 0ull) return GSR_OK;
  ImgArgs A;
  A.data = (const uint8_t*)data;
  A.data_bytes = (unsigned long long)data_bytes;
  A.base_mis = (uint32_t)((uintptr_t)data & 3u);
  A.W = L.width;
  A.H = L.height;
  A.step = L.step;
  A.tiles_x = (L.width + (uint32_t)IMG_TILE_W - 1u) / (uint32_t)IMG_TILE_W;
  A.bpp = (uint32_t)bpp;
  A.bpc = E.bpc;
  A.off[0] = E.ro * E.bpc;
  A.off[1] = E.go * E.bpc;
  A.off[2] = E.bo * E.bpc;
  A.rx = E.rx;
  A.ry = E.ry;
  A.be = L.is_bigendian != 0 ? 1 : 0;
  A.inv = E.bpc == 2u ? 65535.0f : 255.0f;
  A.scale = depth_scale;
  A.lo = depth_lo;
  A.hi = depth_hi;
  A.out = out;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(A.tiles_x * L.height);      // (<= width * height <= 2^30 - 1)
  if (E.mode == IMG_COLOR) GSR_LAUNCH("image_decode_color", k_image_decode<IMG_COLOR>, grid, dim3(IMG_TILE_W), 0, st, A);
  else if (E.mode == IMG_BAYER) GSR_LAUNCH("image_decode_bayer", k_image_decode<IMG_BAYER>, grid, dim3(IMG_TILE_W), 0, st, A);
  else GSR_LAUNCH("image_decode_depth", k_image_decode<IMG_DEPTH>, grid, dim3(IMG_TILE_W), 0, st, A);
  return gsr_launch_status("image_decode launch");
}

int gsr_image_encode_rgb8(int32_t W, int32_t H, const float* image, void* out_bytes, void* stream) {
  const long long n64 = (long long)W * (long long)H;
  if (W < 1 || H < 1 || n64 > 0x3FFFFFFFll || !image || !out_bytes || ((uintptr_t)out_bytes & 3u) != 0u) {
    gsr_set_error("image_encode_rgb8: bad arguments (%d x %d outside [1, 2^30 - 1] pixels; NULL image / out, or out not 4-byte "
                  "aligned)", (int)W, (int)H);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const uint32_t n = (uint32_t)n64, ndw = (3u * n + 3u) / 4u;
  GSR_LAUNCH("image_encode_rgb8", k_image_encode_rgb8, dim3((ndw + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, image,
             (uint8_t*)out_bytes);
  return gsr_launch_status("image_encode_rgb8 launch");
}

// the workspace of gsr_depth_register: the z-buffer of the colour image, depth bits per pixel
struct DregWs {
  uint32_t* zbuf;      // u32[Wc Hc]
  size_t total;
};
static DregWs dreg_ws(void* base, int32_t Wc, int32_t Hc) {
  GsrCarve c(base);
  DregWs w;
  w.zbuf = c.take<uint32_t>((size_t)(Wc < 1 ? 1 : Wc) * (size_t)(Hc < 1 ? 1 : Hc));
  w.total = c.o;
  return w;
}
size_t gsr_depth_register_workspace_bytes(int32_t Wc, int32_t Hc) { return dreg_ws(nullptr, Wc, Hc).total; }

int gsr_depth_register(int32_t Wd, int32_t Hd, const float* depth, const float* Kd, const float* Kc, const double* T_cd,
                       int32_t Wc, int32_t Hc, float* out, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (!depth || !Kd || !Kc || !T_cd || !out || !status_dev || !workspace || Wd < 1 || Hd < 1 || Wc < 1 || Hc < 1 ||
      (long long)Wd * Hd > 0x3FFFFFFFll || (long long)Wc * Hc > 0x3FFFFFFFll) {
    gsr_set_error("depth_register: bad arguments (a NULL pointer, or %d x %d / %d x %d outside [1, 2^30 - 1] pixels)", (int)Wd,
                  (int)Hd, (int)Wc, (int)Hc);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < 4; i++) {
    const bool focal = i < 2;
    if (!(fabsf(Kd[i]) < INFINITY) || !(fabsf(Kc[i]) < INFINITY) || (focal && (!(Kd[i] > 0.f) || !(Kc[i] > 0.f)))) {
      gsr_set_error("depth_register: intrinsics (fx, fy, cx, cy) must be finite, fx and fy positive");
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  for (int i = 0; i < 12; i++) {
    if (!(fabs(T_cd[i]) < (double)INFINITY)) {
      gsr_set_error("depth_register: T_cd[%d] is not finite", i);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  const DregWs w = dreg_ws(workspace, Wc, Hc);
  if (!gsr_workspace_fits("depth_register", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  DregArgs A;
  A.Wd = Wd; A.Hd = Hd; A.Wc = Wc; A.Hc = Hc;
  A.fxd = Kd[0]; A.fyd = Kd[1]; A.cxd = Kd[2]; A.cyd = Kd[3];
  A.fxc = Kc[0]; A.fyc = Kc[1]; A.cxc = Kc[2]; A.cyc = Kc[3];
  for (int i = 0; i < 12; i++) A.T[i] = T_cd[i];
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nd = (uint32_t)Wd * (uint32_t)Hd, nc = (uint32_t)Wc * (uint32_t)Hc;
  uint32_t* buf = w.zbuf;
  GSR_LAUNCH("depth_register_clear", k_dreg_clear, dim3((nc + 255u) / 256u), dim3(256), 0, st, nc, buf, status_dev);
  GSR_LAUNCH("depth_register_splat", k_dreg_splat, dim3((nd + 255u) / 256u), dim3(256), 0, st, A, depth, buf, status_dev);
  GSR_LAUNCH("depth_register_finalize", k_dreg_finalize, dim3((nc + 255u) / 256u), dim3(256), 0, st, nc, (const uint32_t*)buf,
             (uint32_t*)out);
  return gsr_launch_status("depth_register launch");
}

}  // extern "C"
