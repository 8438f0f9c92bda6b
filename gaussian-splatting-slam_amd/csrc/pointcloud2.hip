// pointcloud2.hip - a sensor_msgs/PointCloud2 byte buffer decoded on the device: what the reference's process_pointcloud
// (convert_visual_merged_msg.py:115-185) and read_pointcloud / read_points_with_color (:251-326, pointcloud_pcd.py:13-85) do point
// by point with `struct` in a Python loop - unpack x / y / z / rgb, drop NaN rows, crop by height and range, apply a 4 x 4 pose,
// split the packed colour - and its inverse for the canonical layout (pointcloud_aligner.py:13-44).  Rules: include/gsr.h.
//
// Data path.  A workgroup of 256 threads takes PC2_CHUNK = 256 consecutive points of the message, one point per lane.  Their
// bytes form one contiguous span of the buffer (row padding of an organised cloud included).  Where that span fits
// PC2_LDS_BYTES the workgroup brings it into LDS with coalesced dword loads - the span's start aligned down to the dword of its
// ADDRESS, the first and the last dword assembled from guarded byte loads where they would leave the buffer - and every lane then
// picks its fields out of LDS: two dword reads and a funnel shift per field, whatever its alignment.  (Measured, DESIGN.md
// section 4 item 33: the staged form is NOT the faster one - neighbouring lanes' byte loads share their cache lines anyway - and
// 5 - 19 % slower on a cold depth frame, 3 - 4 % slower at 16.8 M points; it is the specified shape and still the default.)  Where the span does not fit (point_step > 64, or rows of few points with much padding) the lanes read their fields
// straight from global memory byte by byte: the direct path, identical bits (pc2_field is the one decoder of both).
//
// Compaction.  Two passes over the message (the second is served by the L2 / Infinity Cache: a 640 x 480 frame is 6 - 10 MB):
//   k_pc2<COUNT>   decodes x, y, z (and a FLOAT32 colour word, for skip_nans), decides keep, counts the kept rows of the chunk;
//   gsr_scan_u32   exclusive scan of the chunk counts;
//   k_pc2<SCATTER> decodes again, decides keep again (the same compiled decisions on the same bytes), ranks the kept rows inside
//                  the workgroup - wave ballot, popcount below the lane, the four wave counts in order - and writes row
//                  offs[chunk] + rank: message order, independent of scheduling.  The last chunk also writes count and status.
// Storing the decoded rows between the passes instead would write and read 28 B per point to save re-reading point_step bytes.
#include "gsr_common.h"
#include "rigid_common.h"

#define PC2_CHUNK 256                    // points per workgroup = threads per workgroup
#define PC2_LDS_BYTES (PC2_CHUNK * 64 + 64)      // staging buffer: point_step <= 64 always fits, misalignment and row padding included
#define PC2_LDS_WORDS (PC2_LDS_BYTES / 4 + 2)    // (+ the dword behind the last one: pc2_lds_fetch reads two)

static int g_pc2_force_direct = 0;      // gsr_debug_pc2_force_direct: process-wide, read per call, not for concurrent callers

struct Pc2Args {
  gsr_pc2_layout L;
  const uint8_t* data;
  unsigned long long data_bytes;
  uint32_t base_mis;       // (address of data) & 3
  uint32_t N;
  const double* T_dev;     // NULL: no pose
  double min_y, max_range2;
  int32_t skip_nans;
  int32_t force_direct;
  float* out_points;
  float* out_colors;
  int32_t* out_index;
  uint32_t cap;
  int64_t* count_dev;
};

// the workspace of gsr_pc2_decode over N points: per chunk of PC2_CHUNK its count of kept points, their exclusive scan, the scan's scratch
struct Pc2Ws {
  uint32_t *cnt, *offs, *scan_tmp;
  size_t total;
};
static Pc2Ws pc2_ws(void* base, size_t N) {
  GsrCarve c(base);
  Pc2Ws W;
  const size_t nb = (N + PC2_CHUNK - 1) / PC2_CHUNK;
  W.cnt = c.take<uint32_t>(nb);
  W.offs = c.take<uint32_t>(nb);
  W.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(nb));
  W.total = c.o;
  return W;
}

static inline __host__ __device__ int pc2_size(int dt) { return dt <= 2 ? 1 : dt <= 4 ? 2 : dt <= 7 ? 4 : 8; }

__device__ __forceinline__ unsigned long long pc2_byte_of(const gsr_pc2_layout& L, uint32_t n) {
  const uint32_t v = n / L.width, u = n - v * L.width;
  return (unsigned long long)v * L.row_step + (unsigned long long)u * L.point_step;
}

// `nbytes` (1 .. 4) bytes from byte b of the staged span, little-endian in the low bytes; the bytes above them are whatever
// follows in LDS - for a field that ends in the last staged dword, sh[w + 1] is LDS nobody wrote (inside the array:
// PC2_LDS_WORDS has the room).  INVARIANT: every caller masks or shifts those bytes away before it uses the value (pc2_field
// masks the 1- and 2-byte types; a 4-byte field lies wholly inside the span, so the shift brings in staged bytes only).
struct Pc2LdsFetch {
  const uint32_t* sh;
  uint32_t base;      // LDS byte of the point's first byte
  __device__ __forceinline__ uint32_t operator()(uint32_t off, int) const {
    const uint32_t b = base + off, w = b >> 2;
    const unsigned long long two = ((unsigned long long)sh[w + 1u] << 32) | (unsigned long long)sh[w];
    return (uint32_t)(two >> ((b & 3u) * 8u));
  }
};
// the same from global memory: exactly `nbytes` byte loads, nothing beyond the field is touched
struct Pc2GlobalFetch {
  const uint8_t* p;   // the point's first byte
  __device__ __forceinline__ uint32_t operator()(uint32_t off, int nbytes) const {
    uint32_t w = 0u;
    for (int k = 0; k < nbytes; k++) w |= (uint32_t)p[off + (uint32_t)k] << (8 * k);
    return w;
  }
};

__device__ __forceinline__ uint32_t pc2_bswap32(uint32_t w) { return __builtin_bswap32(w); }

// the raw 32-bit word of a 4-byte field in the message's byte order
template <class Fetch>
__device__ __forceinline__ uint32_t pc2_word(const Fetch& f, int off, bool be) {
  const uint32_t w = f((uint32_t)off, 4);
  return be ? pc2_bswap32(w) : w;
}

// one coordinate field as float32: FLOAT32 bit for bit, everything else one conversion (round to nearest even where it rounds)
template <class Fetch>
__device__ __forceinline__ float pc2_field(const Fetch& f, int off, int dt, bool be) {
  const int size = pc2_size(dt);
  uint32_t w0 = f((uint32_t)off, size < 4 ? size : 4), w1 = 0u;
  if (size == 8) w1 = f((uint32_t)off + 4u, 4);
  if (size == 1) w0 &= 0xFFu;
  if (size == 2) {
    w0 &= 0xFFFFu;
    if (be) w0 = ((w0 & 0xFFu) << 8) | (w0 >> 8);
  }
  if (size == 4 && be) w0 = pc2_bswap32(w0);
  if (size == 8 && be) {
    const uint32_t t = pc2_bswap32(w0);
    w0 = pc2_bswap32(w1);
    w1 = t;
  }
  switch (dt) {
    case GSR_PC2_INT8: return (float)(int)(int8_t)w0;
    case GSR_PC2_UINT8: return (float)w0;
    case GSR_PC2_INT16: return (float)(int)(int16_t)w0;
    case GSR_PC2_UINT16: return (float)w0;
    case GSR_PC2_INT32: return (float)(int32_t)w0;
    case GSR_PC2_UINT32: return (float)w0;
    case GSR_PC2_FLOAT32: return __uint_as_float(w0);
    default: return (float)__longlong_as_double((long long)(((unsigned long long)w1 << 32) | (unsigned long long)w0));
  }
}

struct Pc2Point {
  float x, y, z;
  uint32_t color;      // the colour word (0 where it was not read)
  bool keep;
};

// steps 1 - 3 of include/gsr.h for one point; the colour word is read where a rule or an output needs it
template <class Fetch>
__device__ __forceinline__ Pc2Point pc2_point(const Pc2Args& A, const Fetch& f, bool want_color) {
  const gsr_pc2_layout& L = A.L;
  const bool be = L.is_bigendian != 0;
  Pc2Point p;
  p.x = pc2_field(f, L.offset[0], L.datatype[0], be);
  p.y = pc2_field(f, L.offset[1], L.datatype[1], be);
  p.z = pc2_field(f, L.offset[2], L.datatype[2], be);
  const bool nan_color = A.skip_nans != 0 && L.color_offset >= 0 && L.color_datatype == GSR_PC2_FLOAT32;
  p.color = (L.color_offset >= 0 && (want_color || nan_color)) ? pc2_word(f, L.color_offset, be) : 0u;
  bool keep = true;
  if (A.skip_nans != 0) {
    if (p.x != p.x || p.y != p.y || p.z != p.z) keep = false;
    if (nan_color && (p.color & 0x7FFFFFFFu) > 0x7F800000u) keep = false;
  }
  const double dx = (double)p.x, dy = (double)p.y, dz = (double)p.z;
  if (dy < A.min_y) keep = false;
  const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
  if (d2 > A.max_range2) keep = false;
  p.keep = keep;
  return p;
}

template <bool SCATTER>
__global__ __launch_bounds__(PC2_CHUNK) void k_pc2(const Pc2Args A, uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offs) {
  __shared__ uint32_t sh[PC2_LDS_WORDS];
  __shared__ uint32_t wave_cnt[PC2_CHUNK / GSR_WAVE];
  const uint32_t t = threadIdx.x;
  const uint32_t n0 = blockIdx.x * (uint32_t)PC2_CHUNK;                     // (N <= 2^30 - 1: no overflow)
  const uint32_t m = A.N - n0 < (uint32_t)PC2_CHUNK ? A.N - n0 : (uint32_t)PC2_CHUNK;
  // the chunk's byte span [b0, b1) of the buffer; in "virtual" offsets (buffer offset + base_mis) a multiple of 4 is an aligned address
  const unsigned long long b0 = pc2_byte_of(A.L, n0);
  const unsigned long long b1 = pc2_byte_of(A.L, n0 + m - 1u) + A.L.point_step;
  const unsigned long long s0 = b0 + A.base_mis, a0 = s0 & ~3ull;
  const unsigned long long staged = (b1 + A.base_mis) - a0;                 // bytes from the aligned start to the span's end
  const bool use_lds = A.force_direct == 0 && staged <= (unsigned long long)PC2_LDS_BYTES;      // (uniform over the workgroup)
  const bool want_color = SCATTER && A.out_colors != nullptr;

  Pc2Point p;
  p.keep = false;
  if (use_lds) {
    const uint32_t ndw = ((uint32_t)staged + 3u) >> 2;
    const unsigned long long lo = A.base_mis, hi = A.base_mis + A.data_bytes;      // valid virtual offsets: [lo, hi)
    const uint8_t* vbase = A.data - A.base_mis;                                    // virtual offset 0 (an aligned address; never dereferenced itself)
    for (uint32_t i = t; i < ndw; i += (uint32_t)PC2_CHUNK) {
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
    __syncthreads();
    if (t < m) {
      Pc2LdsFetch f;
      f.sh = sh;
      f.base = (uint32_t)((pc2_byte_of(A.L, n0 + t) + A.base_mis) - a0);
      p = pc2_point(A, f, want_color);
    }
  } else if (t < m) {
    Pc2GlobalFetch f;
    f.p = A.data + pc2_byte_of(A.L, n0 + t);
    p = pc2_point(A, f, want_color);
  }

  const unsigned long long ballot = __ballot(p.keep);
  const uint32_t wave = t >> 6;
  if (gsr_lane() == 0) wave_cnt[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t before = 0u, total = 0u;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)(PC2_CHUNK / GSR_WAVE); w++) {
    const uint32_t c = wave_cnt[w];
    if (w < wave) before += c;
    total += c;
  }
  if (!SCATTER) {
    if (t == 0u) cnt[blockIdx.x] = total;
    return;
  }
  const uint32_t base = offs[blockIdx.x];
  if (blockIdx.x == gridDim.x - 1u && t == 0u) {
    const unsigned long long kept = (unsigned long long)base + total;
    A.count_dev[0] = (int64_t)kept;
    A.count_dev[1] = kept > (unsigned long long)A.cap ? 1 : 0;
  }
  if (!p.keep) return;
  const uint32_t row = base + before + (uint32_t)__popcll(ballot & ((1ull << gsr_lane()) - 1ull));
  if (row >= A.cap) return;
  uint32_t* op = reinterpret_cast<uint32_t*>(A.out_points) + 3 * (size_t)row;
  if (A.T_dev) {
    const RegT T = reg_load(A.T_dev);
    const float4 q = reg_apply(T, p.x, p.y, p.z);
    op[0] = __float_as_uint(q.x);
    op[1] = __float_as_uint(q.y);
    op[2] = __float_as_uint(q.z);
  } else {      // (as words: the bits pass, NaN payloads included)
    op[0] = __float_as_uint(p.x);
    op[1] = __float_as_uint(p.y);
    op[2] = __float_as_uint(p.z);
  }
  if (A.out_colors) {
    float* oc = A.out_colors + 3 * (size_t)row;
    oc[0] = __fdiv_rn((float)((p.color >> 16) & 255u), 255.0f);
    oc[1] = __fdiv_rn((float)((p.color >> 8) & 255u), 255.0f);
    oc[2] = __fdiv_rn((float)(p.color & 255u), 255.0f);
  }
  if (A.out_index) A.out_index[row] = (int32_t)(n0 + t);
}

__global__ __launch_bounds__(256) void k_pc2_encode(uint32_t P, const uint32_t* __restrict__ pts, const float* __restrict__ cols,
                                                    uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  uint32_t w = 0u;
  if (cols) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      float c = cols[3 * (size_t)i + a];
      c = (c != c) ? 0.f : fminf(fmaxf(c, 0.f), 1.f);
      w = (w << 8) | (uint32_t)(int)__fadd_rn(__fmul_rn(c, 255.0f), 0.5f);
    }
  }
  uint32_t* o = out + 4 * (size_t)i;
  o[0] = pts[3 * (size_t)i];
  o[1] = pts[3 * (size_t)i + 1];
  o[2] = pts[3 * (size_t)i + 2];
  o[3] = w;
}

static bool pc2_field_ok(int32_t off, int32_t dt, uint32_t point_step) {
  return off >= 0 && (unsigned long long)off + (unsigned long long)pc2_size(dt) <= (unsigned long long)point_step;
}

extern "C" {

size_t gsr_pc2_decode_workspace_bytes(int64_t N) { return pc2_ws(nullptr, (size_t)(N < 1 ? 1 : N)).total; }

int32_t gsr_debug_pc2_force_direct(int32_t on) {
  const int32_t prev = g_pc2_force_direct;
  g_pc2_force_direct = on != 0 ? 1 : 0;
  return prev;
}

int gsr_pc2_decode(const gsr_pc2_layout* layout, const void* data, size_t data_bytes, const double* T_dev, double min_y,
                   double max_range2, int32_t skip_nans, float* out_points, float* out_colors, int32_t* out_index, int64_t cap,
                   int64_t* count_dev, void* workspace, size_t workspace_bytes, void* stream) {
  if (!layout || !data || !count_dev || !workspace || cap < 0 || (cap > 0 && !out_points) || min_y != min_y ||
      max_range2 != max_range2) {
    gsr_set_error("pc2_decode: bad arguments (a NULL pointer, cap = %lld, min_y = %g, max_range2 = %g)", (long long)cap, min_y,
                  max_range2);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const gsr_pc2_layout& L = *layout;
  const unsigned long long n64 = (unsigned long long)L.width * (unsigned long long)L.height;
  if (n64 < 1ull || n64 > 0x3FFFFFFFull) {
    gsr_set_error("pc2_decode: width * height = %llu outside [1, 2^30 - 1]", n64);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  for (int a = 0; a < 3; a++) {
    if (L.datatype[a] < GSR_PC2_INT8 || L.datatype[a] > GSR_PC2_FLOAT64 || !pc2_field_ok(L.offset[a], L.datatype[a], L.point_step)) {
      gsr_set_error("pc2_decode: field %c (offset %d, datatype %d) is no PointField type or leaves point_step = %u", "xyz"[a],
                    (int)L.offset[a], (int)L.datatype[a], L.point_step);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  if (L.color_offset >= 0) {
    const int32_t dt = L.color_datatype;
    if ((dt != GSR_PC2_FLOAT32 && dt != GSR_PC2_UINT32 && dt != GSR_PC2_INT32) || !pc2_field_ok(L.color_offset, dt, L.point_step)) {
      gsr_set_error("pc2_decode: colour field (offset %d, datatype %d) is not FLOAT32 / UINT32 / INT32 inside point_step = %u",
                    (int)L.color_offset, (int)dt, L.point_step);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  } else if (out_colors) {
    gsr_set_error("pc2_decode: out_colors given, but the message has no colour field");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const unsigned long long row_bytes = (unsigned long long)L.width * L.point_step;
  if ((unsigned long long)L.row_step < row_bytes ||
      (unsigned long long)(L.height - 1u) * L.row_step + row_bytes > (unsigned long long)data_bytes) {
    gsr_set_error("pc2_decode: row_step = %u below width * point_step = %llu, or %llu bytes of data are too few", L.row_step,
                  row_bytes, (unsigned long long)data_bytes);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const Pc2Ws W = pc2_ws(workspace, (size_t)n64);
  if (!gsr_workspace_fits("pc2_decode", workspace, workspace_bytes, W.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  Pc2Args A;
  A.L = L;
  A.data = (const uint8_t*)data;
  A.data_bytes = (unsigned long long)data_bytes;
  A.base_mis = (uint32_t)((uintptr_t)data & 3u);
  A.N = (uint32_t)n64;
  A.T_dev = T_dev;
  A.min_y = min_y;
  A.max_range2 = max_range2;
  A.skip_nans = skip_nans != 0 ? 1 : 0;
  A.force_direct = g_pc2_force_direct;
  A.out_points = out_points;
  A.out_colors = out_colors;
  A.out_index = out_index;
  A.cap = (uint32_t)(cap > 0x3FFFFFFF ? 0x3FFFFFFF : cap);
  A.count_dev = count_dev;
  const uint32_t nb = (A.N + (uint32_t)PC2_CHUNK - 1u) / (uint32_t)PC2_CHUNK;
  GSR_LAUNCH("pc2_count", k_pc2<false>, dim3(nb), dim3(PC2_CHUNK), 0, st, A, W.cnt, (const uint32_t*)W.offs);
  gsr_scan_u32(W.cnt, nullptr, W.offs, (size_t)nb, 0, W.scan_tmp, st);
  GSR_LAUNCH("pc2_scatter", k_pc2<true>, dim3(nb), dim3(PC2_CHUNK), 0, st, A, W.cnt, (const uint32_t*)W.offs);
  return gsr_launch_status("pc2_decode launch");
}

int gsr_pc2_encode(int64_t P, const float* points, const float* colors, void* out, void* stream) {
  if (P <= 0 || P > 0x3FFFFFFF || !points || !out || ((uintptr_t)out & 3u) != 0u) {
    gsr_set_error("pc2_encode: bad arguments (P = %lld; NULL points / out, or out not 4-byte aligned)", (long long)P);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const uint32_t n = (uint32_t)P;
  GSR_LAUNCH("pc2_encode", k_pc2_encode, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, (const uint32_t*)points,
             colors, (uint32_t*)out);
  return gsr_launch_status("pc2_encode launch");
}

}  // extern "C"
