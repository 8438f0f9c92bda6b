// orb.hip - sparse image features for place recognition: FAST-9 corners, a 256-bit BRIEF descriptor steered by the intensity
// centroid, and brute-force Hamming matching (include/gsr.h has the full contracts).  Everything
// after the quantisation of gsr_orb_prepare is integer arithmetic: every output is a function of the input alone.
//
// gsr_orb_prepare: k_orb_quantise (one thread per pixel: the odometry's intensity, one explicit fma, floor, clamp) and k_orb_box
//   (5 x 5 sum of the u8 plane with a replicated border, 25 byte loads that the cache serves).
// gsr_orb_detect: one workgroup of 256 threads per 32 x 32 cell.  The cell's pixels with a halo of 4 sit in LDS as bytes (40 x 40),
//   the scores of the cell with a halo of 1 as words (34 x 34: the lanes of a half wave read consecutive words of one row).  The
//   min over 9 consecutive circle pixels comes from sliding minima of 2, 4, 8 and 9 - 64 min per sign instead of 128.  Survivors of
//   the 3 x 3 suppression (at most 256 per cell: no two are neighbours) are appended to an LDS list as keys (score << 10 | 1023 -
//   raster position inside the cell), all distinct; a survivor's slot is the number of larger keys, so neither the order of the
//   appends nor anything else in the schedule reaches the output; thread r then writes slot r.  No global atomics; every slot of
//   the cell is written.
// gsr_orb_describe: one wave per keypoint, four per workgroup.  The 961 pixels of the 31 x 31 square are spread over the lanes, the
//   two moments added by an integer butterfly; every lane then forms the bin itself (float64 atan2 of the same two integers),
//   reads its four pairs as one 16-byte load of the pre-rotated table and compares box sums; eight lanes OR their nibbles into
//   one word.
// gsr_hamming_match / gsr_hamming_vote: 64 queries per workgroup, one per lane, eight words in registers; the four waves of the
//   workgroup take a quarter of every LDS tile of 256 database rows each (a row is read as two 16-byte words at the same address in
//   every lane: a broadcast), and their (best, row, second) records meet in LDS by a merge that is exact for multisets and takes
//   the lexicographic minimum of (distance, row).  The vote kernel runs the same scan over one frame's segment per blockIdx.y and
//   adds the workgroup's count of passing rows to the frame's int32 (an integer add: any order gives the same sum).
#include "gsr_common.h"

#define ORB_CELL GSR_ORB_CELL
#define ORB_PIX (ORB_CELL + 8)          // the cell and a halo of 4
#define ORB_SC (ORB_CELL + 2)           // the cell and a halo of 1
#define ORB_R 15
#define ORB_TABLE_BYTES (GSR_ORB_BINS * 256 * 4)
#define HAM_QUERIES 64
#define HAM_TILE 256

static const int8_t h_orb_pattern[ORB_TABLE_BYTES] = {
#include "orb_pattern.inc"
};
__device__ const int8_t d_orb_pattern[ORB_TABLE_BYTES] __attribute__((aligned(16))) = {
#include "orb_pattern.inc"
};

// ==== prepare ==========================================================================================================================
__global__ __launch_bounds__(256) void k_orb_quantise(uint32_t n, const float* __restrict__ image, int channels,
                                                      uint8_t* __restrict__ u8) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  float I = image[i];
  if (channels == 3) I = __fdiv_rn(__fadd_rn(__fadd_rn(I, image[(size_t)n + i]), image[2 * (size_t)n + i]), 3.0f);
  const float v = floorf(__fmaf_rn(255.0f, I, 0.5f));
  u8[i] = (uint8_t)(v >= 255.0f ? 255 : (v >= 1.0f ? (int)v : 0));      // (NaN: every comparison false, 0)
}

__global__ __launch_bounds__(256) void k_orb_box(int w, int h, const uint8_t* __restrict__ u8, uint16_t* __restrict__ box) {
  const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
  if (x >= w || y >= h) return;
  uint32_t s = 0;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const uint8_t* __restrict__ row = u8 + (size_t)min(max(y + dy, 0), h - 1) * w;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) s += row[min(max(x + dx, 0), w - 1)];
  }
  box[(size_t)y * w + x] = (uint16_t)s;
}

// ==== detect ===========================================================================================================================
// the 16 pixels of the radius-3 circle, clockwise from 12 o'clock (y down)
__device__ __forceinline__ int orb_fast_score(const uint8_t* __restrict__ c, int pitch) {      // c: the centre pixel in LDS
  const int p = (int)c[0];
  int d[16];
  d[0] = (int)c[-3 * pitch] - p;      d[1] = (int)c[-3 * pitch + 1] - p;  d[2] = (int)c[-2 * pitch + 2] - p;
  d[3] = (int)c[-pitch + 3] - p;      d[4] = (int)c[3] - p;               d[5] = (int)c[pitch + 3] - p;
  d[6] = (int)c[2 * pitch + 2] - p;   d[7] = (int)c[3 * pitch + 1] - p;   d[8] = (int)c[3 * pitch] - p;
  d[9] = (int)c[3 * pitch - 1] - p;   d[10] = (int)c[2 * pitch - 2] - p;  d[11] = (int)c[pitch - 3] - p;
  d[12] = (int)c[-3] - p;             d[13] = (int)c[-pitch - 3] - p;     d[14] = (int)c[-2 * pitch - 2] - p;
  d[15] = (int)c[-3 * pitch - 1] - p;
  int best = -255;
#pragma unroll
  for (int sign = 0; sign < 2; sign++) {
    int m2[16], m4[16], m8[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m2[i] = min(d[i], d[(i + 1) & 15]);
#pragma unroll
    for (int i = 0; i < 16; i++) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; i++) m8[i] = min(m4[i], m4[(i + 4) & 15]);
#pragma unroll
    for (int i = 0; i < 16; i++) best = max(best, min(m8[i], d[(i + 8) & 15]));
#pragma unroll
    for (int i = 0; i < 16; i++) d[i] = -d[i];
  }
  return best;
}

__global__ __launch_bounds__(256) void k_orb_detect(int w, int h, int cells_x, const uint8_t* __restrict__ u8,
                                                    const float* __restrict__ mask, int threshold, int per_cell,
                                                    int32_t* __restrict__ slots) {
  __shared__ uint8_t pix[ORB_PIX * ORB_PIX];
  __shared__ int32_t sc[ORB_SC * ORB_SC];
  __shared__ uint32_t keys[256];
  __shared__ uint32_t nkeys;
  __shared__ uint32_t best[GSR_ORB_PER_CELL_MAX];
  const int cx = (int)blockIdx.x, cy = (int)blockIdx.y;
  const int x0 = cx * ORB_CELL, y0 = cy * ORB_CELL;
  if (threadIdx.x == 0) nkeys = 0u;
  if (threadIdx.x < GSR_ORB_PER_CELL_MAX) best[threadIdx.x] = 0u;
  // (a halo pixel outside the image: the clamped one - no pixel that qualifies has it on its circle)
  for (int i = (int)threadIdx.x; i < ORB_PIX * ORB_PIX; i += 256) {
    const int gx = min(max(x0 - 4 + i % ORB_PIX, 0), w - 1), gy = min(max(y0 - 4 + i / ORB_PIX, 0), h - 1);
    pix[i] = u8[(size_t)gy * w + gx];
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < ORB_SC * ORB_SC; i += 256) {
    const int sx = i % ORB_SC, sy = i / ORB_SC;
    const int gx = x0 - 1 + sx, gy = y0 - 1 + sy;
    int s = 0;
    if (gx >= GSR_ORB_BORDER && gx < w - GSR_ORB_BORDER && gy >= GSR_ORB_BORDER && gy < h - GSR_ORB_BORDER &&
        (!mask || mask[(size_t)gy * w + gx] > 0.f)) {
      s = orb_fast_score(pix + (sy + 3) * ORB_PIX + (sx + 3), ORB_PIX);
      if (s <= threshold) s = 0;
    }
    sc[i] = s;
  }
  __syncthreads();
  uint32_t mine[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int lx = (int)(threadIdx.x & 31u), ly = (int)(threadIdx.x >> 5) + 8 * j;
    const int32_t* __restrict__ c = sc + (ly + 1) * ORB_SC + (lx + 1);
    const int s = c[0];
    // earlier neighbours (raster order) must be strictly smaller, later ones may be equal
    // (all nine comparisons, joined without short-circuit branches: straight-line code and one select for the key)
    const bool keep = (s > 0) & (s > c[-ORB_SC - 1]) & (s > c[-ORB_SC]) & (s > c[-ORB_SC + 1]) & (s > c[-1]) & (s >= c[1]) &
                      (s >= c[ORB_SC - 1]) & (s >= c[ORB_SC]) & (s >= c[ORB_SC + 1]);
    mine[j] = keep ? ((uint32_t)s << 10) | (uint32_t)(1023 - (ly * ORB_CELL + lx)) : 0u;
    if (keep) {      // (an LDS counter; at most 256 survivors: no two are neighbours)
      const uint32_t at = atomicAdd(&nkeys, 1u);
      if (at < 256u) keys[at] = mine[j];
    }
  }
  __syncthreads();
  const uint32_t n = min(nkeys, 256u);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (mine[j] == 0u) continue;
    int rank = 0;
    for (uint32_t k = 0; k < n; k++) rank += keys[k] > mine[j] ? 1 : 0;
    if (rank < per_cell) best[rank] = mine[j];      // (the keys are distinct: one writer per rank)
  }
  __syncthreads();
  if ((int)threadIdx.x < per_cell) {      // slot r: the survivor of rank r, or empty
    const uint32_t key = best[threadIdx.x];
    const int pos = 1023 - (int)(key & 1023u);
    int32_t* __restrict__ out = slots + (((size_t)cy * cells_x + cx) * per_cell + threadIdx.x) * 3;
    out[0] = key ? x0 + pos % ORB_CELL : 0;
    out[1] = key ? y0 + pos / ORB_CELL : 0;
    out[2] = (int32_t)(key >> 10);
  }
}

// ==== describe =========================================================================================================================
__global__ __launch_bounds__(256) void k_orb_describe(int w, int h, const uint8_t* __restrict__ u8, const uint16_t* __restrict__ box,
                                                      uint32_t M, const int32_t* __restrict__ kp, int32_t* __restrict__ angle_bin,
                                                      int32_t* __restrict__ moments, int32_t* __restrict__ desc) {
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);      // (wave-uniform; no barrier below)
  if (k >= M) return;
  const int lane = gsr_lane();
  const int x = kp[3 * (size_t)k], y = kp[3 * (size_t)k + 1], score = kp[3 * (size_t)k + 2];
  if (score <= 0 || x < GSR_ORB_BORDER || x >= w - GSR_ORB_BORDER || y < GSR_ORB_BORDER || y >= h - GSR_ORB_BORDER) {
    if (lane == 0) {
      angle_bin[k] = -1;
      if (moments) { moments[2 * (size_t)k] = 0; moments[2 * (size_t)k + 1] = 0; }
    }
    if (lane < 8) desc[8 * (size_t)k + lane] = 0;
    return;
  }
  int m10 = 0, m01 = 0;
  for (int i = lane; i < 31 * 31; i += 64) {
    const int dx = i % 31 - ORB_R, dy = i / 31 - ORB_R;
    if (dx * dx + dy * dy <= ORB_R * ORB_R) {
      const int v = (int)u8[(size_t)(y + dy) * w + (x + dx)];
      m10 += dx * v;
      m01 += dy * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m10 += __shfl_xor(m10, o, 64);
    m01 += __shfl_xor(m01, o, 64);
  }
  const double a = atan2((double)m01, (double)m10) / (2.0 * 3.14159265358979323846 / (double)GSR_ORB_BINS);
  int bin = (int)floor(a + 0.5) % GSR_ORB_BINS;
  if (bin < 0) bin += GSR_ORB_BINS;
  // lane l: bits 4 l .. 4 l + 3, sixteen bytes of the bin's table
  const int4 raw = *reinterpret_cast<const int4*>(d_orb_pattern + ((size_t)bin * 256 + 4 * lane) * 4);
  const int words[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t nib = 0u;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int x1 = (int)(int8_t)(words[b] & 0xFF), y1 = (int)(int8_t)((words[b] >> 8) & 0xFF);
    const int x2 = (int)(int8_t)((words[b] >> 16) & 0xFF), y2 = (int)(int8_t)((words[b] >> 24) & 0xFF);
    const uint32_t A = box[(size_t)(y + y1) * w + (x + x1)], B = box[(size_t)(y + y2) * w + (x + x2)];
    nib |= (A < B ? 1u : 0u) << b;
  }
  uint32_t word = nib << (4 * (lane & 7));
  word |= (uint32_t)__shfl_xor((int)word, 1, 64);
  word |= (uint32_t)__shfl_xor((int)word, 2, 64);
  word |= (uint32_t)__shfl_xor((int)word, 4, 64);
  if ((lane & 7) == 0) desc[8 * (size_t)k + (lane >> 3)] = (int32_t)word;
  if (lane == 0) {
    angle_bin[k] = bin;
    if (moments) { moments[2 * (size_t)k] = m10; moments[2 * (size_t)k + 1] = m01; }
  }
}

// ==== Hamming ==========================================================================================================================
struct HamBest { int32_t best, idx, second; };

__device__ __forceinline__ void ham_merge(HamBest& a, const HamBest& b) {      // the two smallest of the union, (distance, row) order
  if (b.best < a.best || (b.best == a.best && (uint32_t)b.idx < (uint32_t)a.idx)) {
    a.second = min(a.best, b.second);
    a.best = b.best;
    a.idx = b.idx;
  } else {
    a.second = min(a.second, b.best);
  }
}

// The workgroup's 64 queries (one per lane, the same in all four waves) against rows [lo, hi) of the database -> the record of
// query threadIdx.x & 63, valid in wave 0.  Every thread of the workgroup calls it (barriers inside).
__device__ __forceinline__ HamBest ham_scan(const int32_t* __restrict__ query, uint32_t Q, const int32_t* __restrict__ db,
                                            uint32_t lo, uint32_t hi, int4* __restrict__ tile, HamBest* __restrict__ part) {
  const int lane = gsr_lane(), wave = (int)(threadIdx.x >> 6);
  const uint32_t qi = blockIdx.x * (uint32_t)HAM_QUERIES + (uint32_t)lane;
  uint32_t q[8];
  {
    const int4* __restrict__ src = reinterpret_cast<const int4*>(query + 8 * (size_t)(qi < Q ? qi : 0u));
    const int4 a = src[0], b = src[1];
    q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
  }
  HamBest r{GSR_HAMMING_NONE, -1, GSR_HAMMING_NONE};
  for (uint32_t first = lo; first < hi; first += (uint32_t)HAM_TILE) {
    const uint32_t rows = min((uint32_t)HAM_TILE, hi - first);
    __syncthreads();
    if (threadIdx.x < rows) {
      const int4* __restrict__ src = reinterpret_cast<const int4*>(db + 8 * (size_t)(first + threadIdx.x));
      tile[2 * threadIdx.x] = src[0];
      tile[2 * threadIdx.x + 1] = src[1];
    }
    __syncthreads();
    const uint32_t r0 = (uint32_t)wave * (HAM_TILE / 4), r1 = min(rows, r0 + HAM_TILE / 4);
    for (uint32_t t = r0; t < r1; t++) {
      const int4 a = tile[2 * t], b = tile[2 * t + 1];
      const int d = ((__popc(q[0] ^ (uint32_t)a.x) + __popc(q[1] ^ (uint32_t)a.y)) + (__popc(q[2] ^ (uint32_t)a.z) + __popc(q[3] ^ (uint32_t)a.w))) +
                    ((__popc(q[4] ^ (uint32_t)b.x) + __popc(q[5] ^ (uint32_t)b.y)) + (__popc(q[6] ^ (uint32_t)b.z) + __popc(q[7] ^ (uint32_t)b.w)));
      if (d < r.best) {      // (rows ascend inside a wave: a tie keeps the earlier row)
        r.second = r.best;
        r.best = d;
        r.idx = (int32_t)(first + t);
      } else if (d < r.second) {
        r.second = d;
      }
    }
  }
  __syncthreads();
  part[threadIdx.x] = r;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int v = 1; v < 4; v++) ham_merge(r, part[v * 64 + lane]);
  }
  return r;
}

__global__ __launch_bounds__(256) void k_hamming_match(uint32_t Q, const int32_t* __restrict__ query, uint32_t N,
                                                       const int32_t* __restrict__ db, int32_t* __restrict__ idx,
                                                       int32_t* __restrict__ best, int32_t* __restrict__ second) {
  __shared__ int4 tile[2 * HAM_TILE];
  __shared__ HamBest part[256];
  const HamBest r = ham_scan(query, Q, db, 0u, N, tile, part);
  const uint32_t qi = blockIdx.x * (uint32_t)HAM_QUERIES + threadIdx.x;
  if (threadIdx.x < HAM_QUERIES && qi < Q) {
    idx[qi] = r.idx;
    best[qi] = r.best;
    second[qi] = r.second;
  }
}

__global__ __launch_bounds__(256) void k_hamming_vote(uint32_t Q, const int32_t* __restrict__ query, uint32_t N,
                                                      const int32_t* __restrict__ db, const int32_t* __restrict__ seg,
                                                      int max_distance, float ratio, int32_t* __restrict__ votes) {
  __shared__ int4 tile[2 * HAM_TILE];
  __shared__ HamBest part[256];
  const int32_t s0 = seg[blockIdx.y], s1 = seg[blockIdx.y + 1];
  const uint32_t lo = (uint32_t)min(max(s0, 0), (int32_t)N), hi = (uint32_t)min(max(s1, (int32_t)lo), (int32_t)N);   // (never past the database)
  const HamBest r = ham_scan(query, Q, db, lo, hi, tile, part);
  if (threadIdx.x >= HAM_QUERIES) return;
  const uint32_t qi = blockIdx.x * (uint32_t)HAM_QUERIES + threadIdx.x;
  const bool pass = qi < Q && r.idx >= 0 && r.best <= max_distance && (float)r.best < __fmul_rn(ratio, (float)r.second);
  const int c = __popcll(__ballot(pass));
  if (threadIdx.x == 0 && c > 0) atomicAdd(&votes[blockIdx.y], c);
}

static inline bool orb_bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)w * h > 0x3FFFFFFF; }

extern "C" {

int64_t gsr_orb_cells(int32_t w, int32_t h) {
  if (orb_bad_image(w, h)) return 0;
  return (int64_t)((w + ORB_CELL - 1) / ORB_CELL) * ((h + ORB_CELL - 1) / ORB_CELL);
}

int gsr_orb_prepare(int32_t w, int32_t h, const float* image, int32_t channels, uint8_t* u8_out, uint16_t* box_out, void* stream) {
  if (orb_bad_image(w, h) || !image || !u8_out || !box_out || (channels != 1 && channels != 3)) {
    gsr_set_error("orb_prepare: bad arguments (%d x %d, channels = %d: expected 1 or 3)", (int)w, (int)h, (int)channels);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n = (uint32_t)w * (uint32_t)h;
  GSR_LAUNCH("orb_quantise", k_orb_quantise, dim3((n + 255u) / 256u), dim3(256), 0, st, n, image, (int)channels, u8_out);
  GSR_LAUNCH("orb_box", k_orb_box, dim3((w + 31) / 32, (h + 7) / 8), dim3(256), 0, st, (int)w, (int)h, (const uint8_t*)u8_out, box_out);
  return gsr_launch_status("orb_prepare launch");
}

int gsr_orb_detect(int32_t w, int32_t h, const uint8_t* u8, const float* mask, int32_t threshold, int32_t per_cell, int32_t* slots,
                   void* stream) {
  if (orb_bad_image(w, h) || !u8 || !slots || threshold < 0 || threshold > 254 || per_cell < 1 || per_cell > GSR_ORB_PER_CELL_MAX) {
    gsr_set_error("orb_detect: bad arguments (%d x %d, threshold = %d: expected 0 .. 254, per_cell = %d: expected 1 .. %d)", (int)w,
                  (int)h, (int)threshold, (int)per_cell, GSR_ORB_PER_CELL_MAX);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const int gx = (w + ORB_CELL - 1) / ORB_CELL, gy = (h + ORB_CELL - 1) / ORB_CELL;
  if (gy > 65535) {
    gsr_set_error("orb_detect: %d rows of cells, at most 65535", gy);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  GSR_LAUNCH("orb_detect", k_orb_detect, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, (int)w, (int)h, gx, u8, mask,
             (int)threshold, (int)per_cell, slots);
  return gsr_launch_status("orb_detect launch");
}

int gsr_orb_describe(int32_t w, int32_t h, const uint8_t* u8, const uint16_t* box, int64_t M, const int32_t* keypoints,
                     int32_t* angle_bin, int32_t* moments, int32_t* descriptors, void* stream) {
  if (orb_bad_image(w, h) || !u8 || !box || M < 0 || M > 0x3FFFFFFF || (M > 0 && (!keypoints || !angle_bin || !descriptors))) {
    gsr_set_error("orb_describe: bad arguments (%d x %d, M = %lld)", (int)w, (int)h, (long long)M);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (M == 0) return GSR_OK;
  const uint32_t m = (uint32_t)M;
  GSR_LAUNCH("orb_describe", k_orb_describe, dim3((m + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, (int)w, (int)h, u8, box, m,
             keypoints, angle_bin, moments, descriptors);
  return gsr_launch_status("orb_describe launch");
}

int gsr_orb_pattern(int8_t* out) {
  if (!out) {
    gsr_set_error("orb_pattern: NULL out");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < ORB_TABLE_BYTES; i++) out[i] = h_orb_pattern[i];
  return GSR_OK;
}

static bool ham_bad(int64_t Q, const int32_t* query, int64_t N, const int32_t* db) {      // (rows are read as 16-byte words)
  return Q < 0 || Q > 0x3FFFFFFF || N < 0 || N > 0x3FFFFFFF || (Q > 0 && !query) || (N > 0 && !db) || ((uintptr_t)query & 15u) != 0 ||
         ((uintptr_t)db & 15u) != 0;
}

int gsr_hamming_match(int64_t Q, const int32_t* query, int64_t N, const int32_t* db, int32_t* idx, int32_t* best, int32_t* second,
                      void* stream) {
  if (ham_bad(Q, query, N, db) || (Q > 0 && (!idx || !best || !second))) {
    gsr_set_error("hamming_match: bad arguments (Q = %lld, N = %lld)", (long long)Q, (long long)N);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (Q == 0) return GSR_OK;
  const uint32_t q = (uint32_t)Q;
  GSR_LAUNCH("hamming_match", k_hamming_match, dim3((q + HAM_QUERIES - 1u) / HAM_QUERIES), dim3(256), 0, (hipStream_t)stream, q,
             query, (uint32_t)N, db, idx, best, second);
  return gsr_launch_status("hamming_match launch");
}

int gsr_hamming_vote(int64_t Q, const int32_t* query, int64_t N, const int32_t* db, int64_t K, const int32_t* segments,
                     int32_t max_distance, float ratio, int32_t* votes, void* stream) {
  if (ham_bad(Q, query, N, db) || K < 0 || K > 65535 || (K > 0 && (!segments || !votes)) || max_distance < 0 || !(ratio >= 0.f)) {
    gsr_set_error("hamming_vote: bad arguments (Q = %lld, N = %lld, K = %lld: expected 0 .. 65535, max_distance = %d: expected >= 0, "
                  "ratio = %g: expected >= 0)", (long long)Q, (long long)N, (long long)K, (int)max_distance, (double)ratio);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (K == 0) return GSR_OK;
  hipStream_t st = (hipStream_t)stream;
  {
    const int rc = gsr_check(hipMemsetAsync(votes, 0, (size_t)K * 4, st), "hamming_vote: clearing the votes");
    if (rc < 0) return rc;
  }
  if (Q == 0) return GSR_OK;
  const uint32_t q = (uint32_t)Q;
  GSR_LAUNCH("hamming_vote", k_hamming_vote, dim3((q + HAM_QUERIES - 1u) / HAM_QUERIES, (uint32_t)K), dim3(256), 0, st, q, query,
             (uint32_t)N, db, segments, (int)max_distance, ratio, votes);
  return gsr_launch_status("hamming_vote launch");
}

}  // extern "C"
