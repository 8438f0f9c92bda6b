// scancontext.hip - which earlier LiDAR scan the sensor stands in again: the polar "scan context" descriptor of Kim & Kim (IROS
// 2018) - rings x sectors around the sensor, the largest height per cell - and the exhaustive search over all column shifts that
// gives a distance and a yaw together.  The rules are stated in include/gsr.h (gsr_scan_context, gsr_scan_context_distance).
//
// Descriptor, data path.  The output grids are zeroed by a memset.  A workgroup of k_scan_context owns SCX_ROWS consecutive rows of
// the cloud and one origin (grid y).  It keeps a private copy of the grid in LDS (R S words, 19.2 KB at the limits); 256 rows at
// a time come into LDS as one contiguous span of 768 floats and are read back at stride 3 (cloud_image.hip's staging); each lane
// bins its row and raises its cell with an integer atomic max in LDS - a height is >= +0, so its float bits order as unsigned
// integers.  At the end only the non-zero cells go to the output, again by integer atomic max.  A maximum does not depend on the
// order of its operands: the same bits on every run, whatever the order of the points.  No float atomics.
// k_scan_context_norms: one thread per column, rings in ascending order.
//
// Distance, data path.  One workgroup per database row: its grid and norms are staged in LDS once, each query variant in turn
// beside them (2 R S + 2 S words: 9.6 KB + 480 B at 20 x 60).  Lane s owns column shift s - one wave at S <= 64, two above: in
// the inner product over the rings lane s reads word r S + (c + s) mod S of the query grid, neighbouring lanes neighbouring words,
// and every lane the same word r S + c of the database grid, a broadcast.  Each lane's sums run in one fixed order; the lanes'
// results meet in a butterfly of (distance, variant, shift) triples ordered lexicographically, then the two waves through LDS.
#include "gsr_common.h"

// Every rule is a sequence of separately rounded operations and the tests compare bits: no implicit fma contraction in this
// file, and plain operators instead of the __f*_rn intrinsics (see image.hip).
#pragma clang fp contract(off)

#define SCX_BLOCK 256
#define SCX_ROWS 2048                 // rows of the cloud per workgroup: 8 rounds of SCX_BLOCK
#define SCX_CELLS_MAX (GSR_SCAN_CONTEXT_MAX_RINGS * GSR_SCAN_CONTEXT_MAX_SECTORS)
#define SCX_TWO_PI 6.2831855f         // float32(2 pi)
#define SCX_NONE 0x7FFFFFFF

struct ScxArgs {
  uint32_t N;
  int32_t R, S;
  int32_t has_frame;
  float F[12];
  float O[3 * GSR_SCAN_CONTEXT_MAX_ORIGINS];
  float max_range, max_range2, height_offset;
};

__device__ __forceinline__ bool scx_finite(float v) { return fabsf(v) < INFINITY; }      // (false for NaN)

__global__ __launch_bounds__(SCX_BLOCK) void k_scan_context(const ScxArgs A, const float* __restrict__ points,
                                                            uint32_t* __restrict__ out) {
  __shared__ uint32_t grid[SCX_CELLS_MAX];
  __shared__ float sh[3 * SCX_BLOCK];
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint32_t cells = (uint32_t)(A.R * A.S);
  for (uint32_t k = t; k < cells; k += (uint32_t)SCX_BLOCK) grid[k] = 0u;
  const float ox = A.O[3u * b], oy = A.O[3u * b + 1u], oz = A.O[3u * b + 2u];
  const size_t total = 3 * (size_t)A.N;
  for (uint32_t round = 0; round < (uint32_t)(SCX_ROWS / SCX_BLOCK); round++) {
    const uint32_t row0 = blockIdx.x * (uint32_t)SCX_ROWS + round * (uint32_t)SCX_BLOCK;      // (N <= 2^30 - 1: no wrap)
    if (row0 >= A.N) break;                                                                    // (the same in every lane)
    __syncthreads();      // the grid is cleared / the last round's rows have been read
    const size_t first = 3 * (size_t)row0;
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
      const size_t g = first + t + k * (uint32_t)SCX_BLOCK;
      sh[t + k * (uint32_t)SCX_BLOCK] = g < total ? points[g] : 0.f;
    }
    __syncthreads();
    if (row0 + t >= A.N) continue;
    float x = sh[3u * t], y = sh[3u * t + 1u], z = sh[3u * t + 2u];
    if (A.has_frame) {
      const float px = x, py = y, pz = z;
      x = (((A.F[0] * px) + (A.F[1] * py)) + (A.F[2] * pz)) + A.F[3];
      y = (((A.F[4] * px) + (A.F[5] * py)) + (A.F[6] * pz)) + A.F[7];
      z = (((A.F[8] * px) + (A.F[9] * py)) + (A.F[10] * pz)) + A.F[11];
    }
    x = (x - ox);
    y = (y - oy);
    z = (z - oz);
    if (!(scx_finite(x) && scx_finite(y) && scx_finite(z))) continue;
    const float rho2 = ((x * x) + (y * y));
    if (!(rho2 < A.max_range2) || rho2 == 0.f) continue;
    int ring = (int)floorf(((sqrtf(rho2) * (float)A.R) / A.max_range));
    ring = ring > A.R - 1 ? A.R - 1 : (ring < 0 ? 0 : ring);
    float theta = atan2f(y, x);
    if (theta < 0.f) theta = (theta + SCX_TWO_PI);
    int sector = (int)floorf(((theta * (float)A.S) / SCX_TWO_PI));
    sector = sector > A.S - 1 ? A.S - 1 : (sector < 0 ? 0 : sector);
    const float v = (z + A.height_offset);
    const float h = v > 0.f ? v : 0.f;      // (+0 for -0, so that the bits order as unsigned integers)
    if (h > 0.f) atomicMax(&grid[ring * A.S + sector], __float_as_uint(h));
  }
  __syncthreads();
  uint32_t* mine = out + (size_t)b * cells;
  for (uint32_t k = t; k < cells; k += (uint32_t)SCX_BLOCK) {
    const uint32_t v = grid[k];
    if (v != 0u) atomicMax(&mine[k], v);
  }
}

__global__ __launch_bounds__(SCX_BLOCK) void k_scan_context_norms(int32_t R, int32_t S, uint32_t columns,
                                                                  const float* __restrict__ desc, float* __restrict__ norms) {
  const uint32_t i = blockIdx.x * (uint32_t)SCX_BLOCK + threadIdx.x;      // b S + c
  if (i >= columns) return;
  const uint32_t b = i / (uint32_t)S, c = i - b * (uint32_t)S;
  const float* col = desc + (size_t)b * (size_t)(R * S) + c;
  float s = 0.f;
  for (int r = 0; r < R; r++) {
    const float v = col[(size_t)r * S];
    s = (s + (v * v));
  }
  norms[i] = sqrtf(s);
}

// (distance, variant, shift), smaller is better, in that order
struct ScxBest {
  float d;
  int b, s;
};
__device__ __forceinline__ bool scx_better(const ScxBest& a, const ScxBest& o) {
  return a.d < o.d || (a.d == o.d && (a.b < o.b || (a.b == o.b && a.s < o.s)));
}

__global__ __launch_bounds__(128) void k_scan_context_distance(int32_t R, int32_t S, int32_t B, const float* __restrict__ qd,
                                                               const float* __restrict__ qn, const float* __restrict__ dd,
                                                               const float* __restrict__ dn, float* __restrict__ dist,
                                                               int32_t* __restrict__ shift, int32_t* __restrict__ variant) {
  extern __shared__ float scx_lds[];      // q [R S] | d [R S] | nq [S] | nd [S] | (d, b, s) per wave
  const int cells = R * S;
  float* q = scx_lds;
  float* d = q + cells;
  float* nq = d + cells;
  float* nd = nq + S;
  float* red = nd + S;
  const int t = (int)threadIdx.x, nt = (int)blockDim.x;
  const size_t k = blockIdx.x;
  for (int i = t; i < cells; i += nt) d[i] = dd[k * (size_t)cells + i];
  for (int i = t; i < S; i += nt) nd[i] = dn[k * (size_t)S + i];
  ScxBest best = {INFINITY, SCX_NONE, SCX_NONE};
  for (int b = 0; b < B; b++) {
    __syncthreads();      // the last variant has been read
    for (int i = t; i < cells; i += nt) q[i] = qd[(size_t)b * cells + i];
    for (int i = t; i < S; i += nt) nq[i] = qn[(size_t)b * S + i];
    __syncthreads();
    if (t < S) {
      float acc = 0.f;
      int n = 0, j = t;      // j = (c + s) mod S
      for (int c = 0; c < S; c++) {
        const float a = nq[j], e = nd[c];
        if (a != 0.f && e != 0.f) {
          float dot = 0.f;
          for (int r = 0; r < R; r++) dot = (dot + (q[r * S + j] * d[r * S + c]));
          acc = (acc + (dot / (a * e)));
          n++;
        }
        j = j + 1 == S ? 0 : j + 1;
      }
      const ScxBest mine = {n ? (1.0f - (acc / (float)n)) : 1.0f, b, t};
      if (scx_better(mine, best)) best = mine;      // (a NaN never wins, whichever variant it comes from)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const ScxBest other = {__shfl_xor(best.d, o, 64), __shfl_xor(best.b, o, 64), __shfl_xor(best.s, o, 64)};
    if (scx_better(other, best)) best = other;
  }
  if (nt > GSR_WAVE) {      // S > 64: the second wave's winner through LDS
    if (t == GSR_WAVE) {
      red[0] = best.d;
      red[1] = __int_as_float(best.b);
      red[2] = __int_as_float(best.s);
    }
    __syncthreads();
    if (t == 0) {
      const ScxBest other = {red[0], __float_as_int(red[1]), __float_as_int(red[2])};
      if (scx_better(other, best)) best = other;
    }
  }
  if (t == 0) {
    dist[k] = best.d;
    shift[k] = best.s;
    variant[k] = best.b;
  }
}

static bool scx_bad_geometry(int32_t rings, int32_t sectors, int32_t B) {
  return rings < 1 || rings > GSR_SCAN_CONTEXT_MAX_RINGS || sectors < 1 || sectors > GSR_SCAN_CONTEXT_MAX_SECTORS || B < 1 ||
         B > GSR_SCAN_CONTEXT_MAX_ORIGINS;
}

extern "C" {

int gsr_scan_context(int64_t N, const float* points, const float* frame, int32_t B, const float* origins, int32_t rings,
                     int32_t sectors, float max_range, float height_offset, float* descriptors, float* norms, void* stream) {
  if (scx_bad_geometry(rings, sectors, B)) {
    gsr_set_error("scan_context: rings = %d outside [1, %d], sectors = %d outside [1, %d] or B = %d outside [1, %d]", (int)rings,
                  GSR_SCAN_CONTEXT_MAX_RINGS, (int)sectors, GSR_SCAN_CONTEXT_MAX_SECTORS, (int)B, GSR_SCAN_CONTEXT_MAX_ORIGINS);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (N < 0 || N > 0x3FFFFFFFll) {
    gsr_set_error("scan_context: N = %lld outside [0, 2^30 - 1]", (long long)N);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!descriptors || !norms || (N > 0 && !points)) {
    gsr_set_error("scan_context: NULL descriptors / norms, or NULL points with N = %lld", (long long)N);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!origins && B != 1) {
    gsr_set_error("scan_context: NULL origins (one origin, 0 0 0) with B = %d", (int)B);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!(max_range > 0.f) || !(max_range < INFINITY)) {
    gsr_set_error("scan_context: max_range = %g (finite, > 0)", (double)max_range);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!(fabsf(height_offset) < INFINITY)) {
    gsr_set_error("scan_context: height_offset = %g (finite)", (double)height_offset);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  ScxArgs A;
  A.N = (uint32_t)N;
  A.R = rings;
  A.S = sectors;
  A.has_frame = frame ? 1 : 0;
  for (int i = 0; i < 12; i++) {
    A.F[i] = frame ? frame[i] : (i % 5 == 0 ? 1.f : 0.f);
    if (!(fabsf(A.F[i]) < INFINITY)) {
      gsr_set_error("scan_context: frame[%d] is not finite", i);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  for (int i = 0; i < 3 * GSR_SCAN_CONTEXT_MAX_ORIGINS; i++) {
    A.O[i] = origins && i < 3 * B ? origins[i] : 0.f;
    if (!(fabsf(A.O[i]) < INFINITY)) {
      gsr_set_error("scan_context: origins[%d] is not finite", i);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  A.max_range = max_range;
  A.max_range2 = max_range * max_range;
  A.height_offset = height_offset;
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)rings * (size_t)sectors;
  const int rc = gsr_check(hipMemsetAsync(descriptors, 0, (size_t)B * cells * sizeof(float), st), "scan_context: memset");
  if (rc != GSR_OK) return rc;
  if (A.N > 0u)
    GSR_LAUNCH("scan_context", k_scan_context, dim3((A.N + SCX_ROWS - 1u) / SCX_ROWS, (uint32_t)B), dim3(SCX_BLOCK), 0, st, A,
               points, (uint32_t*)descriptors);
  const uint32_t columns = (uint32_t)(B * sectors);
  GSR_LAUNCH("scan_context_norms", k_scan_context_norms, dim3((columns + SCX_BLOCK - 1u) / SCX_BLOCK), dim3(SCX_BLOCK), 0, st,
             rings, sectors, columns, (const float*)descriptors, norms);
  return gsr_launch_status("scan_context launch");
}

int gsr_scan_context_distance(int32_t rings, int32_t sectors, int32_t B, const float* query, const float* query_norms, int64_t K,
                              const float* db, const float* db_norms, float* dist, int32_t* shift, int32_t* variant,
                              void* stream) {
  if (scx_bad_geometry(rings, sectors, B)) {
    gsr_set_error("scan_context_distance: rings = %d outside [1, %d], sectors = %d outside [1, %d] or B = %d outside [1, %d]",
                  (int)rings, GSR_SCAN_CONTEXT_MAX_RINGS, (int)sectors, GSR_SCAN_CONTEXT_MAX_SECTORS, (int)B,
                  GSR_SCAN_CONTEXT_MAX_ORIGINS);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (K < 0 || K > 0x3FFFFFFFll) {
    gsr_set_error("scan_context_distance: K = %lld outside [0, 2^30 - 1]", (long long)K);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!query || !query_norms || (K > 0 && (!db || !db_norms || !dist || !shift || !variant))) {
    gsr_set_error("scan_context_distance: NULL query / query_norms, or NULL db / db_norms / dist / shift / variant with K = %lld",
                  (long long)K);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (K == 0) return GSR_OK;
  const size_t lds = (2 * (size_t)rings * (size_t)sectors + 2 * (size_t)sectors + 4) * sizeof(float);
  GSR_LAUNCH("scan_context_distance", k_scan_context_distance, dim3((uint32_t)K), dim3(sectors <= GSR_WAVE ? GSR_WAVE : 128), lds,
             (hipStream_t)stream, rings, sectors, B, query, query_norms, db, db_norms, dist, shift, variant);
  return gsr_launch_status("scan_context_distance launch");
}

}  // extern "C"
