// features.hip - global registration without a prior: what the reference's pointcloud_registeration (convert_visual_merged_msg.py
// :198-213) would take from Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching to give ICP its
// `init` (include/gsr.h has the full contracts).
//
// gsr_compute_fpfh: a copy of the cloud with the rows whose point OR normal is not finite turned into NaN NaN NaN (nobody's
//   neighbour, and no part of the bounding box or the sort), the structure of knn.hip over THAT copy, the normals gathered into
//   sorted order, then up to three sweeps (knn_sweep, knn_common.h) over the boxes:
//   1. k_fpfh_bound<K>: min(r2, d_k) per row by knn_topk_bound (skipped for max_nn = 0, where the bound is r2);
//   2. k_fpfh_spfh: per row (knn_member_walk here and in 3.) the 3 x 11 histogram of the pair features of its members, as
//      INTEGER counts - exact and independent of the order the members are met in - kept by sorted position, with m = the
//      number of members;
//   3. k_fpfh_sum: per row sum SPFH_j / d2 over its members in float64, in sorted-structure order, the three blocks scaled to
//      100, the row's own SPFH added, one rounding to float32.
//   The 33 bins of a thread are indexed at run time: they live in LDS as bins[b][thread] (consecutive lanes, consecutive words),
//   not in a register array that would go to scratch.  One wave per workgroup: 8.25 KiB of counts / 16.5 KiB of sums each, no
//   barrier between waves, and 9 000 rows spread over 141 CUs instead of 36.
// gsr_feature_nn: brute force over 33-vectors.  256 queries per workgroup, each thread's query in 33 registers; target rows
//   staged through LDS 128 at a time (36-float pitch: nine 16-byte reads per row, the same address in every lane - a broadcast);
//   the target range split over gridDim.y when the queries alone cannot fill the CUs.  Every split folds its (d2, row) minimum
//   into one 64-bit word per query by an INTEGER atomicMin on (bits of d2) << 32 | row - d2 >= +0, so the order of the bit
//   patterns is the order of the values - the lexicographic minimum whatever the split or the order of arrival.
// gsr_ransac_feature_matching: trial t is a pure function of (seed, t).  k_ransac_hyp, one thread per trial: counter-based
//   samples, the checkers, Horn's closed form (horn_common.h, the Jacobi matrices per thread in LDS); survivors compacted in
//   trial order by the library's scan; k_ransac_score, one thread per survivor, walks ALL pairs (staged through LDS, read as
//   broadcasts) in their order - an integer count and a float64 sum in a fixed order, no reduction; one workgroup then takes
//   the lexicographic best of (count max, sum min, trial min) - a minimum over a total order - against the caller's record.
#include "knn_common.h"
#include "horn_common.h"

#define GSR_FPFH_BLOCK 64
#define GSR_FPFH_BINS GSR_FPFH_WIDTH
#define GSR_FEAT_BLOCK 256
#define GSR_FEAT_TILE GSR_FEATURE_NN_TILE          // target rows per LDS tile
#define GSR_FEAT_PITCH4 9                          // float4 per staged row: 33 values + 3 of padding
#define GSR_FEAT_WGS GSR_FEATURE_NN_WORKGROUPS     // workgroups aimed at: two per CU
#define GSR_RANSAC_BLOCK 64
#define GSR_RANSAC_TILE 256        // pairs per LDS tile of the scoring kernel
#define GSR_PI 3.14159265358979323846

// ==== FPFH ==========================================================================================================================
struct FpfhWs {
  GsrNnWs nn;
  float* masked;     // float[P][3]: the points, NaN NaN NaN where the point or the normal is not finite - what the structure is built over
  float4* nrm;       // float4[P]: the normal of every sorted position
  float* bound;      // float[P]: min(r2, d_k) per sorted position (max_nn > 0)
  int32_t* spfh;     // int32[P][33]: the SPFH counts per sorted position
  int32_t* m;        // int32[P]: members besides the row itself
  size_t total;
};
static FpfhWs fpfh_ws(void* base, size_t P) {
  GsrCarve c(base);
  FpfhWs w;
  if (P == 0) P = 1;
  w.nn = nn_carve(c, P);
  w.masked = c.take<float>(3 * P);
  w.nrm = c.take<float4>(P);
  w.bound = c.take<float>(P);
  w.spfh = c.take<int32_t>(P * GSR_FPFH_BINS);
  w.m = c.take<int32_t>(P);
  w.total = c.o;
  return w;
}

// the cloud the structure is built over: a row whose point or normal is not finite becomes NaN NaN NaN BEFORE the build, so it
// takes no part in the bounding box, the Morton sort or the boxes
__global__ __launch_bounds__(256) void k_fpfh_mask(uint32_t P, const float* __restrict__ points, const float* __restrict__ normals,
                                                   float* __restrict__ masked) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  const float nx = normals[3 * (size_t)i], ny = normals[3 * (size_t)i + 1], nz = normals[3 * (size_t)i + 2];
  if (!(knn_finite(x) && knn_finite(y) && knn_finite(z) && knn_finite(nx) && knn_finite(ny) && knn_finite(nz)))
    x = y = z = __builtin_nanf("");
  masked[3 * (size_t)i] = x;
  masked[3 * (size_t)i + 1] = y;
  masked[3 * (size_t)i + 2] = z;
}

// normals into sorted order (the sorted points of a masked row are NaN NaN NaN already; knn_mask_non_finite keeps them so)
__global__ __launch_bounds__(256) void k_fpfh_prepare(uint32_t P, float4* __restrict__ pts, const float* __restrict__ normals,
                                                      float4* __restrict__ nrm) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P) return;
  const float4 p = pts[j];
  const size_t row = (size_t)__float_as_uint(p.w);
  pts[j] = knn_mask_non_finite(p);
  nrm[j] = make_float4(normals[3 * row], normals[3 * row + 1], normals[3 * row + 2], 0.f);
}

// min(r2, d_k) per sorted position: what k_normals (normals.hip) takes from the same call
template <int K>
__global__ __launch_bounds__(256) void k_fpfh_bound(GsrKnnTree t, int k, float r2, float* __restrict__ bound) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const bool active = q < t.P;
  const uint32_t pos = active ? q : 0u;
  float b[K];
  const float d = knn_topk_bound<K, 256>(t, t.pts[pos], pos, active, k, r2, s_lo, s_hi, b);
  if (active) bound[pos] = d;
}

__device__ __forceinline__ int fpfh_bin(double scaled) {      // floor, clamped to 0 .. 10 (a NaN: 0)
  return (int)fmin(10.0, fmax(0.0, floor(scaled)));
}

// the three bins of the pair (i, j): delta = p_j - p_i (float32 differences, promoted), ni / nj the normals (include/gsr.h)
__device__ __forceinline__ void fpfh_pair(double dx, double dy, double dz, const float4 ni, const float4 nj, int& b0, int& b1,
                                          int& b2) {
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  if (d2 > 0.0) {
    const double d = sqrt(d2);
    const double ix = (double)ni.x, iy = (double)ni.y, iz = (double)ni.z, jx = (double)nj.x, jy = (double)nj.y, jz = (double)nj.z;
    const double a1 = ((ix * dx + iy * dy) + iz * dz) / d, a2 = ((jx * dx + jy * dy) + jz * dz) / d;
    const bool sw = fabs(a1) < fabs(a2);
    const double ax = sw ? jx : ix, ay = sw ? jy : iy, az = sw ? jz : iz;      // n1
    const double bx = sw ? ix : jx, by = sw ? iy : jy, bz = sw ? iz : jz;      // n2
    const double ex = sw ? -dx : dx, ey = sw ? -dy : dy, ez = sw ? -dz : dz;
    double vx = ey * az - ez * ay, vy = ez * ax - ex * az, vz = ex * ay - ey * ax;      // delta x n1
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn > 0.0) {
      vx /= vn; vy /= vn; vz /= vn;
      const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;      // n1 x v
      f1 = (vx * bx + vy * by) + vz * bz;
      f0 = atan2((wx * bx + wy * by) + wz * bz, (ax * bx + ay * by) + az * bz);
      f2 = sw ? -a2 : a1;
    }
  }
  b0 = fpfh_bin(11.0 * (f0 + GSR_PI) / (2.0 * GSR_PI));
  b1 = fpfh_bin(11.0 * (f1 + 1.0) / 2.0);
  b2 = fpfh_bin(11.0 * (f2 + 1.0) / 2.0);
}

// (a masked row is NaN in every component: it walks nothing)
// The one search kernel that takes the tree's arrays as arguments of its own and puts the GsrKnnTree together itself: its visit
// writes memory (the LDS bins), and only loads through `const ... __restrict__` kernel arguments stay scalar loads next to that -
// through pointers read out of a by-value struct the wave-uniform loads of the box AABBs and points become vector loads (measured:
// 5 - 6 % of the kernel, profiles/knn_sweep_refactor.txt).
__global__ __launch_bounds__(GSR_FPFH_BLOCK) void k_fpfh_spfh(uint32_t P, float r2, const float* __restrict__ bound_of,
                                                              const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                                              const float4* __restrict__ box_lo,
                                                              const float4* __restrict__ box_hi, uint32_t nbox,
                                                              const float4* __restrict__ sup_lo,
                                                              const float4* __restrict__ sup_hi, uint32_t nsuper,
                                                              int32_t* __restrict__ spfh, int32_t* __restrict__ m_of,
                                                              int32_t* __restrict__ counts_out, int32_t* __restrict__ count_out) {
  __shared__ float4 s_lo[GSR_FPFH_BLOCK], s_hi[GSR_FPFH_BLOCK];
  __shared__ int32_t bins[GSR_FPFH_BINS * GSR_FPFH_BLOCK];
  const GsrKnnTree t{pts, box_lo, box_hi, sup_lo, sup_hi, P, nbox, nsuper};
  const uint32_t q = blockIdx.x * (uint32_t)GSR_FPFH_BLOCK + threadIdx.x;
  const bool live = q < t.P;
  const uint32_t pos = live ? q : 0u;
  const float4 me = t.pts[pos];
  const bool active = live && knn_finite(me.x);
  const float4 ni = nrm[pos];
  const float bound = bound_of ? bound_of[pos] : r2;
#pragma unroll
  for (int b = 0; b < GSR_FPFH_BINS; b++) bins[b * GSR_FPFH_BLOCK + threadIdx.x] = 0;
  int32_t members = 0;
  knn_member_walk<GSR_FPFH_BLOCK>(
      t, me, pos, active, bound, s_lo, s_hi,
      [&](const uint32_t j, const float fx, const float fy, const float fz) __attribute__((always_inline)) {
        int b0, b1, b2;
        fpfh_pair(-(double)fx, -(double)fy, -(double)fz, ni, nrm[j], b0, b1, b2);
        members++;
        bins[b0 * GSR_FPFH_BLOCK + threadIdx.x]++;
        bins[(11 + b1) * GSR_FPFH_BLOCK + threadIdx.x]++;
        bins[(22 + b2) * GSR_FPFH_BLOCK + threadIdx.x]++;
      });
  if (!live) return;
  const size_t row = (size_t)__float_as_uint(me.w);
  const bool finite = active;
  m_of[pos] = members;
  if (count_out) count_out[row] = finite ? members + 1 : 0;
  for (int b = 0; b < GSR_FPFH_BINS; b++) {
    const int32_t c = bins[b * GSR_FPFH_BLOCK + threadIdx.x];
    spfh[(size_t)pos * GSR_FPFH_BINS + b] = c;
    if (counts_out) counts_out[row * GSR_FPFH_BINS + b] = c;
  }
}

__global__ __launch_bounds__(GSR_FPFH_BLOCK) void k_fpfh_sum(GsrKnnTree t, float r2, const float* __restrict__ bound_of,
                                                             const int32_t* __restrict__ spfh,
                                                             const int32_t* __restrict__ m_of, float* __restrict__ fpfh) {
  __shared__ float4 s_lo[GSR_FPFH_BLOCK], s_hi[GSR_FPFH_BLOCK];
  __shared__ double acc[GSR_FPFH_BINS * GSR_FPFH_BLOCK];
  const uint32_t q = blockIdx.x * (uint32_t)GSR_FPFH_BLOCK + threadIdx.x;
  const bool live = q < t.P;
  const uint32_t pos = live ? q : 0u;
  const float4 me = t.pts[pos];
  const bool active = live && knn_finite(me.x);
  const float bound = bound_of ? bound_of[pos] : r2;
#pragma unroll
  for (int b = 0; b < GSR_FPFH_BINS; b++) acc[b * GSR_FPFH_BLOCK + threadIdx.x] = 0.0;
  knn_member_walk<GSR_FPFH_BLOCK>(
      t, me, pos, active, bound, s_lo, s_hi,
      [&](const uint32_t j, const float fx, const float fy, const float fz) __attribute__((always_inline)) {
        const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int32_t mj = m_of[j];
        if (d2 > 0.0 && mj > 0) {
          // SPFH_j(b) / d2 = 100 c / (m_j d2); an empty bin adds +0 to a sum that is >= +0: skipped
          const double w = 100.0 / ((double)mj * d2);
          const int32_t* __restrict__ cj = spfh + (size_t)j * GSR_FPFH_BINS;
          for (int b = 0; b < GSR_FPFH_BINS; b++) {
            const int32_t c = cj[b];
            if (c != 0) acc[b * GSR_FPFH_BLOCK + threadIdx.x] += (double)c * w;
          }
        }
      });
  if (!live) return;
  const size_t row = (size_t)__float_as_uint(me.w);
  float* __restrict__ out = fpfh + row * GSR_FPFH_BINS;
  const int32_t m = m_of[pos];
  if (!knn_finite(me.x)) {
    for (int b = 0; b < GSR_FPFH_BINS; b++) out[b] = __builtin_nanf("");
    return;
  }
  for (int blk = 0; blk < 3; blk++) {
    double sum = 0.0;
    for (int b = 0; b < 11; b++) sum += acc[(11 * blk + b) * GSR_FPFH_BLOCK + threadIdx.x];
    const double scale = sum != 0.0 ? 100.0 / sum : 0.0;
    for (int b = 0; b < 11; b++) {
      const int bb = 11 * blk + b;
      const double own = m > 0 ? 100.0 * (double)spfh[(size_t)pos * GSR_FPFH_BINS + bb] / (double)m : 0.0;
      out[bb] = (float)(acc[bb * GSR_FPFH_BLOCK + threadIdx.x] * scale + own);
    }
  }
}

// ==== feature matching =================================================================================================================
__global__ __launch_bounds__(GSR_FEAT_BLOCK) void k_feature_nn(uint32_t Nq, uint32_t Nt, const float* __restrict__ query,
                                                               const float* __restrict__ target, uint32_t tiles_per_split,
                                                               unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[GSR_FEAT_TILE * GSR_FEAT_PITCH4];
  const uint32_t i = blockIdx.x * (uint32_t)GSR_FEAT_BLOCK + threadIdx.x;
  const bool active = i < Nq;
  float qv[GSR_FPFH_BINS];
#pragma unroll
  for (int b = 0; b < GSR_FPFH_BINS; b++) qv[b] = active ? query[(size_t)i * GSR_FPFH_BINS + b] : 0.f;
  const uint32_t ntiles = (Nt + GSR_FEAT_TILE - 1u) / GSR_FEAT_TILE;
  const uint32_t t0 = blockIdx.y * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
  float bd = KNN_INF;
  uint32_t br = GSR_NONE;
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t first = t * (uint32_t)GSR_FEAT_TILE, rows = min((uint32_t)GSR_FEAT_TILE, Nt - first);
    __syncthreads();
    {
      float* __restrict__ flat = (float*)tile;
      const float* __restrict__ src = target + (size_t)first * GSR_FPFH_BINS;
      for (uint32_t e = threadIdx.x; e < rows * GSR_FPFH_BINS; e += (uint32_t)GSR_FEAT_BLOCK)
        flat[(e / GSR_FPFH_BINS) * (GSR_FEAT_PITCH4 * 4) + e % GSR_FPFH_BINS] = src[e];
    }
    __syncthreads();
    for (uint32_t r = 0; r < rows; r++) {
      const float4* __restrict__ tr = tile + r * GSR_FEAT_PITCH4;
      float d2 = 0.f;
#pragma unroll
      for (int v = 0; v < 8; v++) {
        const float4 x = tr[v];
        float e;
        e = __fsub_rn(qv[4 * v], x.x);     d2 = __fmaf_rn(e, e, d2);
        e = __fsub_rn(qv[4 * v + 1], x.y); d2 = __fmaf_rn(e, e, d2);
        e = __fsub_rn(qv[4 * v + 2], x.z); d2 = __fmaf_rn(e, e, d2);
        e = __fsub_rn(qv[4 * v + 3], x.w); d2 = __fmaf_rn(e, e, d2);
      }
      const float e = __fsub_rn(qv[32], tr[8].x);
      d2 = __fmaf_rn(e, e, d2);
      const uint32_t row = first + r;
      if (d2 < bd || (d2 == bd && row < br)) {      // (false for a NaN on either side)
        bd = d2;
        br = row;
      }
    }
  }
  if (active && br != GSR_NONE) atomicMin(&keys[i], ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned long long)br);
}

__global__ __launch_bounds__(256) void k_feature_nn_finish(uint32_t Nq, const float* __restrict__ query,
                                                           const unsigned long long* __restrict__ keys,
                                                           int32_t* __restrict__ idx, float* __restrict__ dist2) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= Nq) return;
  const unsigned long long key = keys[i];
  if (key != ~0ull) {
    idx[i] = (int32_t)(uint32_t)(key & 0xFFFFFFFFull);
    if (dist2) dist2[i] = __uint_as_float((uint32_t)(key >> 32));
    return;
  }
  bool nan = false;
  for (int b = 0; b < GSR_FPFH_BINS; b++) nan = nan || query[(size_t)i * GSR_FPFH_BINS + b] != query[(size_t)i * GSR_FPFH_BINS + b];
  idx[i] = -1;
  if (dist2) dist2[i] = nan ? __builtin_nanf("") : KNN_INF;      // (no target row without a NaN: +inf)
}

// ==== RANSAC ============================================================================================================================
struct RansacWs {
  uint32_t* meta;       // u32[64]: [0] = survivors of this call
  float4* pairs;        // float4[2 M]: (s, valid), (t, 0)
  uint32_t* flag;       // u32[n]: 1 = the trial survived the checkers
  uint32_t* offset;     // u32[n]: exclusive scan of the flags
  uint32_t* list;       // u32[n]: the survivors, in trial order
  double* hyp;          // double[n][12]: rows 0 .. 2 of the trial's T
  long long* count;     // int64[n]: per survivor
  double* sum;          // double[n]
  uint32_t* scan_tmp;
  size_t total;
};
static RansacWs ransac_ws(void* base, size_t M, size_t n) {
  GsrCarve c(base);
  RansacWs w;
  if (M == 0) M = 1;
  if (n == 0) n = 1;
  w.meta = c.take<uint32_t>(64);
  w.pairs = c.take<float4>(2 * M);
  w.flag = c.take<uint32_t>(n);
  w.offset = c.take<uint32_t>(n);
  w.list = c.take<uint32_t>(n);
  w.hyp = c.take<double>(12 * n);
  w.count = c.take<long long>(n);
  w.sum = c.take<double>(n);
  w.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(n));
  w.total = c.o;
  return w;
}

// the points of every pair, once per call; a pair that names a row outside its cloud or a non-finite point: flag 0
__global__ __launch_bounds__(256) void k_ransac_gather(uint32_t M, const int32_t* __restrict__ pairs, uint32_t Ps,
                                                       const float* __restrict__ src, uint32_t Pt, const float* __restrict__ tgt,
                                                       float4* __restrict__ pp) {
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= M) return;
  const int32_t a = pairs[2 * (size_t)m], b = pairs[2 * (size_t)m + 1];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a >= 0 && (uint32_t)a < Ps && b >= 0 && (uint32_t)b < Pt) {
    s = make_float4(src[3 * (size_t)a], src[3 * (size_t)a + 1], src[3 * (size_t)a + 2], 1.f);
    t = make_float4(tgt[3 * (size_t)b], tgt[3 * (size_t)b + 1], tgt[3 * (size_t)b + 2], 0.f);
    if (!(knn_finite(s.x) && knn_finite(s.y) && knn_finite(s.z) && knn_finite(t.x) && knn_finite(t.y) && knn_finite(t.z))) {
      s = make_float4(0.f, 0.f, 0.f, 0.f);
      t = s;
    }
  }
  pp[2 * (size_t)m] = s;
  pp[2 * (size_t)m + 1] = t;
}

__device__ __forceinline__ uint64_t ransac_mix(uint64_t z) {      // the splitmix64 finaliser
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// status of a trial: 0 survived; 1 two samples coincide; 2 a sampled pair is unusable; 3 edge lengths; 4 no rotation; 5 distance
template <int N>
__global__ __launch_bounds__(GSR_RANSAC_BLOCK) void k_ransac_hyp(uint32_t n, uint64_t t0, uint64_t seed, uint32_t M,
                                                                 const float4* __restrict__ pp, double md2, double theta,
                                                                 uint32_t* __restrict__ flag, double* __restrict__ hyp,
                                                                 int32_t* __restrict__ dbg_samples, int32_t* __restrict__ dbg_status,
                                                                 double* __restrict__ dbg_T) {
  __shared__ double sA[16 * GSR_RANSAC_BLOCK], sV[16 * GSR_RANSAC_BLOCK];
  const uint32_t k = blockIdx.x * (uint32_t)GSR_RANSAC_BLOCK + threadIdx.x;
  if (k >= n) return;      // (no barrier below)
  const uint64_t t = t0 + (uint64_t)k;
  uint32_t idx[N];
#pragma unroll
  for (int s = 0; s < N; s++) {
    const uint64_t z = ransac_mix(seed + (8ull * t + (uint64_t)s + 1ull) * 0x9E3779B97F4A7C15ull);
    idx[s] = (uint32_t)(((z >> 32) * (uint64_t)M) >> 32);
  }
  int st = 0;
#pragma unroll
  for (int a = 0; a < N; a++)
#pragma unroll
    for (int b = a + 1; b < N; b++)
      if (idx[a] == idx[b]) st = 1;
  double S[N][3], Q[N][3];
  if (st == 0) {
    bool ok = true;
#pragma unroll
    for (int s = 0; s < N; s++) {
      const float4 a = pp[2 * (size_t)idx[s]], b = pp[2 * (size_t)idx[s] + 1];
      ok = ok && a.w != 0.f;
      S[s][0] = (double)a.x; S[s][1] = (double)a.y; S[s][2] = (double)a.z;
      Q[s][0] = (double)b.x; Q[s][1] = (double)b.y; Q[s][2] = (double)b.z;
    }
    if (!ok) st = 2;
  }
  if (st == 0 && theta > 0.0) {
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
      for (int b = a + 1; b < N; b++) {
        const double sx = S[a][0] - S[b][0], sy = S[a][1] - S[b][1], sz = S[a][2] - S[b][2];
        const double tx = Q[a][0] - Q[b][0], ty = Q[a][1] - Q[b][1], tz = Q[a][2] - Q[b][2];
        const double ds = sqrt((sx * sx + sy * sy) + sz * sz), dt = sqrt((tx * tx + ty * ty) + tz * tz);
        if (!(ds >= theta * dt && dt >= theta * ds)) st = 3;
      }
  }
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = 0.0;
  if (st == 0) {
    double qb[3] = {0.0, 0.0, 0.0}, pb[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < N; s++)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        qb[a] += S[s][a];
        pb[a] += Q[s][a];
      }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      qb[a] /= (double)N;
      pb[a] /= (double)N;
    }
    double Mx[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < N; s++) v += (S[s][a] - qb[a]) * (Q[s][b] - pb[b]);
        Mx[a][b] = v;
      }
    double R[3][3], eig;
    const HornMat4Strided<GSR_RANSAC_BLOCK> A{sA + threadIdx.x}, V{sV + threadIdx.x};
    if (!horn_rotation(Mx, A, V, R, eig)) {
      st = 4;
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        T[4 * a] = R[a][0]; T[4 * a + 1] = R[a][1]; T[4 * a + 2] = R[a][2];
        T[4 * a + 3] = pb[a] - ((R[a][0] * qb[0] + R[a][1] * qb[1]) + R[a][2] * qb[2]);
      }
#pragma unroll
      for (int s = 0; s < N; s++) {
        double d2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double e = (((T[4 * a] * S[s][0] + T[4 * a + 1] * S[s][1]) + T[4 * a + 2] * S[s][2]) + T[4 * a + 3]) - Q[s][a];
          d2 += e * e;
        }
        if (!(d2 <= md2)) st = 5;
      }
    }
  }
  flag[k] = st == 0 ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 12; i++) hyp[(size_t)k * 12 + i] = T[i];
  if (dbg_samples) {
#pragma unroll
    for (int s = 0; s < 8; s++) dbg_samples[(size_t)k * 8 + s] = s < N ? (int32_t)idx[s < N ? s : 0] : -1;
  }
  if (dbg_status) dbg_status[k] = st;
  if (dbg_T) {
#pragma unroll
    for (int i = 0; i < 12; i++) dbg_T[(size_t)k * 16 + i] = T[i];
    dbg_T[(size_t)k * 16 + 12] = dbg_T[(size_t)k * 16 + 13] = dbg_T[(size_t)k * 16 + 14] = 0.0;
    dbg_T[(size_t)k * 16 + 15] = (st == 0 || st == 5) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_ransac_compact(uint32_t n, const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ offset, uint32_t* __restrict__ list,
                                                        uint32_t* __restrict__ meta) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t f = flag[k], o = offset[k];
  if (f) list[o] = k;      // (o < n: an exclusive scan of 0 / 1 flags)
  if (k == n - 1u) meta[0] = o + f;
}

__global__ __launch_bounds__(GSR_RANSAC_BLOCK) void k_ransac_score(uint32_t M, const float4* __restrict__ pp,
                                                                   const uint32_t* __restrict__ meta,
                                                                   const uint32_t* __restrict__ list,
                                                                   const double* __restrict__ hyp, double md2,
                                                                   long long* __restrict__ count_out, double* __restrict__ sum_out) {
  __shared__ float4 tile[2 * GSR_RANSAC_TILE];
  const uint32_t nsurv = meta[0];
  if (blockIdx.x * (uint32_t)GSR_RANSAC_BLOCK >= nsurv) return;      // (uniform over the workgroup)
  const uint32_t k = blockIdx.x * (uint32_t)GSR_RANSAC_BLOCK + threadIdx.x;
  const bool active = k < nsurv;
  const size_t h = (size_t)list[active ? k : 0u];
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = hyp[h * 12 + i];
  long long count = 0;
  double sum = 0.0;
  for (uint32_t base = 0; base < M; base += (uint32_t)GSR_RANSAC_TILE) {
    const uint32_t rows = min((uint32_t)GSR_RANSAC_TILE, M - base);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < 2u * rows; e += (uint32_t)GSR_RANSAC_BLOCK) tile[e] = pp[2 * (size_t)base + e];
    __syncthreads();
    if (!active) continue;
    for (uint32_t r = 0; r < rows; r++) {
      const float4 s = tile[2 * r], q = tile[2 * r + 1];
      if (s.w == 0.f) continue;      // (uniform: the same pair in every lane)
      const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
      const double ex = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - (double)q.x;
      const double ey = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - (double)q.y;
      const double ez = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - (double)q.z;
      const double d2 = (ex * ex + ey * ey) + ez * ez;
      if (d2 <= md2) {
        count++;
        sum += d2;
      }
    }
  }
  if (active) {
    count_out[k] = count;
    sum_out[k] = sum;
  }
}

// the record of include/gsr.h (gsr_ransac_best) as the kernels address it: 20 eight-byte words
#define RB_COUNT 0
#define RB_SUM 1
#define RB_TRIAL 2
#define RB_T 3
#define RB_CHECKED 19

__device__ __forceinline__ bool ransac_better(long long c, double s, long long t, long long bc, double bs, long long bt) {
  return c > bc || (c == bc && (s < bs || (s == bs && t < bt)));
}

// one workgroup: the best survivor of this call against the caller's record
__global__ __launch_bounds__(256) void k_ransac_best(uint64_t t0, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ list,
                                                     const double* __restrict__ hyp, const long long* __restrict__ count_of,
                                                     const double* __restrict__ sum_of, double* __restrict__ best) {
  __shared__ long long s_c[256], s_t[256];
  __shared__ double s_s[256];
  __shared__ uint32_t s_k[256];
  const uint32_t nsurv = meta[0];
  if (nsurv == 0u) return;      // the record is untouched
  long long bc = -1, bt = 0x7FFFFFFFFFFFFFFFll;
  double bs = (double)KNN_INF;
  uint32_t bk = 0u;
  for (uint32_t k = threadIdx.x; k < nsurv; k += 256u) {
    const long long c = count_of[k], t = (long long)(t0 + (uint64_t)list[k]);
    const double s = sum_of[k];
    if (ransac_better(c, s, t, bc, bs, bt)) {
      bc = c; bs = s; bt = t; bk = k;
    }
  }
  s_c[threadIdx.x] = bc; s_s[threadIdx.x] = bs; s_t[threadIdx.x] = bt; s_k[threadIdx.x] = bk;
  __syncthreads();
  for (uint32_t o = 128u; o > 0u; o >>= 1) {
    if (threadIdx.x < o && ransac_better(s_c[threadIdx.x + o], s_s[threadIdx.x + o], s_t[threadIdx.x + o], s_c[threadIdx.x],
                                         s_s[threadIdx.x], s_t[threadIdx.x])) {
      s_c[threadIdx.x] = s_c[threadIdx.x + o]; s_s[threadIdx.x] = s_s[threadIdx.x + o];
      s_t[threadIdx.x] = s_t[threadIdx.x + o]; s_k[threadIdx.x] = s_k[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  long long* __restrict__ bi = (long long*)best;
  bi[RB_CHECKED] += (long long)nsurv;
  if (!ransac_better(s_c[0], s_s[0], s_t[0], bi[RB_COUNT], best[RB_SUM], bi[RB_TRIAL])) return;
  bi[RB_COUNT] = s_c[0];
  best[RB_SUM] = s_s[0];
  bi[RB_TRIAL] = s_t[0];
  const size_t h = (size_t)list[s_k[0]];
  for (int i = 0; i < 12; i++) best[RB_T + i] = hyp[h * 12 + i];
  best[RB_T + 12] = best[RB_T + 13] = best[RB_T + 14] = 0.0;
  best[RB_T + 15] = 1.0;
}

extern "C" {

size_t gsr_fpfh_workspace_bytes(int64_t P) { return fpfh_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_compute_fpfh(int64_t P, const float* points, const float* normals, float radius, int32_t max_nn, float* fpfh,
                     int32_t* spfh_counts, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  const bool radius_only = max_nn == 0;
  if (gsr_bad_size(P) || !points || !normals || !fpfh || !workspace || !(radius > 0.f) ||
      !(radius_only ? radius < KNN_INF : (max_nn >= 3 && max_nn <= GSR_KNN_K_MAX + 1))) {
    gsr_set_error("compute_fpfh: bad arguments (P = %lld, radius = %g: expected > 0, max_nn = %d: expected 3 .. %d, or 0 with a "
                  "finite radius)", (long long)P, (double)radius, (int)max_nn, GSR_KNN_K_MAX + 1);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const FpfhWs w = fpfh_ws(workspace, (size_t)P);
  if (!gsr_workspace_fits("compute_fpfh", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const GsrKnnTree t = knn_tree(w.nn, (size_t)P);
  const uint32_t n = t.P, nblk = (n + 255u) / 256u;
  GSR_LAUNCH("fpfh_mask", k_fpfh_mask, dim3(nblk), dim3(256), 0, st, n, points, normals, w.masked);
  gsr_knn_build(P, w.masked, w.nn, st);
  const uint32_t fblk = (n + GSR_FPFH_BLOCK - 1u) / GSR_FPFH_BLOCK;
  float* bound = radius_only ? nullptr : w.bound;
  GSR_LAUNCH("fpfh_prepare", k_fpfh_prepare, dim3(nblk), dim3(256), 0, st, n, w.nn.pts, normals, w.nrm);
  const float r2 = radius * radius;      // the float32 square (+inf stays, and a large radius may become, +inf)
  if (!radius_only) {
    const int k = (int)max_nn - 1;
#define FPFH_BOUND_K(K) GSR_LAUNCH("fpfh_bound_k" #K, k_fpfh_bound<K>, dim3(nblk), dim3(256), 0, st, t, k, r2, bound)
    GSR_KNN_PICK_K(k, FPFH_BOUND_K);
#undef FPFH_BOUND_K
  }
  GSR_LAUNCH("fpfh_spfh", k_fpfh_spfh, dim3(fblk), dim3(GSR_FPFH_BLOCK), 0, st, t.P, r2, (const float*)bound, t.pts,
             (const float4*)w.nrm, t.box_lo, t.box_hi, t.nbox, t.sup_lo, t.sup_hi, t.nsuper, w.spfh, w.m, spfh_counts, count_out);
  GSR_LAUNCH("fpfh_sum", k_fpfh_sum, dim3(fblk), dim3(GSR_FPFH_BLOCK), 0, st, t, r2, (const float*)bound, (const int32_t*)w.spfh,
             (const int32_t*)w.m, fpfh);
  return gsr_launch_status("compute_fpfh launch");
}

// the workspace of gsr_feature_nn: one packed (distance bits, target row) key per query, reduced by atomicMin over the splits
struct FeatureNnWs {
  unsigned long long* keys;      // u64[Nq]
  size_t total;
};
static FeatureNnWs feature_nn_ws(void* base, size_t Nq) {
  GsrCarve c(base);
  FeatureNnWs w;
  w.keys = c.take<unsigned long long>(Nq);
  w.total = c.o;
  return w;
}
size_t gsr_feature_nn_workspace_bytes(int64_t Nq) { return feature_nn_ws(nullptr, (size_t)(Nq < 1 ? 1 : Nq)).total; }

int32_t gsr_feature_nn_tiles_per_split(int64_t Nq, int64_t Nt) {
  if (gsr_bad_size(Nq) || gsr_bad_size(Nt)) return 0;
  const uint64_t qblk = ((uint64_t)Nq + GSR_FEAT_BLOCK - 1) / GSR_FEAT_BLOCK, ntiles = ((uint64_t)Nt + GSR_FEAT_TILE - 1) / GSR_FEAT_TILE;
  uint64_t splits = (GSR_FEAT_WGS + qblk - 1) / qblk;
  if (splits > ntiles) splits = ntiles;
  if (splits > 65535u) splits = 65535u;
  return (int32_t)((ntiles + splits - 1) / splits);
}

int gsr_feature_nn(int64_t Nq, const float* query, int64_t Nt, const float* target, int32_t width, int32_t* idx_out,
                   float* dist2_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Nq) || gsr_bad_size(Nt) || !query || !target || !idx_out || !workspace || width != GSR_FPFH_BINS) {
    gsr_set_error("feature_nn: bad arguments (Nq = %lld, Nt = %lld, width = %d: expected %d)", (long long)Nq, (long long)Nt,
                  (int)width, GSR_FPFH_BINS);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const FeatureNnWs w = feature_nn_ws(workspace, (size_t)Nq);
  if (!gsr_workspace_fits("feature_nn", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nq = (uint32_t)Nq, nt = (uint32_t)Nt, qblk = (nq + GSR_FEAT_BLOCK - 1u) / GSR_FEAT_BLOCK;
  const uint32_t ntiles = (nt + GSR_FEAT_TILE - 1u) / GSR_FEAT_TILE;
  const uint32_t tps = (uint32_t)gsr_feature_nn_tiles_per_split(Nq, Nt), splits = (ntiles + tps - 1u) / tps;
  unsigned long long* keys = w.keys;
  {
    const int rc = gsr_check(hipMemsetAsync(keys, 0xFF, (size_t)nq * 8, st), "feature_nn: clearing the keys");
    if (rc < 0) return rc;
  }
  GSR_LAUNCH("feature_nn", k_feature_nn, dim3(qblk, splits), dim3(GSR_FEAT_BLOCK), 0, st, nq, nt, query, target, tps, keys);
  GSR_LAUNCH("feature_nn_finish", k_feature_nn_finish, dim3((nq + 255u) / 256u), dim3(256), 0, st, nq, query,
             (const unsigned long long*)keys, idx_out, dist2_out);
  return gsr_launch_status("feature_nn launch");
}

size_t gsr_ransac_workspace_bytes(int64_t M, int64_t n) {
  return ransac_ws(nullptr, (size_t)(M < 1 ? 1 : M), (size_t)(n < 1 ? 1 : n)).total;
}

int gsr_ransac_feature_matching(int64_t Ps, const float* source, int64_t Pt, const float* target, int64_t M, const int32_t* pairs,
                                float max_distance, int32_t ransac_n, float edge_length_threshold, uint64_t seed, int64_t t0,
                                int64_t n, gsr_ransac_best* best, void* workspace, size_t workspace_bytes,
                                const gsr_ransac_debug* debug, void* stream) {
  if (gsr_bad_size(Ps) || gsr_bad_size(Pt) || gsr_bad_size(M) || !source || !target || !pairs || !best || !workspace ||
      !(max_distance >= 0.f && max_distance < KNN_INF) || ransac_n < 3 || ransac_n > GSR_RANSAC_N_MAX ||
      !(edge_length_threshold >= 0.f && edge_length_threshold <= 1.f) || t0 < 0 || n < 1 || n > GSR_RANSAC_MAX_TRIALS ||
      t0 > (int64_t)1 << 56) {
    gsr_set_error("ransac_feature_matching: bad arguments (Ps = %lld, Pt = %lld, M = %lld, max_distance = %g: expected finite "
                  ">= 0, ransac_n = %d: expected 3 .. %d, edge_length_threshold = %g: expected 0 .. 1, trials [%lld, + %lld): "
                  "expected 1 .. %d per call)", (long long)Ps, (long long)Pt, (long long)M, (double)max_distance, (int)ransac_n,
                  GSR_RANSAC_N_MAX, (double)edge_length_threshold, (long long)t0, (long long)n, GSR_RANSAC_MAX_TRIALS);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const RansacWs w = ransac_ws(workspace, (size_t)M, (size_t)n);
  if (!gsr_workspace_fits("ransac_feature_matching", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t m = (uint32_t)M, nn = (uint32_t)n, hblk = (nn + GSR_RANSAC_BLOCK - 1u) / GSR_RANSAC_BLOCK;
  const double md2 = (double)max_distance * (double)max_distance, theta = (double)edge_length_threshold;
  int32_t* ds = debug ? debug->samples : nullptr;
  int32_t* dst = debug ? debug->status : nullptr;
  double* dT = debug ? debug->T : nullptr;
  GSR_LAUNCH("ransac_gather", k_ransac_gather, dim3((m + 255u) / 256u), dim3(256), 0, st, m, pairs, (uint32_t)Ps, source,
             (uint32_t)Pt, target, w.pairs);
#define RANSAC_HYP(N)                                                                                                     \
  case N:                                                                                                                 \
    GSR_LAUNCH("ransac_hyp_n" #N, k_ransac_hyp<N>, dim3(hblk), dim3(GSR_RANSAC_BLOCK), 0, st, nn, (uint64_t)t0, seed, m,   \
               (const float4*)w.pairs, md2, theta, w.flag, w.hyp, ds, dst, dT);                                           \
    break
  switch (ransac_n) {
    RANSAC_HYP(3);
    RANSAC_HYP(4);
    RANSAC_HYP(5);
    RANSAC_HYP(6);
    RANSAC_HYP(7);
    RANSAC_HYP(8);
  }
#undef RANSAC_HYP
  gsr_scan_u32(w.flag, nullptr, w.offset, (size_t)nn, 0, w.scan_tmp, st);
  GSR_LAUNCH("ransac_compact", k_ransac_compact, dim3((nn + 255u) / 256u), dim3(256), 0, st, nn, (const uint32_t*)w.flag,
             (const uint32_t*)w.offset, w.list, w.meta);
  GSR_LAUNCH("ransac_score", k_ransac_score, dim3(hblk), dim3(GSR_RANSAC_BLOCK), 0, st, m, (const float4*)w.pairs,
             (const uint32_t*)w.meta, (const uint32_t*)w.list, (const double*)w.hyp, md2, w.count, w.sum);
  GSR_LAUNCH("ransac_best", k_ransac_best, dim3(1), dim3(256), 0, st, (uint64_t)t0, (const uint32_t*)w.meta,
             (const uint32_t*)w.list, (const double*)w.hyp, (const long long*)w.count, (const double*)w.sum, (double*)best);
  return gsr_launch_status("ransac_feature_matching launch");
}

}  // extern "C"
