// pointcloud.hip - conditioning of a sensor point cloud before it seeds Gaussians: what the reference's process_point_cloud
// (submodules/ros_workspace/src/gs_slam_msgs/scripts/pointcloud_pcd.py:163-209) does with Open3D on the host.
//
// gsr_voxel_down_sample: one averaged point per occupied voxel.
//   1. lattice origin: the caller's, or min - voxel / 2 of the finite coordinates (gsr_knn_bbox, csrc/knn.hip);
//   2. per point the cell index of every axis - fsub, fdiv, floorf, one correctly rounded float32 operation each - biased by 2^20
//      and packed 21 + 21 + 21 bits into one 64-bit cell word; a dropped row (non-finite, or out of range: status) is ~0;
//   3. three stable radix sorts of the row permutation, by the x, then y, then z field of the cell word (LSD over the axes): rows
//      end in ascending (i_z, i_y, i_x), the rows of one voxel in their original order, the dropped rows behind everything (bit 21
//      of the z key).  The sort takes 32-bit keys and its `bits` on the host, and the grid's extent only exists on the device, so
//      a linearised key "where the extent fits" would cost a read-back to choose it; three sorts of 21-bit keys never need one;
//   4. head flags (first row of a run of equal cell words), gsr_scan_u32 -> voxel ids, run starts;
//   5. segmented reduction split by run length, as k_tile_depth_sort splits by list length: a run of <= GSR_VOXEL_SHORT rows is
//      summed by one thread; a longer one is appended to a list (integer atomic: the list's order changes nothing that is
//      stored) and summed by a whole workgroup - thread t takes rows t, t + 256, ..., then gsr_block_sum (gsr_common.h: a fixed
//      butterfly over the wave and the four wave sums in order).  Sums in float64, mean in float64, rounded to float32
//      once.  Which path a run takes and the order of its additions depend on its sorted rows only: two runs give the same
//      bits.
//
// gsr_statistical_outliers: mean distance to the nb - 1 nearest neighbours (gsr_knn_k_launch), its mean and standard deviation
//   over the finite rows in float64 (fixed slices per workgroup, one final workgroup - the pattern of gsr_l1_mean_*), two passes
//   as Open3D does it (mean first, then squared deviations), the threshold and the keep mask - nothing visits the host.
#include "gsr_common.h"

#define GSR_VOXEL_SHORT 64          // rows one thread may walk
#define GSR_VOXEL_BIAS 1048576      // 2^20: cell indices live in [-2^20, 2^20)
#define GSR_VOXEL_DROPPED 0xFFFFFFFFFFFFFFFFull
#define GSR_VOXEL_LONG_BLOCKS 1024
#define GSR_STAT_BLOCKS 256

struct VoxelWs {
  float *bbox_part, *bbox;           // gsr_knn_bbox's scratch and result
  unsigned long long* cell;          // u64[P]
  uint32_t *key[2], *val[2];         // u32[P] each
  uint32_t *flag, *offs;             // u32[P] each
  uint32_t* start;                   // u32[P + 1]
  uint32_t* longlist;                // u32[P / 64 + 1]
  uint32_t* meta;                    // u32[64]: [0] entries of longlist
  uint32_t *scan_tmp, *radix_tmp;
  size_t total;
};
static VoxelWs voxel_ws(void* base, size_t P) {
  GsrCarve c(base);
  VoxelWs w;
  if (P == 0) P = 1;
  w.bbox_part = c.take<float>(GSR_KNN_BBOX_PART);
  w.bbox = c.take<float>(64);
  w.cell = c.take<unsigned long long>(P);
  for (int i = 0; i < 2; i++) w.key[i] = c.take<uint32_t>(P);
  for (int i = 0; i < 2; i++) w.val[i] = c.take<uint32_t>(P);
  w.flag = c.take<uint32_t>(P);
  w.offs = c.take<uint32_t>(P);
  w.start = c.take<uint32_t>(P + 1);
  w.longlist = c.take<uint32_t>(P / GSR_VOXEL_SHORT + 1);
  w.meta = c.take<uint32_t>(64);
  w.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(P));
  w.radix_tmp = c.take<uint32_t>(gsr_radix_tmp_elems(P));
  w.total = c.o;
  return w;
}

struct GsrVoxelGrid {
  float voxel;
  float origin[3];
  int has_origin;
};

// cell word of every row and the first sort's key (its x field)
__global__ __launch_bounds__(256) void k_voxel_cell(uint32_t P, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                    GsrVoxelGrid g, unsigned long long* __restrict__ cell,
                                                    uint32_t* __restrict__ key, int64_t* __restrict__ count_dev) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  unsigned long long c = 0ull;
  bool keep = true, range = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float p = pts[3 * (size_t)i + a];
    const float o = g.has_origin ? g.origin[a] : __fsub_rn(bbox[a], __fmul_rn(0.5f, g.voxel));
    const float f = floorf(__fdiv_rn(__fsub_rn(p, o), g.voxel));
    if (!knn_finite(p)) keep = false;
    else if (!(f >= -(float)GSR_VOXEL_BIAS && f < (float)GSR_VOXEL_BIAS)) range = false;      // (a NaN index too)
    else c |= (unsigned long long)(uint32_t)((int)f + GSR_VOXEL_BIAS) << (21 * a);
  }
  if (keep && !range) count_dev[1] = 1;      // (every such thread stores the same value)
  if (!keep || !range) c = GSR_VOXEL_DROPPED;
  cell[i] = c;
  key[i] = (uint32_t)(c & 0x1FFFFFull);
}

// the next sort's key: a field of the cell word of the row at every sorted position
__global__ __launch_bounds__(256) void k_voxel_key(uint32_t P, const unsigned long long* __restrict__ cell,
                                                   const uint32_t* __restrict__ perm, int shift, uint32_t mask,
                                                   uint32_t* __restrict__ key) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < P) key[j] = (uint32_t)(cell[perm[j]] >> shift) & mask;
}

__global__ __launch_bounds__(256) void k_voxel_flag(uint32_t P, const unsigned long long* __restrict__ cell,
                                                    const uint32_t* __restrict__ perm, uint32_t* __restrict__ flag) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P) return;
  const unsigned long long c = cell[perm[j]];
  flag[j] = (c != GSR_VOXEL_DROPPED && (j == 0u || c != cell[perm[j - 1u]])) ? 1u : 0u;
}

// start[v] = first sorted position of voxel v, start[n_voxels] = number of kept rows; count_dev[0] = n_voxels
__global__ __launch_bounds__(256) void k_voxel_starts(uint32_t P, const unsigned long long* __restrict__ cell,
                                                      const uint32_t* __restrict__ perm, const uint32_t* __restrict__ flag,
                                                      const uint32_t* __restrict__ offs, uint32_t* __restrict__ start,
                                                      int64_t* __restrict__ count_dev) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P) return;
  const uint32_t f = flag[j], o = offs[j];
  if (f) start[o] = j;
  if (cell[perm[j]] != GSR_VOXEL_DROPPED && (j == P - 1u || cell[perm[j + 1u]] == GSR_VOXEL_DROPPED)) {      // the last kept row
    start[o + f] = j + 1u;
    count_dev[0] = (int64_t)(o + f);
  }
}

struct GsrVoxelOut {
  float* points;
  float* colors;      // NULL: no colours
  int32_t* npts;      // NULL: not wanted
  uint32_t capacity;
};

__device__ __forceinline__ void voxel_store(const GsrVoxelOut& out, uint32_t v, const double s[6], uint32_t len) {
  if (v >= out.capacity) return;
  const double n = (double)len;
#pragma unroll
  for (int a = 0; a < 3; a++) out.points[3 * (size_t)v + a] = (float)(s[a] / n);
  if (out.colors) {
#pragma unroll
    for (int a = 0; a < 3; a++) out.colors[3 * (size_t)v + a] = (float)(s[3 + a] / n);
  }
  if (out.npts) out.npts[v] = (int32_t)len;
}

// one thread per voxel: sums a short run, lists a long one
__global__ __launch_bounds__(256) void k_voxel_reduce_short(uint32_t P, const int64_t* __restrict__ count_dev,
                                                            const uint32_t* __restrict__ start, const uint32_t* __restrict__ perm,
                                                            const float* __restrict__ pts, const float* __restrict__ cols,
                                                            GsrVoxelOut out, uint32_t* __restrict__ longlist,
                                                            uint32_t* __restrict__ meta) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const int64_t nv = count_dev[0];
  if (v >= P || (int64_t)v >= nv) return;
  const uint32_t s0 = start[v], s1 = start[v + 1u], len = s1 - s0;
  if (len > (uint32_t)GSR_VOXEL_SHORT) {
    longlist[atomicAdd(&meta[0], 1u)] = v;      // (at most P / 65 of them: the list holds P / 64 + 1)
    return;
  }
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t j = s0; j < s1; j++) {
    const size_t i = (size_t)perm[j];
#pragma unroll
    for (int a = 0; a < 3; a++) s[a] += (double)pts[3 * i + a];
    if (out.colors) {
#pragma unroll
      for (int a = 0; a < 3; a++) s[3 + a] += (double)cols[3 * i + a];
    }
  }
  voxel_store(out, v, s, len);
}

// one workgroup per listed voxel
__global__ __launch_bounds__(256) void k_voxel_reduce_long(const uint32_t* __restrict__ meta, const uint32_t* __restrict__ longlist,
                                                           const uint32_t* __restrict__ start, const uint32_t* __restrict__ perm,
                                                           const float* __restrict__ pts, const float* __restrict__ cols,
                                                           GsrVoxelOut out) {
  const uint32_t nlong = meta[0];
  for (uint32_t li = blockIdx.x; li < nlong; li += gridDim.x) {      // (uniform over the workgroup)
    const uint32_t v = longlist[li];
    const uint32_t s0 = start[v], s1 = start[v + 1u];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = s0 + threadIdx.x; j < s1; j += 256u) {
      const size_t i = (size_t)perm[j];
#pragma unroll
      for (int a = 0; a < 3; a++) s[a] += (double)pts[3 * i + a];
      if (out.colors) {
#pragma unroll
        for (int a = 0; a < 3; a++) s[3 + a] += (double)cols[3 * i + a];
      }
    }
    gsr_block_sum(s);
    if (threadIdx.x == 0) voxel_store(out, v, s, s1 - s0);
    __syncthreads();      // (the next round writes the sum's LDS again)
  }
}

// ---- statistical outlier filter -----------------------------------------------------------------------------------------------
struct OutlierWs {
  void* knn;         // gsr_knn_k's workspace
  float* dbar;       // float[P] (mean_dist == NULL)
  double* part;      // double[GSR_STAT_BLOCKS][2]
  double* stats;     // double[4] (stats_dev == NULL)
  size_t total;
};
static OutlierWs outlier_ws(void* base, size_t P) {
  GsrCarve c(base);
  OutlierWs w;
  if (P == 0) P = 1;
  w.knn = c.bytes(gsr_knn_k_workspace_bytes((int64_t)P));
  w.dbar = c.take<float>(P);
  w.part = c.take<double>((size_t)GSR_STAT_BLOCKS * 2);
  w.stats = c.take<double>(32);
  w.total = c.o;
  return w;
}

// MODE 0: (sum of dbar, number of finite dbar) of this workgroup's rows; MODE 1: (sum of (dbar - mu)^2, 0)
template <int MODE>
__global__ __launch_bounds__(256) void k_outlier_partial(uint32_t P, const float* __restrict__ dbar,
                                                         const double* __restrict__ stats, double* __restrict__ part) {
  const double mu = MODE == 1 ? stats[1] : 0.0;
  double s[2] = {0.0, 0.0};      // the sum, the count
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < P; i += gridDim.x * 256u) {
    const float d = dbar[i];
    if (knn_finite(d)) {
      if (MODE == 0) {
        s[0] += (double)d;
        s[1] += 1.0;
      } else {
        const double e = __dsub_rn((double)d, mu);
        s[0] = __dadd_rn(s[0], __dmul_rn(e, e));
      }
    }
  }
  gsr_block_sum_store(s, part);
}

// one workgroup: MODE 0 -> stats[0] = n_valid, stats[1] = mu; MODE 1 -> stats[2] = sigma, stats[3] = threshold
template <int MODE>
__global__ __launch_bounds__(256) void k_outlier_final(uint32_t nblk, const double* __restrict__ part, double std_ratio,
                                                       double* __restrict__ stats) {
  double s[2];      // the sum, the count
  gsr_block_sum_rows(s, part, nblk);
  if (threadIdx.x != 0) return;
  if (MODE == 0) {
    stats[0] = s[1];
    stats[1] = s[1] > 0.0 ? s[0] / s[1] : 0.0;
  } else {
    const double n = stats[0], mu = stats[1];
    const double sigma = n >= 2.0 ? sqrt(s[0] / (n - 1.0)) : 0.0;
    stats[2] = sigma;
    stats[3] = __dadd_rn(mu, __dmul_rn(std_ratio, sigma));
  }
}

__global__ __launch_bounds__(256) void k_outlier_keep(uint32_t P, const float* __restrict__ dbar, const double* __restrict__ stats,
                                                      uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  const float d = dbar[i];      // (NaN - a non-finite row - fails both comparisons)
  keep[i] = (d > 0.f && (double)d < stats[3]) ? 1 : 0;
}

extern "C" {

size_t gsr_voxel_workspace_bytes(int64_t P) { return voxel_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_voxel_down_sample(int64_t P, const float* points, const float* colors, float voxel_size, const float* origin,
                          float* out_points, float* out_colors, int32_t* out_npts, int64_t capacity, int64_t* count_dev,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const bool origin_ok = !origin || (fabsf(origin[0]) < KNN_INF && fabsf(origin[1]) < KNN_INF && fabsf(origin[2]) < KNN_INF);
  if (gsr_bad_size(P) || !points || !count_dev || !workspace || capacity < 0 || (capacity > 0 && !out_points) ||
      (capacity > 0 && colors && !out_colors) || !(voxel_size > 0.f) || !(voxel_size < KNN_INF) || !origin_ok) {
    gsr_set_error("voxel_down_sample: bad arguments (P = %lld, voxel_size = %g, capacity = %lld)", (long long)P,
                  (double)voxel_size, (long long)capacity);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const VoxelWs w = voxel_ws(workspace, (size_t)P);
  if (!gsr_workspace_fits("voxel_down_sample", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n = (uint32_t)P, nblk = (n + 255u) / 256u;

  GsrVoxelGrid g;
  g.voxel = voxel_size;
  g.has_origin = origin ? 1 : 0;
  for (int a = 0; a < 3; a++) g.origin[a] = origin ? origin[a] : 0.f;
  (void)hipMemsetAsync(count_dev, 0, 2 * sizeof(int64_t), st);
  (void)hipMemsetAsync(w.meta, 0, 256, st);
  if (!origin) gsr_knn_bbox(P, points, w.bbox_part, w.bbox, st);
  GSR_LAUNCH("voxel_cell", k_voxel_cell, dim3(nblk), dim3(256), 0, st, n, points, (const float*)w.bbox, g, w.cell, w.key[0],
             count_dev);
  // LSD over the axes: x, y, z; `at` = the buffer pair that holds the permutation so far
  int at = gsr_radix_sort_pairs(w.key[0], w.val[0], w.key[1], w.val[1], true, (size_t)n, 21, w.radix_tmp, st);
  for (int axis = 1; axis < 3; axis++) {
    const int bits = axis == 2 ? 22 : 21;      // (bit 21 of the z key: a dropped row)
    GSR_LAUNCH("voxel_key", k_voxel_key, dim3(nblk), dim3(256), 0, st, n, (const unsigned long long*)w.cell,
               (const uint32_t*)w.val[at], 21 * axis, (1u << bits) - 1u, w.key[at]);
    const int r = gsr_radix_sort_pairs(w.key[at], w.val[at], w.key[at ^ 1], w.val[at ^ 1], false, (size_t)n, bits, w.radix_tmp, st);
    at ^= r;
  }
  const uint32_t* perm = w.val[at];
  GSR_LAUNCH("voxel_flag", k_voxel_flag, dim3(nblk), dim3(256), 0, st, n, (const unsigned long long*)w.cell, perm, w.flag);
  gsr_scan_u32(w.flag, nullptr, w.offs, (size_t)n, 0, w.scan_tmp, st);
  GSR_LAUNCH("voxel_starts", k_voxel_starts, dim3(nblk), dim3(256), 0, st, n, (const unsigned long long*)w.cell, perm,
             (const uint32_t*)w.flag, (const uint32_t*)w.offs, w.start, count_dev);
  GsrVoxelOut out;
  out.points = out_points;
  out.colors = (colors && out_colors) ? out_colors : nullptr;
  out.npts = out_npts;
  out.capacity = (uint32_t)(capacity > 0x7FFFFFFF ? 0x7FFFFFFF : capacity);
  GSR_LAUNCH("voxel_reduce_short", k_voxel_reduce_short, dim3(nblk), dim3(256), 0, st, n, (const int64_t*)count_dev,
             (const uint32_t*)w.start, perm, points, colors, out, w.longlist, w.meta);
  const uint32_t max_long = n / (uint32_t)(GSR_VOXEL_SHORT + 1);
  if (max_long > 0u) {
    const uint32_t lblk = max_long < (uint32_t)GSR_VOXEL_LONG_BLOCKS ? max_long : (uint32_t)GSR_VOXEL_LONG_BLOCKS;
    GSR_LAUNCH("voxel_reduce_long", k_voxel_reduce_long, dim3(lblk), dim3(256), 0, st, (const uint32_t*)w.meta,
               (const uint32_t*)w.longlist, (const uint32_t*)w.start, perm, points, colors, out);
  }
  return gsr_launch_status("voxel_down_sample launch");
}

size_t gsr_outlier_workspace_bytes(int64_t P) { return outlier_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_statistical_outliers(int64_t P, const float* points, int32_t nb_neighbors, double std_ratio, uint8_t* keep,
                             float* mean_dist, double* stats_dev, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(P) || !points || !keep || !workspace || nb_neighbors < 2 || nb_neighbors > GSR_KNN_K_MAX + 1 ||
      !(fabs(std_ratio) < (double)KNN_INF)) {
    gsr_set_error("statistical_outliers: bad arguments (P = %lld, nb_neighbors = %d: expected 2 .. %d, std_ratio = %g)",
                  (long long)P, (int)nb_neighbors, GSR_KNN_K_MAX + 1, std_ratio);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const OutlierWs w = outlier_ws(workspace, (size_t)P);
  if (!gsr_workspace_fits("statistical_outliers", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n = (uint32_t)P, nblk = (n + 255u) / 256u;
  float* dbar = mean_dist ? mean_dist : w.dbar;
  double* part = w.part;
  double* stats = stats_dev ? stats_dev : w.stats;
  gsr_knn_k_launch(P, points, (int)nb_neighbors - 1, nullptr, dbar, w.knn, st);
  const uint32_t sblk = nblk < (uint32_t)GSR_STAT_BLOCKS ? nblk : (uint32_t)GSR_STAT_BLOCKS;
  GSR_LAUNCH("outlier_sum", k_outlier_partial<0>, dim3(sblk), dim3(256), 0, st, n, (const float*)dbar, (const double*)stats, part);
  GSR_LAUNCH("outlier_mean", k_outlier_final<0>, dim3(1), dim3(256), 0, st, sblk, (const double*)part, std_ratio, stats);
  GSR_LAUNCH("outlier_dev", k_outlier_partial<1>, dim3(sblk), dim3(256), 0, st, n, (const float*)dbar, (const double*)stats, part);
  GSR_LAUNCH("outlier_sigma", k_outlier_final<1>, dim3(1), dim3(256), 0, st, sblk, (const double*)part, std_ratio, stats);
  GSR_LAUNCH("outlier_keep", k_outlier_keep, dim3(nblk), dim3(256), 0, st, n, (const float*)dbar, (const double*)stats, keep);
  return gsr_launch_status("statistical_outliers launch");
}

}  // extern "C"
