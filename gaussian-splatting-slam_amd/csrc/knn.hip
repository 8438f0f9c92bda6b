// knn.hip - the mapping half's two native calls: exact 3-nearest-neighbour distances (what the reference takes from
// `simple_knn._C.distCUDA2`, scene/gaussian_model.py:20,:140) and the back-projection of an RGB-D keyframe into new points.
//
// gsr_knn_dist2: mean squared distance of every point to its three nearest OTHER points, exact.
//   1. bounding box of the finite coordinates: per-workgroup min / max over a fixed slice, then one workgroup over the partials
//      (min / max are order-independent: deterministic without any ordering argument, and no float atomics);
//   2. 30-bit Morton code per point (10 bits per axis of the box), sorted with the library's stable radix sort (value = index);
//   3. the points gathered in sorted order as float4 (xyz, original index), cut into BOXES of GSR_KNN_BOX = 64 consecutive
//      points (one wave builds one box: its AABB by cross-lane min / max) and SUPER-BOXES of GSR_KNN_SUPER = 64 consecutive
//      boxes (4096 points);
//   4. one thread per query, queries in Morton order so that the lanes of a wave accept the same boxes: an upper bound of the
//      third-nearest distance from the six neighbours in Morton order, then knn_sweep (knn_common.h: ALL super-boxes, their
//      AABBs staged through LDS 256 at a time, descending only where the AABB distance does not exceed the radius) with the
//      radius min(bound, current third best).
//   The structure only prunes (the rounding argument stands next to knn_sweep).  The answer of a query is the three smallest
//   values of a multiset that does not depend on the traversal: two runs, and runs with a different first_query, give the same
//   bits.
//   Box size: 64 = one wave builds a box, and a leaf visit is 64 distance evaluations against a box test of about the same cost
//   as two of them; with 64 x 64 the sweep at 5 M points is 1.2 k super-box tests per query (a single level of 64-point boxes
//   would be 78 k).  Distances are (a-b).(a-b) from differences: scenes sit far from the origin.
//   Fewer than four points: the mean runs over the min(3, P-1) neighbours that exist, P == 1 gives 0.  (The upstream module is
//   recalled to leave FLT_MAX-derived values there; nothing in the reference pins either behaviour.)
//   Non-finite coordinates never enter the bounding box, get Morton code 0 where the quantisation is undefined, and fail every
//   `<` comparison: no hang, no out-of-bounds access, unspecified values for those rows.
//
// gsr_knn_k: the same search for k = 1 .. 32 neighbours - every squared distance in ascending order and / or the mean of their
//   square roots (what a statistical outlier filter thresholds; csrc/pointcloud.hip): knn_topk_bound (knn_common.h) without a
//   cut.  The per-thread list is knn_insert generalised: a fully unrolled compare-exchange chain over a compile-time size K in
//   {4, 8, 16, 32}, the smallest that holds k (GSR_KNN_PICK_K).
//   The K - k slots that are not needed start at -inf and stay at the head of the list, so list[K - 1] is the k-th smallest
//   candidate - the same pruning threshold a list of exactly k entries would give - and no register is ever indexed at run time.
//
// gsr_unproject_rgbd: strided pixels of a depth image -> world-space points + colours, selected by validity and (optionally) by
//   what the map's render of the same view does not explain, compacted in row-major pixel order by a prefix sum.
#include "knn_common.h"

// the workspace of gsr_knn_dist2 and gsr_knn_k: the structure's blob (knn_common.h), then what a subset of queries needs
struct KnnWs {
  GsrNnWs nn;
  uint32_t *qflag, *qpos, *qlist;   // u32[P] each: first_query > 0 only - query flags in sorted order, their scan, the compacted list
  uint32_t* scan_tmp;
  size_t total;
};
static KnnWs knn_ws(void* base, size_t P) {
  GsrCarve c(base);
  KnnWs w;
  if (P == 0) P = 1;
  w.nn = nn_carve(c, P);
  w.qflag = c.take<uint32_t>(P);
  w.qpos = c.take<uint32_t>(P);
  w.qlist = c.take<uint32_t>(P);
  w.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(P));
  w.total = c.o;
  return w;
}

// min / max of six per-thread values over a 256-thread workgroup -> out[6] (thread 0 writes)
__device__ __forceinline__ void knn_block_minmax(float lo[3], float hi[3], float* __restrict__ out) {
  __shared__ float s[4][6];
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = knn_wave_min(lo[a]);
    hi[a] = knn_wave_max(hi[a]);
  }
  if (gsr_lane() == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      s[w][a] = lo[a];
      s[w][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = s[0][a];
    for (int k = 1; k < 4; k++) v = a < 3 ? fminf(v, s[k][a]) : fmaxf(v, s[k][a]);
    out[a] = v;
  }
}

__global__ __launch_bounds__(256) void k_knn_bbox_partial(uint32_t P, const float* __restrict__ pts, float* __restrict__ part) {
  float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < P; i += gridDim.x * 256u) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = pts[3 * (size_t)i + a];
      if (knn_finite(v)) {
        lo[a] = fminf(lo[a], v);
        hi[a] = fmaxf(hi[a], v);
      }
    }
  }
  knn_block_minmax(lo, hi, part + 6 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void k_knn_bbox_final(uint32_t nblk, const float* __restrict__ part, float* __restrict__ bbox) {
  float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
  for (uint32_t b = threadIdx.x; b < nblk; b += 256u) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      lo[a] = fminf(lo[a], part[6 * (size_t)b + a]);
      hi[a] = fmaxf(hi[a], part[6 * (size_t)b + 3 + a]);
    }
  }
  knn_block_minmax(lo, hi, bbox);
}

__global__ __launch_bounds__(256) void k_knn_morton(uint32_t P, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                    uint32_t* __restrict__ codes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  codes[i] = knn_morton_code(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], bbox);
}

// one wave per box: gathers its 64 points into sorted order and reduces their AABB
__global__ __launch_bounds__(256) void k_knn_boxes(uint32_t P, const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                   float4* __restrict__ sorted, float4* __restrict__ box_lo,
                                                   float4* __restrict__ box_hi, uint32_t first_query,
                                                   uint32_t* __restrict__ qflag) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;      // sorted position; box = j / 64 = one wave
  float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
  if (j < P) {
    const uint32_t i = order[j];
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    sorted[j] = make_float4(x, y, z, __uint_as_float(i));
    if (qflag) qflag[j] = i >= first_query ? 1u : 0u;
    lo[0] = hi[0] = x;      // (fminf / fmaxf drop a NaN operand: a box of NaN points keeps +inf / -inf and is never entered)
    lo[1] = hi[1] = y;
    lo[2] = hi[2] = z;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = knn_wave_min(lo[a]);
    hi[a] = knn_wave_max(hi[a]);
  }
  const uint32_t b = j >> 6;
  if (gsr_lane() == 0 && (size_t)b * GSR_KNN_BOX < P) {
    box_lo[b] = make_float4(lo[0], lo[1], lo[2], 0.f);
    box_hi[b] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

// one wave per super-box: lane l holds box l of it
__global__ __launch_bounds__(256) void k_knn_supers(uint32_t nbox, const float4* __restrict__ box_lo,
                                                    const float4* __restrict__ box_hi, float4* __restrict__ sup_lo,
                                                    float4* __restrict__ sup_hi) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  float4 lo = make_float4(KNN_INF, KNN_INF, KNN_INF, 0.f), hi = make_float4(-KNN_INF, -KNN_INF, -KNN_INF, 0.f);
  if (b < nbox) {
    lo = box_lo[b];
    hi = box_hi[b];
  }
  lo.x = knn_wave_min(lo.x); lo.y = knn_wave_min(lo.y); lo.z = knn_wave_min(lo.z);
  hi.x = knn_wave_max(hi.x); hi.y = knn_wave_max(hi.y); hi.z = knn_wave_max(hi.z);
  const uint32_t s = b >> 6;
  if (gsr_lane() == 0 && s * (uint32_t)GSR_KNN_SUPER < nbox) {
    sup_lo[s] = lo;
    sup_hi[s] = hi;
  }
}

// first_query > 0: the sorted positions that hold a query, in sorted order
__global__ __launch_bounds__(256) void k_knn_compact(uint32_t P, const uint32_t* __restrict__ qflag,
                                                     const uint32_t* __restrict__ qpos, uint32_t* __restrict__ qlist) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < P && qflag[j]) qlist[qpos[j]] = j;
}

__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2) {
  if (d < b2) {      // (false for NaN: it never enters the min / max network below)
    const float t0 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    const float t1 = fmaxf(b1, t0);
    b1 = fminf(b1, t0);
    b2 = fminf(b2, t1);
  }
}

__global__ __launch_bounds__(256) void k_knn_query(GsrKnnTree t, uint32_t nq, const uint32_t* __restrict__ qlist,
                                                   uint32_t first_query, float* __restrict__ out) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t P = t.P;
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const bool active = q < nq;
  const uint32_t pos = active ? (qlist ? qlist[q] : q) : 0u;
  const float4 me = t.pts[pos];          // (pos < P always: P >= 1)
  float b0 = KNN_INF, b1 = KNN_INF, b2 = KNN_INF;
  if (active) {
    const uint32_t j0 = pos >= 3u ? pos - 3u : 0u, j1 = min(P - 1u, pos + 3u);
    for (uint32_t j = j0; j <= j1; j++)
      if (j != pos) knn_insert(knn_point_d2(me, t.pts[j]), b0, b1, b2);
  }
  // an upper bound of the third-nearest distance (inf with fewer than three candidates); the sweep starts from an empty
  // list again, so no candidate is counted twice
  const float bound = b2;
  b0 = b1 = b2 = KNN_INF;
  knn_sweep<256>(
      t, me, active, s_lo, s_hi, [&]() __attribute__((always_inline)) { return fminf(b2, bound); },
      [&](const uint32_t j, const float4 p) __attribute__((always_inline)) {
        if (j != pos) knn_insert(knn_point_d2(me, p), b0, b1, b2);
      });
  if (active) {
    float r;
    if (P >= 4u) r = __fdiv_rn(__fadd_rn(__fadd_rn(b0, b1), b2), 3.0f);
    else if (P == 3u) r = __fmul_rn(__fadd_rn(b0, b1), 0.5f);
    else if (P == 2u) r = b0;
    else r = 0.f;
    out[__float_as_uint(me.w) - first_query] = r;
  }
}

// ---- k = 1 .. 32 ------------------------------------------------------------------------------------------------------------
// one thread per query, as k_knn_query (every row is a query); dist2 [P,k] and / or mean [P] in ORIGINAL row order
template <int K>
__global__ __launch_bounds__(256) void k_knn_query_k(GsrKnnTree t, int k, float* __restrict__ dist2, float* __restrict__ mean) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t P = t.P;
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const bool active = q < P;
  const uint32_t pos = active ? q : 0u;
  const float4 me = t.pts[pos];          // (pos < P always: P >= 1)
  const int pad = K - k;
  float b[K];
  knn_topk_bound<K, 256>(t, me, pos, active, k, KNN_INF, s_lo, s_hi, b);      // (no cut: the whole list is the answer)
  if (!active) return;
  const size_t row = (size_t)__float_as_uint(me.w);
  // a row with a non-finite coordinate has no neighbours: +inf distances, NaN mean (gsr_statistical_outliers drops it on that)
  const bool finite = knn_finite(me.x) && knn_finite(me.y) && knn_finite(me.z);
  if (dist2) {
#pragma unroll
    for (int i = 0; i < K; i++)
      if (i >= pad) dist2[row * (size_t)k + (size_t)(i - pad)] = finite ? b[i] : KNN_INF;
  }
  if (mean) {
    // the square roots summed in ascending order in float64; the divisor counts the point itself at distance 0
    const uint32_t keff = min((uint32_t)k, P - 1u);
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++)
      if (i >= pad && b[i] < KNN_INF) sum += sqrt((double)b[i]);
    mean[row] = finite ? (float)(sum / (double)(keff + 1u)) : __builtin_nanf("");
  }
}

// ---- RGB-D keyframe -> points -------------------------------------------------------------------------------------------------
struct GsrUnprojectArgs {
  int H, W, Hs, Ws, stride;
  float tanfovx, tanfovy, min_depth, max_depth, alpha_below, front_margin;
  float ox, oy;      // principal point, as the projection matrix's offsets P[0,2], P[1,2] (0: the image centre)
};

__device__ __forceinline__ bool unproject_selected(const GsrUnprojectArgs& a, size_t pix, const float* __restrict__ depth,
                                                   const float* __restrict__ alpha, const float* __restrict__ rendered_z,
                                                   float& d) {
  d = depth[pix];
  if (!(knn_finite(d) && d > a.min_depth && d <= a.max_depth)) return false;
  if (!alpha) return true;
  const float A = alpha[pix];
  if (A < a.alpha_below) return true;
  if (!rendered_z) return false;
  // in front of the surface the map renders there (sum w z / A), by more than front_margin x the reading
  const float surface = __fdiv_rn(rendered_z[pix], A);
  return d < __fsub_rn(surface, __fmul_rn(a.front_margin, d));
}

__global__ __launch_bounds__(256) void k_unproject_flag(GsrUnprojectArgs a, const float* __restrict__ depth,
                                                        const float* __restrict__ alpha, const float* __restrict__ rendered_z,
                                                        uint32_t* __restrict__ flags) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= (uint32_t)(a.Ws * a.Hs)) return;
  const int sy = (int)(c / (uint32_t)a.Ws), sx = (int)(c % (uint32_t)a.Ws);
  float d;
  flags[c] = unproject_selected(a, (size_t)(sy * a.stride) * a.W + (size_t)(sx * a.stride), depth, alpha, rendered_z, d) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_unproject_write(GsrUnprojectArgs a, const float* __restrict__ depth,
                                                         const float* __restrict__ color, const float* __restrict__ view,
                                                         const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                                         float* __restrict__ xyz, float* __restrict__ rgb, uint32_t capacity,
                                                         int64_t* __restrict__ count) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = (uint32_t)(a.Ws * a.Hs);
  if (c >= n) return;
  const uint32_t f = flags[c], o = offs[c];
  if (c == n - 1u) *count = (int64_t)o + (int64_t)f;
  if (!f || o >= capacity) return;
  const int py = (int)(c / (uint32_t)a.Ws) * a.stride, px = (int)(c % (uint32_t)a.Ws) * a.stride;
  const size_t pix = (size_t)py * a.W + px;
  const float d = depth[pix];
  // pixel centres at integer coordinates: ndc = (2 p + 1) / S - 1
  const float nx = __fsub_rn(__fdiv_rn((float)(2 * px + 1), (float)a.W), 1.0f);
  const float ny = __fsub_rn(__fdiv_rn((float)(2 * py + 1), (float)a.H), 1.0f);
  // view = W2C^T row-major: view-space v_i = sum_j w_j view[4 j + i] + view[12 + i]; rigid inverse w_j = sum_i view[4 j + i] (v_i - t_i)
  // (nx - 0 is nx, bit for bit: the centred call computes what it always did)
  const float v0 = __fsub_rn(__fmul_rn(__fmul_rn(__fsub_rn(nx, a.ox), a.tanfovx), d), view[12]);
  const float v1 = __fsub_rn(__fmul_rn(__fmul_rn(__fsub_rn(ny, a.oy), a.tanfovy), d), view[13]);
  const float v2 = __fsub_rn(d, view[14]);
#pragma unroll
  for (int j = 0; j < 3; j++)
    xyz[3 * (size_t)o + j] = __builtin_fmaf(view[4 * j + 2], v2, __builtin_fmaf(view[4 * j + 1], v1, __fmul_rn(view[4 * j], v0)));
  const size_t plane = (size_t)a.H * a.W;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) rgb[3 * (size_t)o + ch] = color[ch * plane + pix];
}

// the workspace of gsr_unproject_rgbd, sized for every pixel of the image (stride 1)
struct UnprojectWs {
  uint32_t *flags, *offs, *scan_tmp;
  size_t total;
};
static UnprojectWs unproject_ws(void* base, int32_t W, int32_t H) {
  GsrCarve c(base);
  UnprojectWs w;
  const size_t n = (size_t)(W < 1 ? 1 : W) * (size_t)(H < 1 ? 1 : H);
  w.flags = c.take<uint32_t>(n);
  w.offs = c.take<uint32_t>(n);
  w.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(n));
  w.total = c.o;
  return w;
}

// gsr_unproject_rgbd (ox = oy = 0) and gsr_unproject_rgbd_k: one flag pass, one scan, one write pass
static int unproject_rgbd(const gsr_unproject_params* p, float ox, float oy, const float* depth, const float* color,
                          const float* alpha, const float* rendered_z, float* xyz, float* rgb, int64_t capacity,
                          int64_t* count_dev, void* workspace, size_t workspace_bytes, void* stream) {
  if (!p || !depth || !color || !count_dev || !workspace || capacity < 0 || (capacity > 0 && (!xyz || !rgb)) ||
      p->image_width < 1 || p->image_height < 1 || (int64_t)p->image_width * p->image_height > 0x3FFFFFFF || p->stride < 1 ||
      !p->viewmatrix || !(p->tanfovx > 0.f) || !(p->tanfovy > 0.f) || !(fabsf(ox) <= 1.f) || !(fabsf(oy) <= 1.f)) {
    gsr_set_error("unproject_rgbd: bad arguments");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const UnprojectWs w = unproject_ws(workspace, p->image_width, p->image_height);
  if (!gsr_workspace_fits("unproject_rgbd", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  GsrUnprojectArgs a;
  a.H = p->image_height; a.W = p->image_width; a.stride = p->stride;
  a.Hs = (a.H + a.stride - 1) / a.stride; a.Ws = (a.W + a.stride - 1) / a.stride;
  a.tanfovx = p->tanfovx; a.tanfovy = p->tanfovy; a.min_depth = p->min_depth; a.max_depth = p->max_depth;
  a.alpha_below = p->alpha_below; a.front_margin = p->front_margin;
  a.ox = ox; a.oy = oy;
  const size_t n = (size_t)a.Ws * a.Hs;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((n + 255) / 256);
  GSR_LAUNCH("unproject_flag", k_unproject_flag, dim3(grid), dim3(256), 0, st, a, depth, alpha, rendered_z, w.flags);
  gsr_scan_u32(w.flags, nullptr, w.offs, n, 0, w.scan_tmp, st);
  const uint32_t cap = (uint32_t)(capacity > 0x7FFFFFFF ? 0x7FFFFFFF : capacity);
  GSR_LAUNCH("unproject_write", k_unproject_write, dim3(grid), dim3(256), 0, st, a, depth, color, p->viewmatrix,
             (const uint32_t*)w.flags, (const uint32_t*)w.offs, xyz, rgb, cap, count_dev);
  return gsr_launch_status("unproject_rgbd launch");
}

// bounding box of the finite coordinates -> bbox[6] (min xyz, max xyz; +inf / -inf without a finite value); part: float[1024][6]
void gsr_knn_bbox(int64_t P, const float* points, float* part, float* bbox, hipStream_t st) {
  const uint32_t n = (uint32_t)P, nblk = (n + 255u) / 256u;
  const uint32_t bblk = nblk < (uint32_t)GSR_KNN_BBOX_BLOCKS ? nblk : (uint32_t)GSR_KNN_BBOX_BLOCKS;
  GSR_LAUNCH("knn_bbox_partial", k_knn_bbox_partial, dim3(bblk), dim3(256), 0, st, n, points, part);
  GSR_LAUNCH("knn_bbox_final", k_knn_bbox_final, dim3(1), dim3(256), 0, st, bblk, (const float*)part, bbox);
}

// the structure over a cloud (knn_common.h): what every search starts with
void gsr_knn_build(int64_t P, const float* points, const GsrNnWs& b, hipStream_t st, uint32_t first_query, uint32_t* qflag) {
  const uint32_t n = (uint32_t)P, nblk = (n + 255u) / 256u, nbox = (uint32_t)knn_nbox(n);
  gsr_knn_bbox(P, points, b.bbox_part, b.bbox, st);
  GSR_LAUNCH("knn_morton", k_knn_morton, dim3(nblk), dim3(256), 0, st, n, points, (const float*)b.bbox, b.key[0]);
  const int where = gsr_radix_sort_pairs(b.key[0], b.val[0], b.key[1], b.val[1], true, (size_t)n, 30, b.radix_tmp, st);
  GSR_LAUNCH("knn_boxes", k_knn_boxes, dim3(nblk), dim3(256), 0, st, n, points, (const uint32_t*)b.val[where], b.pts, b.box_lo,
             b.box_hi, first_query, qflag);
  GSR_LAUNCH("knn_supers", k_knn_supers, dim3((nbox + 255u) / 256u), dim3(256), 0, st, nbox, (const float4*)b.box_lo,
             (const float4*)b.box_hi, b.sup_lo, b.sup_hi);
}

// the launches of gsr_knn_k, arguments already checked (also the first stage of gsr_statistical_outliers, csrc/pointcloud.hip)
void gsr_knn_k_launch(int64_t P, const float* points, int k, float* dist2, float* mean, void* workspace, hipStream_t st) {
  const GsrNnWs b = knn_ws(workspace, (size_t)P).nn;
  gsr_knn_build(P, points, b, st);
  const GsrKnnTree t = knn_tree(b, (size_t)P);
  const uint32_t nblk = (t.P + 255u) / 256u;
#define KNN_QUERY_K(K) GSR_LAUNCH("knn_query_k" #K, k_knn_query_k<K>, dim3(nblk), dim3(256), 0, st, t, k, dist2, mean)
  GSR_KNN_PICK_K(k, KNN_QUERY_K);
#undef KNN_QUERY_K
}

extern "C" {

size_t gsr_knn_workspace_bytes(int64_t P) { return knn_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_knn_dist2(int64_t P, const float* points, int64_t first_query, float* mean_dist2, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(P) || !points || !mean_dist2 || !workspace || first_query < 0 || first_query >= P) {
    gsr_set_error("knn_dist2: bad arguments (P = %lld, first_query = %lld)", (long long)P, (long long)first_query);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const KnnWs w = knn_ws(workspace, (size_t)P);
  if (!gsr_workspace_fits("knn_dist2", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n = (uint32_t)P, nblk = (n + 255u) / 256u;
  const bool subset = first_query > 0;

  gsr_knn_build(P, points, w.nn, st, (uint32_t)first_query, subset ? w.qflag : nullptr);
  const uint32_t nq = (uint32_t)(P - first_query);
  if (subset) {
    gsr_scan_u32(w.qflag, nullptr, w.qpos, (size_t)n, 0, w.scan_tmp, st);
    GSR_LAUNCH("knn_compact", k_knn_compact, dim3(nblk), dim3(256), 0, st, n, (const uint32_t*)w.qflag, (const uint32_t*)w.qpos,
               w.qlist);
  }
  GSR_LAUNCH("knn_query", k_knn_query, dim3((nq + 255u) / 256u), dim3(256), 0, st, knn_tree(w.nn, (size_t)P), nq,
             subset ? (const uint32_t*)w.qlist : (const uint32_t*)nullptr, (uint32_t)first_query, mean_dist2);
  return gsr_launch_status("knn_dist2 launch");
}

size_t gsr_knn_k_workspace_bytes(int64_t P) { return knn_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_knn_k(int64_t P, const float* points, int32_t k, float* dist2_out, float* mean_dist_out, void* workspace,
              size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(P) || !points || !workspace || k < 1 || k > GSR_KNN_K_MAX || (!dist2_out && !mean_dist_out)) {
    gsr_set_error("knn_k: bad arguments (P = %lld, k = %d: expected 1 .. %d and at least one output)", (long long)P, (int)k,
                  GSR_KNN_K_MAX);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!gsr_workspace_fits("knn_k", workspace, workspace_bytes, knn_ws(nullptr, (size_t)P).total)) return GSR_ERR_STATE_TOO_SMALL;
  gsr_knn_k_launch(P, points, (int)k, dist2_out, mean_dist_out, workspace, (hipStream_t)stream);
  return gsr_launch_status("knn_k launch");
}

size_t gsr_unproject_workspace_bytes(int32_t W, int32_t H) { return unproject_ws(nullptr, W, H).total; }

int gsr_unproject_rgbd(const gsr_unproject_params* p, const float* depth, const float* color, const float* alpha,
                       const float* rendered_z, float* xyz, float* rgb, int64_t capacity, int64_t* count_dev, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return unproject_rgbd(p, 0.f, 0.f, depth, color, alpha, rendered_z, xyz, rgb, capacity, count_dev, workspace, workspace_bytes,
                        stream);
}

int gsr_unproject_rgbd_k(const gsr_unproject_params_k* p, const float* depth, const float* color, const float* alpha,
                         const float* rendered_z, float* xyz, float* rgb, int64_t capacity, int64_t* count_dev, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return unproject_rgbd(p ? &p->base : nullptr, p ? p->ox : 0.f, p ? p->oy : 0.f, depth, color, alpha, rendered_z, xyz, rgb,
                        capacity, count_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
