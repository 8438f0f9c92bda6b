// registration.hip - rigid registration of one point cloud to another: what the reference does with Open3D's point-to-point ICP
// (convert_visual_merged_msg.py:187-249 pointcloud_registeration, :393-432 pointcloud_registration_gpu) before it merges a
// message's cloud into the accumulated one.
//
// gsr_nn_index_build: the structure of knn.hip (knn_common.h: bounding box, 30-bit Morton sort, 64-point boxes, 64-box
//   super-boxes) over the TARGET, once per registration - the target does not move between iterations.  The blob keeps the sorted
//   float4 points (xyz, bits of the original row), both levels of AABBs and the bounding box; the sort's scratch lies behind them
//   in the same blob.  A row with a non-finite coordinate is stored as NaN NaN NaN: every distance to it is NaN, which fails every
//   comparison - it is nobody's neighbour.
//
// gsr_nn_search: one thread per source row, knn_sweep of knn_common.h (super-box AABBs staged through LDS 256 at a time,
//   descent where the AABB distance does not exceed the bound) with the best distance so far as the radius.  The query is q =
//   (float)(R s + t), formed by reg_apply below: float64, every operation rounded separately, one fixed order, rounded to
//   float32 once per component - numpy float64 gives the same bits.  The answer is the lexicographic minimum of (float32 d2,
//   original target row) over the finite target rows with d2 <= max_dist2: a multiset minimum, so neither distance nor row
//   depend on the traversal, the order of the source rows or the `order` permutation.  A box is entered when its AABB distance
//   is <= the bound (not <): a tie with a smaller row is never lost.
//
// gsr_icp_update: correspondences -> the next transform, nothing on the host.  A first kernel takes the target point of the
//   first valid row as the shift every sum is formed about (a cloud at +1000 loses nothing); <= 256 workgroups then sum, over
//   fixed slices, n, |q - p|^2, q, p and q p^T in float64 (gsr_block_sum, gsr_common.h: a fixed order, no float atomics); one
//   workgroup adds the partials and one thread solves Horn's closed form: the rotation is the eigenvector of the largest
//   eigenvalue of the symmetric 4 x 4 matrix built from the centred cross-covariance - a unit quaternion, so a reflection
//   cannot come out - found by cyclic Jacobi with a fixed number of sweeps (horn_common.h, shared with features.hip).  T <- dT
//   T.
//
// gsr_icp_update_plane / gsr_icp_update_colored: the same shift and summation structure over the point-to-plane residual - and,
//   for the coloured update, the photometric residual in the target's tangent plane beside it (the gradient of colored.hip) -
//   then the final kernel all 6-unknown updates share (k_gn6_final, solve6_common.h: the rows of partial sums, the stats, the
//   n < 6 rule, one 6 x 6 LDL^T solve and dT = Tr(c) [Rz Ry Rx, t] Tr(-c)).  The three entries share their host prelude too
//   (icp_begin: the workspace check, the shift launch).
#include "knn_common.h"
#include "horn_common.h"
#include "rigid_common.h"
#include "solve6_common.h"
#include "icp_common.h"

#define GSR_ICP_SUMS 17                                  // n, sum d2, q[3], p[3], q p^T [9]
#define GSR_ICP_PLANE_H 3                                // n, sum d2, sum r^2
#define GSR_ICP_COLORED_H 4                              // n, sum d2, sum r_G^2, sum r_I^2 (both unweighted)
#define GSR_ICP_PLANE_SUMS (GSR_ICP_PLANE_H + GSR_GN6_TERMS)          // ... J^T r [6], upper triangle of J^T J [21]
#define GSR_ICP_COLORED_SUMS (GSR_ICP_COLORED_H + GSR_GN6_TERMS)

// (the index blob: GsrNnWs / nn_ws of knn_common.h - normals.hip's workspace is the same blob)

// workspace of gsr_nn_query_order: codes / rows ping-pong and the sort's scratch
struct NnOrderWs {
  uint32_t *key[2], *val[2], *radix_tmp;
  size_t total;
};
static NnOrderWs nn_order_ws(void* base, size_t P) {
  GsrCarve c(base);
  NnOrderWs w;
  if (P == 0) P = 1;
  for (int i = 0; i < 2; i++) w.key[i] = c.take<uint32_t>(P);
  for (int i = 0; i < 2; i++) w.val[i] = c.take<uint32_t>(P);
  w.radix_tmp = c.take<uint32_t>(gsr_radix_tmp_elems(P));
  w.total = c.o;
  return w;
}

// workspace of gsr_icp_update and gsr_icp_update_plane: gn_ws(.., GSR_ICP_PLANE_SUMS, true) (solve6_common.h; the point-to-point
// update uses GSR_ICP_SUMS of each row's); of gsr_icp_update_colored: gn_ws(.., GSR_ICP_COLORED_SUMS, true), a size of its own

// ---- q = (float)(R s + t): RegT, reg_load, reg_apply (rigid_common.h, shared with pointcloud2.hip) -----------------------------

// ---- index ----------------------------------------------------------------------------------------------------------------------
// rows with a non-finite coordinate become NaN NaN NaN; thread 0 also leaves the box centre (0 where the box is empty)
__global__ __launch_bounds__(256) void k_nn_finish_index(uint32_t P, float4* __restrict__ pts, float* __restrict__ bbox) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j == 0u) {
    double* c = (double*)(bbox + 16);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double m = 0.5 * ((double)bbox[a] + (double)bbox[3 + a]);
      c[a] = fabs(m) < (double)KNN_INF ? m : 0.0;
    }
  }
  if (j >= P) return;
  pts[j] = knn_mask_non_finite(pts[j]);
}

// Morton code, in the target's box, of every transformed source row (the key of the `order` permutation)
__global__ __launch_bounds__(256) void k_nn_query_codes(uint32_t Ps, const float* __restrict__ src, const double* __restrict__ T_dev,
                                                        const float* __restrict__ bbox, uint32_t* __restrict__ codes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= Ps) return;
  const RegT T = reg_load(T_dev);
  const float4 q = reg_apply(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
  codes[i] = knn_morton_code(q.x, q.y, q.z, bbox);
}

__global__ __launch_bounds__(256) void k_nn_transform(uint32_t P, const float* __restrict__ src, const double* __restrict__ T_dev,
                                                      float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  const RegT T = reg_load(T_dev);
  const float4 q = reg_apply(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
  out[3 * (size_t)i] = q.x;
  out[3 * (size_t)i + 1] = q.y;
  out[3 * (size_t)i + 2] = q.z;
}

// (d2, row) < (bd, br) lexicographically; false for a NaN d2.  (Two selects, no branch: the inner loop of the search)
__device__ __forceinline__ void nn_take(float d2, uint32_t row, float& bd, uint32_t& br) {
  const bool take = (d2 < bd) | ((d2 == bd) & (row < br));
  bd = take ? d2 : bd;
  br = take ? row : br;
}

__global__ __launch_bounds__(256) void k_nn_search(GsrKnnTree t, uint32_t Ps, const float* __restrict__ src,
                                                   const uint32_t* __restrict__ order, const double* __restrict__ T_dev,
                                                   float max_dist2, int32_t* __restrict__ idx_out,
                                                   float* __restrict__ dist2_out) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t row = i < Ps ? (order ? order[i] : i) : 0u;
  // (an `order` entry outside the cloud is not followed: that thread answers nothing)
  const bool active = i < Ps && row < Ps;
  if (!active) row = 0u;
  const RegT T = reg_load(T_dev);
  const float4 me = reg_apply(T, src[3 * (size_t)row], src[3 * (size_t)row + 1], src[3 * (size_t)row + 2]);
  const bool finite = knn_finite(me.x) && knn_finite(me.y) && knn_finite(me.z);
  // the bound starts at max_dist2 with no row: a candidate AT max_dist2 is taken (valid iff d2 <= max_dist2), one beyond never
  float bd = max_dist2;
  uint32_t br = GSR_NONE;
  knn_sweep<256>(
      t, me, active && finite, s_lo, s_hi, [&]() __attribute__((always_inline)) { return bd; },
      [&](const uint32_t, const float4 p) __attribute__((always_inline)) {
        nn_take(knn_point_d2(me, p), __float_as_uint(p.w), bd, br);
      });
  if (!active) return;
  const bool valid = br != GSR_NONE;
  idx_out[row] = valid ? (int32_t)br : -1;
  if (dist2_out) dist2_out[row] = valid ? bd : KNN_INF;
}

// ---- one ICP update ---------------------------------------------------------------------------------------------------------------
// (icp_pair, k_icp_shift: icp_common.h, shared with gicp.hip)

__global__ __launch_bounds__(256) void k_icp_partial(uint32_t Ps, const float* __restrict__ src, uint32_t Pt,
                                                     const float* __restrict__ tgt, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ T_dev, const double* __restrict__ shift,
                                                     double* __restrict__ part) {
  const RegT T = reg_load(T_dev);
  const double c0 = shift[0], c1 = shift[1], c2 = shift[2];
  double s[GSR_ICP_SUMS];
#pragma unroll
  for (int a = 0; a < GSR_ICP_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < Ps; i += gridDim.x * 256u) {
    float4 qf, pf;
    if (!icp_pair(i, src, Pt, tgt, idx, T, qf, pf)) continue;
    // (float32 values: the differences below are exact in float64)
    const double q[3] = {(double)qf.x - c0, (double)qf.y - c1, (double)qf.z - c2};
    const double p[3] = {(double)pf.x - c0, (double)pf.y - c1, (double)pf.z - c2};
    const double ex = (double)qf.x - (double)pf.x, ey = (double)qf.y - (double)pf.y, ez = (double)qf.z - (double)pf.z;
    s[0] += 1.0;
    s[1] += (ex * ex + ey * ey) + ez * ez;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      s[2 + a] += q[a];
      s[5 + a] += p[a];
#pragma unroll
      for (int b = 0; b < 3; b++) s[8 + 3 * a + b] += q[a] * p[b];
    }
  }
  gsr_block_sum_store(s, part);
}

// one workgroup: the partials, then thread 0 solves and composes
__global__ __launch_bounds__(256) void k_icp_final(uint32_t nblk, uint32_t Ps, const double* __restrict__ part,
                                                   const double* __restrict__ shift, double* __restrict__ T_dev,
                                                   double* __restrict__ stats) {
  __shared__ double A[4][4], V[4][4];      // thread 0 only: indexed at run time, which registers cannot be
  double s[GSR_ICP_SUMS];
  gsr_block_sum_rows(s, part, nblk);
  if (threadIdx.x != 0) return;
  gn_stats_header<2>(s, (double)Ps, stats);      // (n, sum d2)
  const double n = s[0];
  if (n < 3.0) {
    stats[3] = 1.0;      // too few correspondences: T stays
    return;
  }
  // centred cross-covariance M[a][b] = sum (q_a - qbar_a)(p_b - pbar_b), about the shift
  double qb[3], pb[3], M[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    qb[a] = s[2 + a] / n;
    pb[a] = s[5 + a] / n;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) M[a][b] = s[8 + 3 * a + b] - s[2 + a] * pb[b];
  }
  double R[3][3];
  if (!horn_rotation(M, HornMat4{A}, HornMat4{V}, R, stats[5])) {      // (horn_common.h)
    stats[3] = 2.0;
    return;
  }
  // dT x = R (x - (c + qbar)) + (c + pbar)
  double td[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double cq0 = shift[0] + qb[0], cq1 = shift[1] + qb[1], cq2 = shift[2] + qb[2];
    td[a] = (shift[a] + pb[a]) - ((R[a][0] * cq0 + R[a][1] * cq1) + R[a][2] * cq2);
  }
  // T <- dT T
  double Tn[12];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 4; b++)
      Tn[4 * a + b] = ((R[a][0] * T_dev[b] + R[a][1] * T_dev[4 + b]) + R[a][2] * T_dev[8 + b]) + (b == 3 ? td[a] : 0.0);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) T_dev[i] = Tn[i];
  T_dev[12] = T_dev[13] = T_dev[14] = 0.0;
  T_dev[15] = 1.0;
  stats[3] = 0.0;
}

// ---- one point-to-plane update ------------------------------------------------------------------------------------------------------
// per workgroup: s[0] = n, s[1] = sum |q - p|^2, s[2] = sum r^2, s[3..8] = J^T r, s[9..29] = J^T J rows 0 .. 5 from the diagonal on
__global__ __launch_bounds__(256) void k_icp_plane_partial(uint32_t Ps, const float* __restrict__ src, uint32_t Pt,
                                                           const float* __restrict__ tgt, const float* __restrict__ nrm,
                                                           const int32_t* __restrict__ idx, const double* __restrict__ T_dev,
                                                           const double* __restrict__ shift, double* __restrict__ part) {
  const RegT T = reg_load(T_dev);
  const double c0 = shift[0], c1 = shift[1], c2 = shift[2];
  double s[GSR_ICP_PLANE_SUMS];
#pragma unroll
  for (int a = 0; a < GSR_ICP_PLANE_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < Ps; i += gridDim.x * 256u) {
    float4 qf, pf;
    if (!icp_pair(i, src, Pt, tgt, idx, T, qf, pf)) continue;
    const size_t k = (size_t)idx[i];
    const float n0 = nrm[3 * k], n1 = nrm[3 * k + 1], n2 = nrm[3 * k + 2];
    if (!(knn_finite(n0) && knn_finite(n1) && knn_finite(n2))) continue;
    // (float32 values: the differences below are exact in float64)
    const double q[3] = {(double)qf.x - c0, (double)qf.y - c1, (double)qf.z - c2};
    const double e[3] = {(double)qf.x - (double)pf.x, (double)qf.y - (double)pf.y, (double)qf.z - (double)pf.z};
    const double n[3] = {(double)n0, (double)n1, (double)n2};
    const double res = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2];
    const double J[6] = {q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]};
    s[0] += 1.0;
    s[1] += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    s[2] += res * res;
    int o = 9;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      s[3 + a] += J[a] * res;
#pragma unroll
      for (int b = a; b < 6; b++) s[o++] += J[a] * J[b];
    }
  }
  gsr_block_sum_store(s, part);
}

// (the final kernel shared by the plane update, the coloured one and odometry.hip: k_gn6_final, solve6_common.h)

// ---- one coloured update (Park, Zhou, Koltun 2017; Open3D's TransformationEstimationForColoredICP) -------------------------------------
// I = (r + g + b) / 3 in float64, left to right (colored.hip forms the target's gradient from the same value)
__device__ __forceinline__ double icp_intensity(const float* __restrict__ colors, size_t row) {
  return (((double)colors[3 * row] + (double)colors[3 * row + 1]) + (double)colors[3 * row + 2]) / 3.0;
}

// per workgroup: s[0] = n, s[1] = sum |q - p|^2, s[2] = sum ((q - p).n)^2 (0 with lambda = 0), s[3] = sum (I_s - I_proj)^2 (0 with
// lambda = 1), s[4..9] = J^T r, s[10..30] = J^T J rows 0 .. 5 from the diagonal on, r and J over both residuals
__global__ __launch_bounds__(256) void k_icp_colored_partial(uint32_t Ps, const float* __restrict__ src,
                                                             const float* __restrict__ scol, uint32_t Pt,
                                                             const float* __restrict__ tgt, const float* __restrict__ nrm,
                                                             const float* __restrict__ tcol, const float* __restrict__ grad,
                                                             const int32_t* __restrict__ idx, double sqrt_g, double sqrt_i,
                                                             const double* __restrict__ T_dev, const double* __restrict__ shift,
                                                             double* __restrict__ part) {
  const RegT T = reg_load(T_dev);
  const double c0 = shift[0], c1 = shift[1], c2 = shift[2];
  double s[GSR_ICP_COLORED_SUMS];
#pragma unroll
  for (int a = 0; a < GSR_ICP_COLORED_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < Ps; i += gridDim.x * 256u) {
    float4 qf, pf;
    if (!icp_pair(i, src, Pt, tgt, idx, T, qf, pf)) continue;
    const size_t k = (size_t)idx[i];
    const float n0 = nrm[3 * k], n1 = nrm[3 * k + 1], n2 = nrm[3 * k + 2];
    const float g0 = grad[3 * k], g1 = grad[3 * k + 1], g2 = grad[3 * k + 2];
    const double is = icp_intensity(scol, (size_t)i), it = icp_intensity(tcol, k);
    if (!(knn_finite(n0) && knn_finite(n1) && knn_finite(n2) && knn_finite(g0) && knn_finite(g1) && knn_finite(g2) &&
          fabs(is) < (double)KNN_INF && fabs(it) < (double)KNN_INF))
      continue;
    // (float32 values: the differences below are exact in float64)
    const double q[3] = {(double)qf.x - c0, (double)qf.y - c1, (double)qf.z - c2};
    const double e[3] = {(double)qf.x - (double)pf.x, (double)qf.y - (double)pf.y, (double)qf.z - (double)pf.z};
    const double n[3] = {(double)n0, (double)n1, (double)n2};
    const double d[3] = {(double)g0, (double)g1, (double)g2};
    const double en = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2];
    const double dn = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    // q_proj - p = e - (e.n) n;  I_proj = I_t + d.(q_proj - p);  m = -(I - n n^T) d
    const double w[3] = {e[0] - en * n[0], e[1] - en * n[1], e[2] - en * n[2]};
    const double ri = is - (it + ((d[0] * w[0] + d[1] * w[1]) + d[2] * w[2]));
    const double m[3] = {dn * n[0] - d[0], dn * n[1] - d[1], dn * n[2] - d[2]};
    const double rg = sqrt_g * en, rp = sqrt_i * ri;
    const double JG[6] = {sqrt_g * (q[1] * n[2] - q[2] * n[1]), sqrt_g * (q[2] * n[0] - q[0] * n[2]),
                          sqrt_g * (q[0] * n[1] - q[1] * n[0]), sqrt_g * n[0], sqrt_g * n[1], sqrt_g * n[2]};
    const double JI[6] = {sqrt_i * (q[1] * m[2] - q[2] * m[1]), sqrt_i * (q[2] * m[0] - q[0] * m[2]),
                          sqrt_i * (q[0] * m[1] - q[1] * m[0]), sqrt_i * m[0], sqrt_i * m[1], sqrt_i * m[2]};
    s[0] += 1.0;
    s[1] += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    s[2] += sqrt_g > 0.0 ? en * en : 0.0;
    s[3] += sqrt_i > 0.0 ? ri * ri : 0.0;
    int o = 10;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      s[4 + a] += JG[a] * rg + JI[a] * rp;
#pragma unroll
      for (int b = a; b < 6; b++) s[o++] += JG[a] * JG[b] + JI[a] * JI[b];
    }
  }
  gsr_block_sum_store(s, part);
}

// ---- host: what the update entries do alike: IcpRun, icp_begin (icp_common.h, shared with gicp.hip) ----

extern "C" {

size_t gsr_nn_index_bytes(int64_t Pt) { return nn_ws(nullptr, (size_t)(Pt < 1 ? 1 : Pt)).total; }

int gsr_nn_index_build(int64_t Pt, const float* target, void* index, size_t index_bytes, void* stream) {
  if (gsr_bad_size(Pt) || !target || !index) {
    gsr_set_error("nn_index_build: bad arguments (Pt = %lld)", (long long)Pt);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrNnBlob w = nn_ws(index, (size_t)Pt);
  if (!gsr_workspace_fits("nn_index_build", index, index_bytes, w.total, "index")) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const GsrNnWs& b = w.nn;
  gsr_knn_build(Pt, target, b, st);
  const uint32_t n = (uint32_t)Pt;
  GSR_LAUNCH("nn_finish_index", k_nn_finish_index, dim3((n + 255u) / 256u), dim3(256), 0, st, n, b.pts, b.bbox);
  return gsr_launch_status("nn_index_build launch");
}

size_t gsr_nn_order_workspace_bytes(int64_t Ps) { return nn_order_ws(nullptr, (size_t)(Ps < 1 ? 1 : Ps)).total; }

int gsr_nn_query_order(int64_t Pt, const void* index, int64_t Ps, const float* source, const double* T_dev, int32_t* order_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Pt) || gsr_bad_size(Ps) || !index || !source || !order_out || !workspace) {
    gsr_set_error("nn_query_order: bad arguments (Pt = %lld, Ps = %lld)", (long long)Pt, (long long)Ps);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const NnOrderWs w = nn_order_ws(workspace, (size_t)Ps);
  if (!gsr_workspace_fits("nn_query_order", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n = (uint32_t)Ps;
  const float* bbox = nn_ws(index, (size_t)Pt).nn.bbox;
  GSR_LAUNCH("nn_query_codes", k_nn_query_codes, dim3((n + 255u) / 256u), dim3(256), 0, st, n, source, T_dev, bbox, w.key[0]);
  const int where = gsr_radix_sort_pairs(w.key[0], w.val[0], w.key[1], w.val[1], true, (size_t)n, 30, w.radix_tmp, st);
  (void)hipMemcpyAsync(order_out, w.val[where], (size_t)n * 4, hipMemcpyDeviceToDevice, st);
  return gsr_launch_status("nn_query_order launch");
}

int gsr_nn_search(int64_t Pt, const void* index, int64_t Ps, const float* source, const double* T_dev, float max_dist2,
                  const int32_t* order, int32_t* idx_out, float* dist2_out, void* stream) {
  if (gsr_bad_size(Pt) || gsr_bad_size(Ps) || !index || !source || !idx_out || !(max_dist2 >= 0.f)) {
    gsr_set_error("nn_search: bad arguments (Pt = %lld, Ps = %lld, max_dist2 = %g)", (long long)Pt, (long long)Ps,
                  (double)max_dist2);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrKnnTree t = knn_tree(nn_ws(index, (size_t)Pt).nn, (size_t)Pt);
  const uint32_t ns = (uint32_t)Ps;
  GSR_LAUNCH("nn_search", k_nn_search, dim3((ns + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, t, ns, source,
             (const uint32_t*)order, T_dev, max_dist2, idx_out, dist2_out);
  return gsr_launch_status("nn_search launch");
}

int gsr_transform_points(int64_t P, const float* points, const double* T_dev, float* out, void* stream) {
  if (gsr_bad_size(P) || !points || !out) {
    gsr_set_error("transform_points: bad arguments (P = %lld)", (long long)P);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const uint32_t n = (uint32_t)P;
  GSR_LAUNCH("nn_transform", k_nn_transform, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, points, T_dev, out);
  return gsr_launch_status("transform_points launch");
}

size_t gsr_icp_workspace_bytes(int64_t Ps) {
  (void)Ps;      // (the partial sums of at most GSR_GN_BLOCKS workgroups: the size does not grow with the cloud)
  return gn_ws(nullptr, GSR_ICP_PLANE_SUMS, true).total;
}

int gsr_icp_update(int64_t Ps, const float* source, int64_t Pt, const float* target, const int32_t* idx, double* T_dev,
                   double* stats_dev, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Ps) || gsr_bad_size(Pt) || !source || !target || !idx || !T_dev || !stats_dev || !workspace) {
    gsr_set_error("icp_update: bad arguments (Ps = %lld, Pt = %lld)", (long long)Ps, (long long)Pt);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  IcpRun r;
  if (const int rc = icp_begin("icp_update", GSR_ICP_PLANE_SUMS, Ps, source, Pt, target, idx, T_dev, workspace, workspace_bytes,
                               stream, r))
    return rc;
  GSR_LAUNCH("icp_partial", k_icp_partial, dim3(r.sblk), dim3(256), 0, r.st, r.ns, source, r.nt, target, idx, (const double*)T_dev,
             (const double*)r.shift, r.part);
  GSR_LAUNCH("icp_final", k_icp_final, dim3(1), dim3(256), 0, r.st, r.sblk, r.ns, (const double*)r.part, (const double*)r.shift,
             T_dev, stats_dev);
  return gsr_launch_status("icp_update launch");
}

int gsr_icp_update_plane(int64_t Ps, const float* source, int64_t Pt, const float* target, const float* target_normals,
                         const int32_t* idx, double* T_dev, double* stats_dev, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (gsr_bad_size(Ps) || gsr_bad_size(Pt) || !source || !target || !target_normals || !idx || !T_dev || !stats_dev ||
      !workspace) {
    gsr_set_error("icp_update_plane: bad arguments (Ps = %lld, Pt = %lld)", (long long)Ps, (long long)Pt);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  IcpRun r;
  if (const int rc = icp_begin("icp_update_plane", GSR_ICP_PLANE_SUMS, Ps, source, Pt, target, idx, T_dev, workspace,
                               workspace_bytes, stream, r))
    return rc;
  GSR_LAUNCH("icp_plane_partial", k_icp_plane_partial, dim3(r.sblk), dim3(256), 0, r.st, r.ns, source, r.nt, target, target_normals,
             idx, (const double*)T_dev, (const double*)r.shift, r.part);
  GSR_LAUNCH("icp_plane_final", k_gn6_final<GSR_ICP_PLANE_H>, dim3(1), dim3(256), 0, r.st, r.sblk, (double)r.ns, 1,
             (const double*)r.part, (const double*)r.shift, T_dev, stats_dev);
  return gsr_launch_status("icp_update_plane launch");
}

size_t gsr_icp_colored_workspace_bytes(int64_t Ps) {
  (void)Ps;      // (as gsr_icp_workspace_bytes: at most GSR_GN_BLOCKS rows of partial sums)
  return gn_ws(nullptr, GSR_ICP_COLORED_SUMS, true).total;
}

int gsr_icp_update_colored(int64_t Ps, const float* source, const float* source_colors, int64_t Pt, const float* target,
                           const float* target_normals, const float* target_colors, const float* target_gradient,
                           const int32_t* idx, double lambda_geometric, double* T_dev, double* stats_dev, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Ps) || gsr_bad_size(Pt) || !source || !source_colors || !target || !target_normals || !target_colors ||
      !target_gradient || !idx || !T_dev || !stats_dev || !workspace || !(lambda_geometric >= 0.0 && lambda_geometric <= 1.0)) {
    gsr_set_error("icp_update_colored: bad arguments (Ps = %lld, Pt = %lld, lambda_geometric = %g: expected 0 .. 1)",
                  (long long)Ps, (long long)Pt, lambda_geometric);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  IcpRun r;
  if (const int rc = icp_begin("icp_update_colored", GSR_ICP_COLORED_SUMS, Ps, source, Pt, target, idx, T_dev, workspace,
                               workspace_bytes, stream, r))
    return rc;
  const double sqrt_g = sqrt(lambda_geometric), sqrt_i = sqrt(1.0 - lambda_geometric);
  GSR_LAUNCH("icp_colored_partial", k_icp_colored_partial, dim3(r.sblk), dim3(256), 0, r.st, r.ns, source, source_colors, r.nt,
             target, target_normals, target_colors, target_gradient, idx, sqrt_g, sqrt_i, (const double*)T_dev,
             (const double*)r.shift, r.part);
  GSR_LAUNCH("icp_colored_final", k_gn6_final<GSR_ICP_COLORED_H>, dim3(1), dim3(256), 0, r.st, r.sblk, (double)r.ns, 1,
             (const double*)r.part, (const double*)r.shift, T_dev, stats_dev);
  return gsr_launch_status("icp_update_colored launch");
}

}  // extern "C"
