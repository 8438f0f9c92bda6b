// normals.hip - surface normals of a point cloud: what the reference takes from Open3D's
// estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (convert_visual_merged_msg.py:181, :193-196, :348) - the input of a
// point-to-plane registration (csrc/registration.hip, gsr_icp_update_plane).
//
// gsr_estimate_normals: the structure of knn.hip (knn_common.h) over the cloud, rows with a non-finite coordinate turned into
//   NaN NaN NaN (every distance to them is NaN and fails every comparison: nobody's neighbour), then ONE launch, one thread per
//   query in Morton order, two sweeps (knn_sweep, knn_common.h) over the same boxes and one LDS allocation:
//   1. the bound.  k = max_nn - 1 (max_nn counts the point itself).  knn_topk_bound, cut at r2, gives min(r2, d_k), d_k the k-th
//      smallest d2 to the other finite rows (+inf with fewer than k).
//   2. the sums.  bound = min(r2, d_k) is now a FIXED pruning radius (it prunes from the first box).  knn_member_walk: every
//      row j != i with d2(i,j) <= bound is a member - rows tied at the bound all are, so no row tie-break is needed and no
//      neighbour index is ever stored.  delta = p_j - p_i per component in float32 (__fsub_rn), promoted; S1 = sum delta and S2
//      = sum delta delta^T (six values) in float64, in sorted-position order: fixed for a given input, so two runs give the
//      same bits.  The point itself contributes delta = 0 and counts: n = 1 + members.
//   Then C = S2 / n - (S1 / n)(S1 / n)^T and cyclic Jacobi on the symmetric 3 x 3 in float64, a fixed number of sweeps, every
//   index a compile-time constant (registers, no scratch); eigenvalues ascending; the normal is the eigenvector of the smallest,
//   normalised again in float64 and rounded to float32 once.  Sign: towards the viewpoint (n.(v - p) >= 0), or without one the
//   component of largest magnitude positive.  n < 3: (0, 0, 1) and zero eigenvalues, whatever the viewpoint.  A non-finite row:
//   NaN normal and eigenvalues, count 0.
//   The top-K registers of sweep 1 are dead in sweep 2, where the nine float64 sums live: one launch holds both.
#include "knn_common.h"
#include "jacobi3_common.h"      // normals_rotate, GSR_NORMALS_SWEEPS (shared with gicp.hip)

// rows with a non-finite coordinate become NaN NaN NaN (.w, the original row, stays)
__global__ __launch_bounds__(256) void k_normals_mask(uint32_t P, float4* __restrict__ pts) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P) return;
  pts[j] = knn_mask_non_finite(pts[j]);
}

struct GsrNormalsView {
  float x, y, z;
  int32_t on;
};

template <int K>
__global__ __launch_bounds__(256) void k_normals(GsrKnnTree t, int k, float r2, GsrNormalsView view, float* __restrict__ normals,
                                                 int32_t* __restrict__ count_out, float* __restrict__ eig_out) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const bool active = q < t.P;
  const uint32_t pos = active ? q : 0u;
  const float4 me = t.pts[pos];          // (pos < P always: P >= 1)
  // ---- sweep 1: min(r2, d_k) ----
  float bound;
  {
    float b[K];
    bound = knn_topk_bound<K, 256>(t, me, pos, active, k, r2, s_lo, s_hi, b);
  }
  // ---- sweep 2: the sums over { j != i : d2 <= bound } ----
  double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  uint32_t members = 0u;
  knn_member_walk<256>(t, me, pos, active, bound, s_lo, s_hi,
                       [&](const uint32_t, const float fx, const float fy, const float fz) __attribute__((always_inline)) {
                         // delta = p_j - p_i = -(p_i - p_j), exactly
                         const double dx = -(double)fx, dy = -(double)fy, dz = -(double)fz;
                         members++;
                         s1x += dx; s1y += dy; s1z += dz;
                         sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                         syy += dy * dy; syz += dy * dz; szz += dz * dz;
                       });
  if (!active) return;
  const size_t row = (size_t)__float_as_uint(me.w);
  const bool finite = knn_finite(me.x) && knn_finite(me.y) && knn_finite(me.z);
  const uint32_t count = finite ? members + 1u : 0u;
  if (count_out) count_out[row] = (int32_t)count;
  float nx = 0.f, ny = 0.f, nz = 1.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
  if (!finite) {
    nx = ny = nz = e0 = e1 = e2 = __builtin_nanf("");
  } else if (count >= 3u) {
    const double n = (double)count;
    const double mx = s1x / n, my = s1y / n, mz = s1z / n;
    double a00 = sxx / n - mx * mx, a01 = sxy / n - mx * my, a02 = sxz / n - mx * mz;
    double a11 = syy / n - my * my, a12 = syz / n - my * mz, a22 = szz / n - mz * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < GSR_NORMALS_SWEEPS; sweep++) {
      normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), third index 2
      normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), third index 1
      normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), third index 0
    }
    // the column of the smallest diagonal entry (the first on ties), and the three values in ascending order
    const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
    double wx = c0 ? v00 : (c1 ? v01 : v02), wy = c0 ? v10 : (c1 ? v11 : v12), wz = c0 ? v20 : (c1 ? v21 : v22);
    const double lo = fmin(a00, fmin(a11, a22)), hi = fmax(a00, fmax(a11, a22));
    const double mid = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
    const double norm = sqrt((wx * wx + wy * wy) + wz * wz);
    wx /= norm; wy /= norm; wz /= norm;
    nx = (float)wx; ny = (float)wy; nz = (float)wz;
    e0 = (float)lo; e1 = (float)mid; e2 = (float)hi;
    bool flip;
    if (view.on) {
      const double d = (wx * ((double)view.x - (double)me.x) + wy * ((double)view.y - (double)me.y)) +
                       wz * ((double)view.z - (double)me.z);
      flip = d < 0.0;
    } else {
      const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
      const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
      flip = lead < 0.f;
    }
    if (flip) {
      nx = -nx; ny = -ny; nz = -nz;
    }
  }
  normals[3 * row] = nx;
  normals[3 * row + 1] = ny;
  normals[3 * row + 2] = nz;
  if (eig_out) {
    eig_out[3 * row] = e0;
    eig_out[3 * row + 1] = e1;
    eig_out[3 * row + 2] = e2;
  }
}

extern "C" {

size_t gsr_normals_workspace_bytes(int64_t P) { return nn_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_estimate_normals(int64_t P, const float* points, float radius, int32_t max_nn, const float* viewpoint, float* normals,
                         int32_t* count_out, float* eigenvalues_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(P) || !points || !normals || !workspace || max_nn < 3 || max_nn > GSR_KNN_K_MAX + 1 ||
      !(radius > 0.f) ||
      (viewpoint && !(fabsf(viewpoint[0]) < KNN_INF && fabsf(viewpoint[1]) < KNN_INF && fabsf(viewpoint[2]) < KNN_INF))) {
    gsr_set_error("estimate_normals: bad arguments (P = %lld, radius = %g: expected > 0, max_nn = %d: expected 3 .. %d, a finite "
                  "viewpoint or none)", (long long)P, (double)radius, (int)max_nn, GSR_KNN_K_MAX + 1);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrNnBlob w = nn_ws(workspace, (size_t)P);      // (the blob of a target index: knn_common.h)
  if (!gsr_workspace_fits("estimate_normals", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const GsrNnWs& b = w.nn;
  gsr_knn_build(P, points, b, st);
  const GsrKnnTree t = knn_tree(b, (size_t)P);
  const uint32_t nblk = (t.P + 255u) / 256u;
  GSR_LAUNCH("normals_mask", k_normals_mask, dim3(nblk), dim3(256), 0, st, t.P, b.pts);
  const float r2 = radius * radius;      // the float32 square (+inf stays, and a large radius may become, +inf)
  GsrNormalsView view;
  view.on = viewpoint ? 1 : 0;
  view.x = viewpoint ? viewpoint[0] : 0.f;
  view.y = viewpoint ? viewpoint[1] : 0.f;
  view.z = viewpoint ? viewpoint[2] : 0.f;
  const int k = (int)max_nn - 1;
#define NORMALS_K(K) \
  GSR_LAUNCH("normals_k" #K, k_normals<K>, dim3(nblk), dim3(256), 0, st, t, k, r2, view, normals, count_out, eigenvalues_out)
  GSR_KNN_PICK_K(k, NORMALS_K);
#undef NORMALS_K
  return gsr_launch_status("estimate_normals launch");
}

}  // extern "C"
