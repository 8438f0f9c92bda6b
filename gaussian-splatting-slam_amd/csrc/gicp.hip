// gicp.hip - generalized ICP (Segal, Haehnel, Thrun 2009; Open3D's registration_generalized_icp): every pair is weighted by the
// combined covariance of BOTH surfaces, M = Sigma_t + R Sigma_s R^T.  Flat covariances on both sides: plane-to-plane.  Isotropic
// ones: point-to-point, so the 6 x 6 system stays solvable on a single plane, where gsr_icp_update_plane's does not.  The
// Gaussians' own covariances as the target's: a scan registered to the splat map.
//
// gsr_estimate_covariances: normals.hip's launch with another ending.  The structure of knn.hip over the cloud, non-finite rows
//   masked, then ONE launch, one thread per query in Morton order: knn_topk_bound gives min(r2, d_k), knn_member_walk the float64
//   sums S1, S2 over exactly N_i of gsr_estimate_normals, C = S2 / n - (S1 / n)(S1 / n)^T; then the body below.
// gsr_regularize_covariances: one thread per row over covariances that are given; the body below.
// gicp_regularised (ONE body, both callers): cyclic Jacobi (normals_rotate, GSR_NORMALS_SWEEPS: jacobi3_common.h, the normals'
//   own), the column of the smallest diagonal entry (the first on ties), normalised again in float64, Sigma = I - (1 - eps) w w^T
//   = V diag(eps, 1, 1) V^T - Open3D's regularisation; w enters as a square, so no sign rule is needed.
// gsr_icp_update_generalized: gsr_icp_update_plane's structure - k_icp_shift and icp_begin (icp_common.h), a partial kernel of at
//   most GSR_GN_BLOCKS workgroups over fixed slices, k_gn6_final<3> (solve6_common.h).  Per row 12 + 24 bytes are gathered through
//   idx and 12 + 24 + 4 streamed; M, its adjugate inverse W, J^T W J and J^T W d in float64, about 250 operations.
#include "knn_common.h"
#include "jacobi3_common.h"
#include "icp_common.h"

// No implicit fma contraction below the shared headers (see odometry.hip): the order written here is the order executed, which is
// what include/gsr.h states and a float64 restatement follows.
#pragma clang fp contract(off)

#define GSR_GICP_H 3                                     // n, sum |d|^2, sum d^T W d
#define GSR_GICP_SUMS (GSR_GICP_H + GSR_GN6_TERMS)       // ... J^T W d [6], upper triangle of J^T W J [21]

__device__ __forceinline__ bool gicp_finite(double x) { return fabs(x) < (double)KNN_INF; }

// rows with a non-finite coordinate become NaN NaN NaN (.w, the original row, stays)
__global__ __launch_bounds__(256) void k_gicp_mask(uint32_t P, float4* __restrict__ pts) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P) return;
  pts[j] = knn_mask_non_finite(pts[j]);
}

// Sigma = I - (1 - eps) w w^T, w the unit eigenvector of the smallest eigenvalue of the symmetric (a00 .. a22), as float32
// xx, xy, xz, yy, yz, zz; the identity where the three diagonal entries after the sweeps are equal (a00 == a11 && a11 == a22)
__device__ __forceinline__ void gicp_regularised(double a00, double a01, double a02, double a11, double a12, double a22, double eps,
                                                 float* __restrict__ out) {
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < GSR_NORMALS_SWEEPS; sweep++) {
    normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), third index 2
    normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), third index 1
    normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), third index 0
  }
  if (a00 == a11 && a11 == a22) {      // no direction is the flat one
    out[0] = 1.f; out[1] = 0.f; out[2] = 0.f; out[3] = 1.f; out[4] = 0.f; out[5] = 1.f;
    return;
  }
  // the column of the smallest diagonal entry (the first on ties), as k_normals picks it
  const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
  double wx = c0 ? v00 : (c1 ? v01 : v02), wy = c0 ? v10 : (c1 ? v11 : v12), wz = c0 ? v20 : (c1 ? v21 : v22);
  const double norm = sqrt((wx * wx + wy * wy) + wz * wz);
  wx /= norm; wy /= norm; wz /= norm;
  const double k = 1.0 - eps;
  const double kx = k * wx, ky = k * wy, kz = k * wz;
  out[0] = (float)(1.0 - kx * wx);
  out[1] = (float)(0.0 - kx * wy);
  out[2] = (float)(0.0 - kx * wz);
  out[3] = (float)(1.0 - ky * wy);
  out[4] = (float)(0.0 - ky * wz);
  out[5] = (float)(1.0 - kz * wz);
}

template <int K>
__global__ __launch_bounds__(256) void k_gicp_covariances(GsrKnnTree t, int k, float r2, double eps, float* __restrict__ cov_out,
                                                          int32_t* __restrict__ count_out) {
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
  // ---- sweep 2: the sums over { j != i : d2 <= bound }, as k_normals forms them ----
  double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  uint32_t members = 0u;
  knn_member_walk<256>(t, me, pos, active, bound, s_lo, s_hi,
                       [&](const uint32_t, const float fx, const float fy, const float fz) __attribute__((always_inline)) {
                         const double dx = -(double)fx, dy = -(double)fy, dz = -(double)fz;      // delta = p_j - p_i, exactly
                         members++;
                         s1x += dx; s1y += dy; s1z += dz;
                         sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                         syy += dy * dy; syz += dy * dz; szz += dz * dz;
                       });
  if (!active) return;
  const size_t row = (size_t)__float_as_uint(me.w);      // (< P: the index build wrote it)
  const bool finite = knn_finite(me.x) && knn_finite(me.y) && knn_finite(me.z);
  const uint32_t count = finite ? members + 1u : 0u;
  if (count_out) count_out[row] = (int32_t)count;
  float* out = cov_out + 6 * row;
  if (!finite) {
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int a = 0; a < 6; a++) out[a] = nan;
  } else if (count < 3u) {
    out[0] = 1.f; out[1] = 0.f; out[2] = 0.f; out[3] = 1.f; out[4] = 0.f; out[5] = 1.f;
  } else {
    const double n = (double)count;
    const double mx = s1x / n, my = s1y / n, mz = s1z / n;
    gicp_regularised(sxx / n - mx * mx, sxy / n - mx * my, sxz / n - mx * mz, syy / n - my * my, syz / n - my * mz,
                     szz / n - mz * mz, eps, out);
  }
}

// one thread per row; `out` may be `in` (a row is read completely before it is written, by the thread that writes it)
__global__ __launch_bounds__(256) void k_gicp_regularize(uint32_t P, const float* in, double eps, float* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  float c[6];
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    c[a] = in[6 * (size_t)i + a];
    finite = finite && knn_finite(c[a]);
  }
  float r[6];
  if (!finite) {
#pragma unroll
    for (int a = 0; a < 6; a++) r[a] = __builtin_nanf("");
  } else {
    gicp_regularised((double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4], (double)c[5], eps, r);
  }
#pragma unroll
  for (int a = 0; a < 6; a++) out[6 * (size_t)i + a] = r[a];
}

// ---- one generalized update --------------------------------------------------------------------------------------------------------
// per workgroup: s[0] = n, s[1] = sum |d|^2, s[2] = sum d^T W d, s[3..8] = J^T W d, s[9..29] = J^T W J rows 0 .. 5 from the diagonal on
__global__ __launch_bounds__(256) void k_gicp_partial(uint32_t Ps, const float* __restrict__ src, const float* __restrict__ scov,
                                                      uint32_t Pt, const float* __restrict__ tgt, const float* __restrict__ tcov,
                                                      const int32_t* __restrict__ idx, const double* __restrict__ T_dev,
                                                      const double* __restrict__ shift, double* __restrict__ part) {
  const RegT T = reg_load(T_dev);
  const double c0 = shift[0], c1 = shift[1], c2 = shift[2];
  double s[GSR_GICP_SUMS];
#pragma unroll
  for (int a = 0; a < GSR_GICP_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < Ps; i += gridDim.x * 256u) {
    float4 qf, pf;
    if (!icp_pair(i, src, Pt, tgt, idx, T, qf, pf)) continue;      // (0 <= idx[i] < Pt from here on)
    const size_t k = (size_t)idx[i];
    double S[6], C[6];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      const float sv = scov[6 * (size_t)i + a], tv = tcov[6 * k + a];
      finite = finite && knn_finite(sv) && knn_finite(tv);
      S[a] = (double)sv;
      C[a] = (double)tv;
    }
    if (!finite) continue;
    // A = R Sigma_s, B = A R^T (the upper triangle), M = Sigma_t + B
    const double Ss[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    double A[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) A[a][b] = (T.m[4 * a] * Ss[0][b] + T.m[4 * a + 1] * Ss[1][b]) + T.m[4 * a + 2] * Ss[2][b];
    }
    double M[6];
    {
      int o = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = a; b < 3; b++) {
          M[o] = C[o] + ((A[a][0] * T.m[4 * b] + A[a][1] * T.m[4 * b + 1]) + A[a][2] * T.m[4 * b + 2]);
          o++;
        }
      }
    }
    // W = adj(M) / det M; M = [m0 m1 m2; m1 m3 m4; m2 m4 m5]
    const double k00 = M[3] * M[5] - M[4] * M[4], k01 = M[2] * M[4] - M[1] * M[5], k02 = M[1] * M[4] - M[2] * M[3];
    const double k11 = M[0] * M[5] - M[2] * M[2], k12 = M[1] * M[2] - M[0] * M[4], k22 = M[0] * M[3] - M[1] * M[1];
    const double det = (M[0] * k00 + M[1] * k01) + M[2] * k02;
    if (!(gicp_finite(det) && det > 0.0)) continue;
    const double W[3][3] = {{k00 / det, k01 / det, k02 / det}, {k01 / det, k11 / det, k12 / det}, {k02 / det, k12 / det, k22 / det}};
    // (float32 values: the differences below are exact in float64)
    const double q[3] = {(double)qf.x - c0, (double)qf.y - c1, (double)qf.z - c2};
    const double d[3] = {(double)qf.x - (double)pf.x, (double)qf.y - (double)pf.y, (double)qf.z - (double)pf.z};
    // J = [-[q']x, I]: column a of the rotation block is e_a x q'
    const double J[3][6] = {{0.0, q[2], -q[1], 1.0, 0.0, 0.0}, {-q[2], 0.0, q[0], 0.0, 1.0, 0.0}, {q[1], -q[0], 0.0, 0.0, 0.0, 1.0}};
    double G[3][6];      // W J
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int a = 0; a < 6; a++) G[r][a] = (W[r][0] * J[0][a] + W[r][1] * J[1][a]) + W[r][2] * J[2][a];
    }
    double Wd[3];
#pragma unroll
    for (int r = 0; r < 3; r++) Wd[r] = (W[r][0] * d[0] + W[r][1] * d[1]) + W[r][2] * d[2];
    s[0] += 1.0;
    s[1] += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    s[2] += (d[0] * Wd[0] + d[1] * Wd[1]) + d[2] * Wd[2];
    int o = 9;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      s[3 + a] += (J[0][a] * Wd[0] + J[1][a] * Wd[1]) + J[2][a] * Wd[2];
#pragma unroll
      for (int b = a; b < 6; b++) s[o++] += (J[0][a] * G[0][b] + J[1][a] * G[1][b]) + J[2][a] * G[2][b];
    }
  }
  gsr_block_sum_store(s, part);
}

extern "C" {

size_t gsr_covariance_workspace_bytes(int64_t P) { return nn_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_estimate_covariances(int64_t P, const float* points, float radius, int32_t max_nn, double epsilon, float* cov_out,
                             int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(P) || !points || !cov_out || !workspace || max_nn < 3 || max_nn > GSR_KNN_K_MAX + 1 || !(radius > 0.f) ||
      !(epsilon > 0.0 && epsilon <= 1.0)) {
    gsr_set_error("estimate_covariances: bad arguments (P = %lld, radius = %g: expected > 0, max_nn = %d: expected 3 .. %d, "
                  "epsilon = %g: expected > 0 and <= 1)", (long long)P, (double)radius, (int)max_nn, GSR_KNN_K_MAX + 1, epsilon);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrNnBlob w = nn_ws(workspace, (size_t)P);      // (the blob of a target index: knn_common.h)
  if (!gsr_workspace_fits("estimate_covariances", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const GsrNnWs& b = w.nn;
  gsr_knn_build(P, points, b, st);
  const GsrKnnTree t = knn_tree(b, (size_t)P);
  const uint32_t nblk = (t.P + 255u) / 256u;
  GSR_LAUNCH("gicp_mask", k_gicp_mask, dim3(nblk), dim3(256), 0, st, t.P, b.pts);
  const float r2 = radius * radius;      // the float32 square (+inf stays, and a large radius may become, +inf)
  const int k = (int)max_nn - 1;
#define GICP_K(K) \
  GSR_LAUNCH("gicp_covariances_k" #K, k_gicp_covariances<K>, dim3(nblk), dim3(256), 0, st, t, k, r2, epsilon, cov_out, count_out)
  GSR_KNN_PICK_K(k, GICP_K);
#undef GICP_K
  return gsr_launch_status("estimate_covariances launch");
}

int gsr_regularize_covariances(int64_t P, const float* cov_in, double epsilon, float* cov_out, void* stream) {
  if (gsr_bad_size(P) || !cov_in || !cov_out || !(epsilon > 0.0 && epsilon <= 1.0)) {
    gsr_set_error("regularize_covariances: bad arguments (P = %lld, epsilon = %g: expected > 0 and <= 1)", (long long)P, epsilon);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const uint32_t n = (uint32_t)P;
  GSR_LAUNCH("gicp_regularize", k_gicp_regularize, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, n, cov_in, epsilon,
             cov_out);
  return gsr_launch_status("regularize_covariances launch");
}

size_t gsr_icp_generalized_workspace_bytes(int64_t Ps) {
  (void)Ps;      // (as gsr_icp_workspace_bytes: at most GSR_GN_BLOCKS rows of partial sums)
  return gn_ws(nullptr, GSR_GICP_SUMS, true).total;
}

int gsr_icp_update_generalized(int64_t Ps, const float* source, const float* source_cov, int64_t Pt, const float* target,
                               const float* target_cov, const int32_t* idx, double* T_dev, double* stats_dev, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Ps) || gsr_bad_size(Pt) || !source || !source_cov || !target || !target_cov || !idx || !T_dev || !stats_dev ||
      !workspace) {
    gsr_set_error("icp_update_generalized: bad arguments (Ps = %lld, Pt = %lld)", (long long)Ps, (long long)Pt);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  IcpRun r;
  if (const int rc = icp_begin("icp_update_generalized", GSR_GICP_SUMS, Ps, source, Pt, target, idx, T_dev, workspace,
                               workspace_bytes, stream, r))
    return rc;
  GSR_LAUNCH("gicp_partial", k_gicp_partial, dim3(r.sblk), dim3(256), 0, r.st, r.ns, source, source_cov, r.nt, target, target_cov,
             idx, (const double*)T_dev, (const double*)r.shift, r.part);
  GSR_LAUNCH("gicp_final", k_gn6_final<GSR_GICP_H>, dim3(1), dim3(256), 0, r.st, r.sblk, (double)r.ns, 1, (const double*)r.part,
             (const double*)r.shift, T_dev, stats_dev);
  return gsr_launch_status("icp_update_generalized launch");
}

}  // extern "C"
