// transform.hip - moves Gaussians that are already in the map into a corrected world frame (include/gsr.h,
// gsr_transform_gaussians): a loop closure or pose-graph update moved the keyframes the rows were
// created from, a map is aligned to another frame (with a scale factor), two sub-maps are merged.
//
// A transform is x' = s R x + t (R a proper rotation, s > 0), given as a float64 4x4.  For a row that moves:
//   xyz            s R x + t, formed in float64 from the float32 input and rounded once (a map far from the origin keeps its bits)
//   rotation       q' = q_R (x) q_raw, the Hamilton product with the unit quaternion of R: the raw norm is preserved
//   scaling        log-scale + ln s
//   features_rest  SH bands 1..3 live in the WORLD frame: per colour channel c'_l = D_l(R) c_l with the (2l+1)x(2l+1) real-SH
//                  rotation matrix of band l
//   Adam moments   (optional) zeroed: they describe gradients in the old frame
// features_dc and opacity are invariant.  Two kernels:
//   k_transform_table  one lane per transform, float64: s, R, t, the quaternion, ln s and D_1..D_3.  D_l = A_l^-1 B_l(dirs R) with
//                      2l+1 fixed sample directions whose basis matrix A_l is well conditioned (transform_constants.inc, generated
//                      from scene_utils/sh_rotation.py): B_l(d) D_l = B_l(d R) holds for every direction d (as a row), so it
//                      holds for the samples, and they determine D_l.
//   k_transform_rows   one thread per row, one pass.  The rows of features_rest are 3 M floats (180 B at degree 3): a workgroup's
//                      256 rows are one contiguous span that moves as flat 16-B pieces through LDS (rows at an odd stride, so the
//                      thread that then walks its own row meets no bank conflict), never as per-thread strided pieces.
// A row whose anchor names no transform is not written at all; a 16-B piece that straddles a moved and an unmoved row is stored
// float by float.  No atomics, every sum in a fixed order: bitwise reproducible.
#include "gsr_common.h"

namespace {

#define XF_CONST static __device__ const
#include "transform_constants.inc"

// One transform as the row kernel reads it (private to this file).  Every member starts on a 16-B boundary.
struct XfEntry {
  double sR[9];     // s R, row-major
  double t[3];
  float q[4];       // unit quaternion of R, (w, x, y, z)
  float ln_s, s, pad0, pad1;
  float D[84];      // D_1 [3][3], D_2 [5][5], D_3 [7][7] row-major, one float of padding
};
static_assert(sizeof(XfEntry) % 16 == 0, "table entries are read as 16-B pieces");
#define XF_D1 0
#define XF_D2 9
#define XF_D3 34

// band l of the real SH basis at unit direction (x, y, z): scene_utils/sh.py (reference utils/sh_utils.py:57-112), float64
__device__ __forceinline__ void sh_band1(double x, double y, double z, double* b) {
  const double C1 = 0.4886025119029199;
  b[0] = -C1 * y; b[1] = C1 * z; b[2] = -C1 * x;
}
__device__ __forceinline__ void sh_band2(double x, double y, double z, double* b) {
  const double xx = x * x, yy = y * y, zz = z * z;
  b[0] = 1.0925484305920792 * x * y;
  b[1] = -1.0925484305920792 * y * z;
  b[2] = 0.31539156525252005 * (2.0 * zz - xx - yy);
  b[3] = -1.0925484305920792 * x * z;
  b[4] = 0.5462742152960396 * (xx - yy);
}
__device__ __forceinline__ void sh_band3(double x, double y, double z, double* b) {
  const double xx = x * x, yy = y * y, zz = z * z;
  b[0] = -0.5900435899266435 * y * (3.0 * xx - yy);
  b[1] = 2.890611442640554 * x * y * z;
  b[2] = -0.4570457994644658 * y * (4.0 * zz - xx - yy);
  b[3] = 0.3731763325901154 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
  b[4] = -0.4570457994644658 * x * (4.0 * zz - xx - yy);
  b[5] = 1.445305721320277 * z * (xx - yy);
  b[6] = -0.5900435899266435 * x * (xx - 3.0 * yy);
}

// D = AINV . B_l(DIRS R), rounded to float32 once
template <int L, typename F>
__device__ __forceinline__ void band_matrix(const double (&dirs)[2 * L + 1][3], const double (&ainv)[2 * L + 1][2 * L + 1],
                                            const double* R, F basis, float* D) {
  constexpr int N = 2 * L + 1;
  double E[N][N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    // row vector times R: e_c = sum_r d_r R[r][c]
    const double ex = dirs[j][0] * R[0] + dirs[j][1] * R[3] + dirs[j][2] * R[6];
    const double ey = dirs[j][0] * R[1] + dirs[j][1] * R[4] + dirs[j][2] * R[7];
    const double ez = dirs[j][0] * R[2] + dirs[j][1] * R[5] + dirs[j][2] * R[8];
    basis(ex, ey, ez, E[j]);
  }
#pragma unroll
  for (int a = 0; a < N; a++)
#pragma unroll
    for (int b = 0; b < N; b++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; j++) s += ainv[a][j] * E[j][b];
      D[a * N + b] = (float)s;
    }
}

__global__ __launch_bounds__(64) void k_transform_table(int K, const double* __restrict__ transforms, XfEntry* __restrict__ table) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const double* T = transforms + 16 * (size_t)k;
  double M[9], R[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[3 * i + j] = T[4 * i + j];
  // det(s R) = s^3
  const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  const double s = cbrt(det);
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = M[i] / s;
  XfEntry e;
#pragma unroll
  for (int i = 0; i < 9; i++) e.sR[i] = M[i];
#pragma unroll
  for (int i = 0; i < 3; i++) e.t[i] = T[4 * i + 3];
  // unit quaternion of R (Shepperd: the largest of trace, R00, R11, R22 picks the component that is formed from a square root,
  // which is therefore positive - the sign convention scene_utils.transform.quat_from_matrix states too)
  const double tr = R[0] + R[4] + R[8];
  double qw, qx, qy, qz;
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    const double r = sqrt(1.0 + tr);
    const double h = 0.5 / r;
    qw = 0.5 * r; qx = (R[7] - R[5]) * h; qy = (R[2] - R[6]) * h; qz = (R[3] - R[1]) * h;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double r = sqrt(1.0 + R[0] - R[4] - R[8]);
    const double h = 0.5 / r;
    qx = 0.5 * r; qw = (R[7] - R[5]) * h; qy = (R[1] + R[3]) * h; qz = (R[2] + R[6]) * h;
  } else if (R[4] >= R[8]) {
    const double r = sqrt(1.0 - R[0] + R[4] - R[8]);
    const double h = 0.5 / r;
    qy = 0.5 * r; qw = (R[2] - R[6]) * h; qx = (R[1] + R[3]) * h; qz = (R[5] + R[7]) * h;
  } else {
    const double r = sqrt(1.0 - R[0] - R[4] + R[8]);
    const double h = 0.5 / r;
    qz = 0.5 * r; qw = (R[3] - R[1]) * h; qx = (R[2] + R[6]) * h; qy = (R[5] + R[7]) * h;
  }
  const double qn = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  e.q[0] = (float)(qw * qn); e.q[1] = (float)(qx * qn); e.q[2] = (float)(qy * qn); e.q[3] = (float)(qz * qn);
  e.ln_s = (float)log(s);
  e.s = (float)s;
  e.pad0 = e.pad1 = 0.f;
  band_matrix<1>(XF_DIRS1, XF_AINV1, R, sh_band1, e.D + XF_D1);
  band_matrix<2>(XF_DIRS2, XF_AINV2, R, sh_band2, e.D + XF_D2);
  band_matrix<3>(XF_DIRS3, XF_AINV3, R, sh_band3, e.D + XF_D3);
  e.D[83] = 0.f;
  table[k] = e;
}

// exp_avg / exp_avg_sq of xyz, rotation, scaling, f_rest - each may be NULL
struct XfMoments {
  float* p[8];
};

// c_l <- D_l c_l for the three channels of one LDS row; coefficient k of channel ch sits at row[3 k + ch]
template <int N, int OFF>
__device__ __forceinline__ void rotate_band(float* row, const float* __restrict__ D) {
  float d[N * N];
#pragma unroll
  for (int i = 0; i < N * N; i++) d[i] = D[i];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    float c[N];
#pragma unroll
    for (int b = 0; b < N; b++) c[b] = row[3 * (OFF + b) + ch];
#pragma unroll
    for (int a = 0; a < N; a++) {
      float acc = d[a * N] * c[0];
#pragma unroll
      for (int b = 1; b < N; b++) acc = __builtin_fmaf(d[a * N + b], c[b], acc);
      row[3 * (OFF + a) + ch] = acc;
    }
  }
}

#define XF_BT 256

// S = floats per features_rest row (0, 9, 24, 45).  UNIFORM: no anchors, every row moves by entry 0 (its loads are scalar).
template <int S, bool UNIFORM>
__global__ __launch_bounds__(XF_BT) void k_transform_rows(int P, const int32_t* __restrict__ anchor, int K,
                                                          const XfEntry* __restrict__ table, float* __restrict__ xyz,
                                                          float* __restrict__ rotation, float* __restrict__ scaling,
                                                          float* __restrict__ frest, XfMoments mom) {
  constexpr int SD = S ? S : 1;                   // (divisor: S == 0 instantiates, never runs, the SH part)
  constexpr int Sp = S | 1;                       // LDS row stride: odd
  constexpr int TRIPS = S ? (S + 3) / 4 : 1;              // 16-B pieces per thread: 256 rows x S floats / 4 / 256 threads
  __shared__ int s_a[XF_BT];                      // the row's table entry, -1 = the row stays
  __shared__ __attribute__((aligned(16))) float s_sh[S ? XF_BT * Sp : 1];
  const int tid = (int)threadIdx.x;
  const int row0 = (int)blockIdx.x * XF_BT;
  const int rows = min(XF_BT, P - row0);
  const int i = row0 + tid;
  int a = -1;
  if (tid < rows) {
    a = UNIFORM ? 0 : anchor[i];
    if (a < 0 || a >= K) a = -1;
  }
  s_a[tid] = a;
  __syncthreads();

  // ---- features_rest in: the span of this workgroup's rows as flat 16-B pieces; pieces no moved row touches are not fetched ----
  const int nflt = rows * S, n4 = nflt >> 2;
  float* span = S ? frest + (size_t)row0 * S : nullptr;
  if (S) {
    float4 v[TRIPS];
    bool want[TRIPS];
#pragma unroll
    for (int it = 0; it < TRIPS; it++) {
      const int p = tid + XF_BT * it, e = 4 * p;
      want[it] = p < n4;
      if (!UNIFORM && want[it]) want[it] = s_a[e / SD] >= 0 || s_a[(e + 3) / SD] >= 0;     // a piece spans at most two rows (S >= 4)
      if (want[it]) v[it] = gsr_ld_stream4(reinterpret_cast<const float4*>(span) + p);
    }
#pragma unroll
    for (int it = 0; it < TRIPS; it++) {
      if (!want[it]) continue;
      const int e = 4 * (tid + XF_BT * it);
      if (Sp == S) {                              // the LDS image is the span itself
        *reinterpret_cast<float4*>(&s_sh[e]) = v[it];
      } else {
        const float vv[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        int r = e / SD, c = e - r * S;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          s_sh[r * Sp + c] = vv[k];
          if (++c == S) { c = 0; r++; }
        }
      }
    }
    for (int e = n4 * 4 + tid; e < nflt; e += XF_BT) {       // (the last workgroup's 1..3 floats behind the last whole piece)
      const int r = e / SD;
      if (UNIFORM || s_a[r] >= 0) s_sh[r * Sp + (e - r * S)] = span[e];
    }
  }

  // ---- the short rows, one thread each (the three streams of a wave are contiguous 768-B / 1-KB spans) ----
  const XfEntry* T = UNIFORM ? table : table + (a < 0 ? 0 : a);
  if (a >= 0) {
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const double x = (double)xyz[i3], y = (double)xyz[i3 + 1], z = (double)xyz[i3 + 2];
#pragma unroll
    for (int r = 0; r < 3; r++)
      xyz[i3 + r] = (float)(fma(T->sR[3 * r], x, fma(T->sR[3 * r + 1], y, fma(T->sR[3 * r + 2], z, T->t[r]))));
    const float4 q = *reinterpret_cast<const float4*>(rotation + i4);
    const float a0 = T->q[0], a1 = T->q[1], a2 = T->q[2], a3 = T->q[3];
    float4 o;
    o.x = __builtin_fmaf(-a3, q.w, __builtin_fmaf(-a2, q.z, __builtin_fmaf(-a1, q.y, a0 * q.x)));
    o.y = __builtin_fmaf(-a3, q.z, __builtin_fmaf(a2, q.w, __builtin_fmaf(a1, q.x, a0 * q.y)));
    o.z = __builtin_fmaf(a3, q.y, __builtin_fmaf(a2, q.x, __builtin_fmaf(-a1, q.w, a0 * q.z)));
    o.w = __builtin_fmaf(a3, q.x, __builtin_fmaf(-a2, q.y, __builtin_fmaf(a1, q.z, a0 * q.w)));
    *reinterpret_cast<float4*>(rotation + i4) = o;
    if (scaling) {
      const float ls = T->ln_s;
#pragma unroll
      for (int r = 0; r < 3; r++) scaling[i3 + r] += ls;
    }
#pragma unroll
    for (int m = 0; m < 2; m++) {
      if (mom.p[m]) { mom.p[m][i3] = 0.f; mom.p[m][i3 + 1] = 0.f; mom.p[m][i3 + 2] = 0.f; }
      if (mom.p[2 + m]) *reinterpret_cast<float4*>(mom.p[2 + m] + i4) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (mom.p[4 + m]) { mom.p[4 + m][i3] = 0.f; mom.p[4 + m][i3 + 1] = 0.f; mom.p[4 + m][i3 + 2] = 0.f; }
    }
  }
  if (!S) return;
  __syncthreads();

  // ---- every thread rotates its own row in LDS ----
  if (a >= 0) {
    float* row = s_sh + tid * Sp;
    rotate_band<3, 0>(row, T->D + XF_D1);
    if (S >= 24) rotate_band<5, 3>(row, T->D + XF_D2);
    if (S >= 45) rotate_band<7, 8>(row, T->D + XF_D3);
  }
  __syncthreads();

  // ---- features_rest out (and zeros into its moments): whole pieces where both rows of the piece moved ----
  float* const m_avg = mom.p[6] ? mom.p[6] + (size_t)row0 * S : nullptr;
  float* const m_sq = mom.p[7] ? mom.p[7] + (size_t)row0 * S : nullptr;
#pragma unroll
  for (int it = 0; it < TRIPS; it++) {
    const int p = tid + XF_BT * it, e = 4 * p;
    if (p >= n4) continue;
    int r = e / SD, c = e - r * S;
    const bool m0 = UNIFORM || s_a[r] >= 0, m1 = UNIFORM || s_a[(e + 3) / SD] >= 0;
    if (!m0 && !m1) continue;
    float vv[4];
    bool mv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      mv[k] = (r == e / SD) ? m0 : m1;
      vv[k] = mv[k] ? s_sh[r * Sp + c] : 0.f;
      if (++c == S) { c = 0; r++; }
    }
    if (m0 && m1) {
      gsr_st_stream4(reinterpret_cast<float4*>(span) + p, make_float4(vv[0], vv[1], vv[2], vv[3]));
      if (m_avg) gsr_st_stream4(reinterpret_cast<float4*>(m_avg) + p, make_float4(0.f, 0.f, 0.f, 0.f));
      if (m_sq) gsr_st_stream4(reinterpret_cast<float4*>(m_sq) + p, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (mv[k]) {
          span[e + k] = vv[k];
          if (m_avg) m_avg[e + k] = 0.f;
          if (m_sq) m_sq[e + k] = 0.f;
        }
    }
  }
  for (int e = n4 * 4 + tid; e < nflt; e += XF_BT) {
    const int r = e / SD;
    if (UNIFORM || s_a[r] >= 0) {
      span[e] = s_sh[r * Sp + (e - r * S)];
      if (m_avg) m_avg[e] = 0.f;
      if (m_sq) m_sq[e] = 0.f;
    }
  }
}

template <int S>
void launch_rows(bool uniform, dim3 grid, hipStream_t st, int P, const int32_t* anchor, int K, const XfEntry* table, float* xyz,
                 float* rotation, float* scaling, float* frest, const XfMoments& mom) {
  if (uniform)
    GSR_LAUNCH("transform_rows", (k_transform_rows<S, true>), grid, dim3(XF_BT), 0, st, P, anchor, K, table, xyz, rotation, scaling,
               frest, mom);
  else
    GSR_LAUNCH("transform_rows", (k_transform_rows<S, false>), grid, dim3(XF_BT), 0, st, P, anchor, K, table, xyz, rotation,
               scaling, frest, mom);
}

}  // namespace

// the workspace of gsr_transform_gaussians: the table of K prepared transforms
struct XfWs {
  XfEntry* table;      // XfEntry[K]
  size_t total;
};
static XfWs xf_ws(void* base, int32_t K) {
  GsrCarve c(base);
  XfWs w;
  w.table = c.take<XfEntry>((size_t)(K < 1 ? 1 : K));
  w.total = c.o;
  return w;
}

extern "C" size_t gsr_transform_workspace_bytes(int32_t K) { return xf_ws(nullptr, K).total; }

extern "C" int gsr_transform_gaussians(int64_t P, const int32_t* anchor, int32_t K, const double* transforms, void* workspace,
                                       size_t workspace_bytes, float* xyz, float* rotation, float* scaling_raw,
                                       float* features_rest, int32_t sh_coeffs_rest, float* const* moments8, void* stream) {
  if (sh_coeffs_rest != 0 && sh_coeffs_rest != 3 && sh_coeffs_rest != 8 && sh_coeffs_rest != 15) {
    gsr_set_error("transform_gaussians: sh_coeffs_rest = %d, expected 0, 3, 8 or 15", (int)sh_coeffs_rest);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (P < 0 || P > 0x7FFFFFFF || K < 0) {
    gsr_set_error("transform_gaussians: P = %lld, K = %d out of range", (long long)P, (int)K);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const XfWs w = xf_ws(workspace, K);
  if (K > 0 && !gsr_workspace_fits("transform_gaussians", workspace, workspace_bytes, w.total)) return GSR_ERR_INVALID_ARGUMENT;
  if (P > 0 && !xyz) {
    gsr_set_error("transform_gaussians: xyz is NULL");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (P == 0 || K == 0) return 0;
  if (!transforms || !rotation || (sh_coeffs_rest > 0 && !features_rest)) {
    gsr_set_error("transform_gaussians: transforms, rotation or features_rest is NULL");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  XfMoments mom;
  for (int k = 0; k < 8; k++) mom.p[k] = moments8 ? moments8[k] : nullptr;
  if (sh_coeffs_rest == 0) mom.p[6] = mom.p[7] = nullptr;
  // rotation rows, features_rest spans and their moments move as 16-B pieces
  const uintptr_t mis = (uintptr_t)rotation | (uintptr_t)features_rest | (uintptr_t)mom.p[2] | (uintptr_t)mom.p[3] |
                        (uintptr_t)mom.p[6] | (uintptr_t)mom.p[7] | (uintptr_t)workspace;
  if (mis & 15) {
    gsr_set_error("transform_gaussians: rotation, features_rest, their moments and the workspace must be 16-byte aligned");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  XfEntry* table = w.table;
  GSR_LAUNCH("transform_table", k_transform_table, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, (int)K, transforms, table);
  const dim3 grid((unsigned)((P + XF_BT - 1) / XF_BT));
  const bool uniform = anchor == nullptr;
  switch (sh_coeffs_rest) {
    case 0: launch_rows<0>(uniform, grid, st, (int)P, anchor, K, table, xyz, rotation, scaling_raw, features_rest, mom); break;
    case 3: launch_rows<9>(uniform, grid, st, (int)P, anchor, K, table, xyz, rotation, scaling_raw, features_rest, mom); break;
    case 8: launch_rows<24>(uniform, grid, st, (int)P, anchor, K, table, xyz, rotation, scaling_raw, features_rest, mom); break;
    default: launch_rows<45>(uniform, grid, st, (int)P, anchor, K, table, xyz, rotation, scaling_raw, features_rest, mom); break;
  }
  return gsr_launch_status("transform_gaussians launch");
}
