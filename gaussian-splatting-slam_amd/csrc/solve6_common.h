// solve6_common.h - the 6-unknown Gauss-Newton step of include/gsr.h, shared by registration.hip (gsr_icp_update_plane,
// gsr_icp_update_colored) and odometry.hip (gsr_odometry_update): ONE workspace description, ONE final kernel (the rows of partial sums,
// the stats header, the n < 6 rule, the unpacking of the triangle) and ONE body for the LDL^T solve, the vector-to-matrix
// composition and T <- dT T (posegraph.hip takes the same three for its 6 x 6 node blocks and its pose update), so the
// thresholds, the stats layout, the pivot rule and the order of operations agree by construction.  What differs between the updates stays in their files: the partial kernel that forms a workgroup's row
//   s[0] = n, s[1 .. H-1] = sums of squared residuals, s[H .. H+5] = J^T r, s[H+6 .. H+26] = J^T J rows 0 .. 5 from the diagonal on.
// (Everything here is defined above odometry.hip's `fp contract(off)`: both files compile these bodies alike.)
#pragma once
#include "gsr_common.h"

#define GSR_ICP_PIVOT_MIN 1e-12   // LDL^T: a pivot at or below this share of its diagonal entry is no pivot
#define GSR_GN_BLOCKS 256         // workgroups of a partial kernel at most = rows of partial sums
#define GSR_GN6_TERMS 27          // J^T r [6], upper triangle of J^T J [21]: what follows the H header sums of a row

// workspace of an update: the rows of partial sums do not grow with the cloud or the image
struct GsrGnWs {
  double* shift;     // double[4]: the shift, [3] = 1 when a valid row exists (with_shift only, else NULL)
  double* part;      // double[GSR_GN_BLOCKS][sums]
  size_t total;
};
static inline GsrGnWs gn_ws(void* base, int sums, bool with_shift) {
  GsrCarve c(base);
  GsrGnWs w;
  w.shift = with_shift ? c.take<double>(4) : nullptr;
  w.part = c.take<double>((size_t)GSR_GN_BLOCKS * sums);
  w.total = c.o;
  return w;
}
// workgroups of a partial kernel over n rows or pixels: 256 each, the rest by the grid-stride loop
static inline uint32_t gn_partial_blocks(uint32_t n) {
  const uint32_t nblk = (n + 255u) / 256u;
  return nblk < (uint32_t)GSR_GN_BLOCKS ? nblk : (uint32_t)GSR_GN_BLOCKS;
}

#ifdef __HIPCC__
// thread 0 of a final kernel: stats[0..2] and [4..7] of include/gsr.h from a summed row with H header sums (s[0] = n, s[1] = the
// sum the RMSE is taken from); stats[3] is the caller's
template <int H, int N>
__device__ __forceinline__ void gn_stats_header(const double (&s)[N], double denom, double* __restrict__ stats) {
  const double n = s[0];
  stats[0] = n;
  stats[1] = n / denom;
  stats[2] = n > 0.0 ? sqrt(s[1] / n) : 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) stats[4 + k] = k < H - 1 ? s[1 + k] : 0.0;
}

// The three bodies of the step, shared with posegraph.hip (one 6 x 6 block per node there): the LDL^T factorisation with its pivot
// rule, the two triangular solves, and M(x): dR = Rz(gamma) Ry(beta) Rx(alpha) with T <- [dR, td] T.  The arrays are indexed at
// run time: LDS in the one-thread callers below, per-thread arrays (unrolled by the compiler) in posegraph.hip.
// A = L D L^T, L unit lower triangular; every pivot is held against its own diagonal entry (scale-free per unknown).  false: a
// pivot that is not finite or is <= GSR_ICP_PIVOT_MIN x its diagonal entry
__device__ __forceinline__ bool gsr_ldlt6_factor(const double (&A)[6][6], double (&L)[6][6], double (&D)[6]) {
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
    if (!(fabs(d) < (double)KNN_INF) || !(d > GSR_ICP_PIVOT_MIN * A[j][j])) return false;
    D[j] = d;
    L[j][j] = 1.0;
    for (int i = j + 1; i < 6; i++) {
      double v = A[i][j];
      for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
  return true;
}
// L D L^T x = g
__device__ __forceinline__ void gsr_ldlt6_solve(const double (&L)[6][6], const double (&D)[6], const double (&g)[6],
                                                double (&x)[6]) {
  for (int i = 0; i < 6; i++) {      // L y = g
    double v = g[i];
    for (int k = 0; k < i; k++) v -= L[i][k] * x[k];
    x[i] = v;
  }
  for (int i = 0; i < 6; i++) x[i] /= D[i];
  for (int i = 5; i >= 0; i--) {      // L^T x = y / D
    double v = x[i];
    for (int k = i + 1; k < 6; k++) v -= L[k][i] * x[k];
    x[i] = v;
  }
}
// dR = Rz(gamma) Ry(beta) Rx(alpha) from x[0..2] = (alpha, beta, gamma)
__device__ __forceinline__ void gsr_rotation6(const double (&x)[6], double (&R)[3][3]) {
  double sa, ca, sb, cb, sg, cg;
  sincos(x[0], &sa, &ca);
  sincos(x[1], &sb, &cb);
  sincos(x[2], &sg, &cg);
  R[0][0] = cb * cg; R[0][1] = sa * sb * cg - ca * sg; R[0][2] = ca * sb * cg + sa * sg;
  R[1][0] = cb * sg; R[1][1] = sa * sb * sg + ca * cg; R[1][2] = ca * sb * sg - sa * cg;
  R[2][0] = -sb;     R[2][1] = sa * cb;                R[2][2] = ca * cb;
}
// T <- [R, td] T, row 3 written as 0 0 0 1
__device__ __forceinline__ void gsr_rigid_left6(const double (&R)[3][3], const double (&td)[3], double* __restrict__ T_dev) {
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
}

// thread 0 of the final kernel: J^T J x = -J^T r on the matrix in A and the right-hand side in g, both filled by the caller; then
// dR, dT and T <- dT T.  stats[3] = 0, or 2 with T as it was.  The arrays are LDS: indexed at run time, which registers cannot
// be.  `shift`: the point dT is formed about (three zeros: about the origin).
__device__ __forceinline__ void icp_solve6_compose(double (&A)[6][6], double (&L)[6][6], double (&D)[6], double (&g)[6],
                                                   double (&x)[6], const double* __restrict__ shift, double* __restrict__ T_dev,
                                                   double* __restrict__ stats) {
  if (!gsr_ldlt6_factor(A, L, D)) {
    stats[3] = 2.0;      // the correspondences do not fix this unknown (one plane, or sums that overflowed): T stays
    return;
  }
  gsr_ldlt6_solve(L, D, g, x);
  double ok = 0.0;
  for (int i = 0; i < 6; i++) ok += x[i];
  if (!(fabs(ok) < (double)KNN_INF)) {
    stats[3] = 2.0;
    return;
  }
  double R[3][3];
  gsr_rotation6(x, R);
  // dT y = dR (y - c) + t + c
  double td[3];
#pragma unroll
  for (int a = 0; a < 3; a++)
    td[a] = (x[3 + a] + shift[a]) - ((R[a][0] * shift[0] + R[a][1] * shift[1]) + R[a][2] * shift[2]);
  gsr_rigid_left6(R, td, T_dev);
  stats[3] = 0.0;
}

// one workgroup: the `nblk` rows of partial sums, then thread 0 writes the stats, solves and composes.  H: the header sums of a
// row (3: plane and odometry, 4: coloured).  denom: what fitness = n / denom is taken over (source rows, pixels).  shift: the
// point the unknowns are formed about, NULL = the origin (camera coordinates).  T_dev is written only with status 0 and `apply`:
// status 1 (n < 6), status 2 (a rejected pivot) and apply = 0 leave it bit for bit.  (static: each file launches its own copy)
template <int H>
static __global__ __launch_bounds__(256) void k_gn6_final(uint32_t nblk, double denom, int apply, const double* __restrict__ part,
                                                          const double* __restrict__ shift, double* __restrict__ T_dev,
                                                          double* __restrict__ stats) {
  // thread 0 only: indexed at run time, which registers cannot be.  Tn: the copy the step is composed into
  __shared__ double A[6][6], L[6][6], D[6], g[6], x[6], c[3], Tn[16];
  double s[H + GSR_GN6_TERMS];
  gsr_block_sum_rows(s, part, nblk);
  if (threadIdx.x != 0) return;
  gn_stats_header<H>(s, denom, stats);
  if (s[0] < 6.0) {
    stats[3] = 1.0;      // fewer rows than unknowns: T stays
    return;
  }
  {
    int o = H + 6;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      g[a] = -s[H + a];
#pragma unroll
      for (int b = a; b < 6; b++) {
        A[a][b] = A[b][a] = s[o];
        o++;
      }
    }
  }
  for (int a = 0; a < 3; a++) c[a] = shift ? shift[a] : 0.0;
  for (int i = 0; i < 16; i++) Tn[i] = T_dev[i];
  icp_solve6_compose(A, L, D, g, x, c, Tn, stats);      // (sets stats[3])
  if (apply && stats[3] == 0.0) {
    for (int i = 0; i < 16; i++) T_dev[i] = Tn[i];
  }
}
#endif
