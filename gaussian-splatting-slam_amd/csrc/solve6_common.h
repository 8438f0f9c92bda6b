// solve6_common.h - the 6-unknown Gauss-Newton step of include/gsr.h, shared by registration.hip (gsr_icp_update_plane,
// gsr_icp_update_colored) and odometry.hip (gsr_odometry_update): ONE body for the LDL^T solve, the vector-to-matrix composition
// and T <- dT T, so the pivot rule and the order of operations agree by construction.
#pragma once

#define GSR_ICP_PIVOT_MIN 1e-12   // LDL^T: a pivot at or below this share of its diagonal entry is no pivot

#ifdef __HIPCC__
// thread 0 of a final kernel (the plane update's, the coloured one's and the odometry's): J^T J x = -J^T r on the matrix in A and
// the right-hand side in g, both filled by the caller; then dR, dT and T <- dT T.  stats[3] = 0, or 2 with T as it was.  The
// arrays are LDS: indexed at run time, which registers cannot be.  `shift`: the point dT is formed about (three zeros: about the
// origin).
__device__ __forceinline__ void icp_solve6_compose(double (&A)[6][6], double (&L)[6][6], double (&D)[6], double (&g)[6],
                                                   double (&x)[6], const double* __restrict__ shift, double* __restrict__ T_dev,
                                                   double* __restrict__ stats) {
  // J^T J = L D L^T, L unit lower triangular; every pivot is held against its own diagonal entry (scale-free per unknown)
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
    if (!(fabs(d) < (double)KNN_INF) || !(d > GSR_ICP_PIVOT_MIN * A[j][j])) {
      stats[3] = 2.0;      // the correspondences do not fix this unknown (one plane, or sums that overflowed): T stays
      return;
    }
    D[j] = d;
    L[j][j] = 1.0;
    for (int i = j + 1; i < 6; i++) {
      double v = A[i][j];
      for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
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
  double ok = 0.0;
  for (int i = 0; i < 6; i++) ok += x[i];
  if (!(fabs(ok) < (double)KNN_INF)) {
    stats[3] = 2.0;
    return;
  }
  // dR = Rz(gamma) Ry(beta) Rx(alpha)
  double sa, ca, sb, cb, sg, cg;
  sincos(x[0], &sa, &ca);
  sincos(x[1], &sb, &cb);
  sincos(x[2], &sg, &cg);
  double R[3][3];
  R[0][0] = cb * cg; R[0][1] = sa * sb * cg - ca * sg; R[0][2] = ca * sb * cg + sa * sg;
  R[1][0] = cb * sg; R[1][1] = sa * sb * sg + ca * cg; R[1][2] = ca * sb * sg - sa * cg;
  R[2][0] = -sb;     R[2][1] = sa * cb;                R[2][2] = ca * cb;
  // dT y = dR (y - c) + t + c
  double td[3];
#pragma unroll
  for (int a = 0; a < 3; a++)
    td[a] = (x[3 + a] + shift[a]) - ((R[a][0] * shift[0] + R[a][1] * shift[1]) + R[a][2] * shift[2]);
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
#endif
