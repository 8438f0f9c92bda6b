// jacobi3_common.h - the cyclic Jacobi step on a symmetric 3 x 3 in float64, shared by normals.hip (gsr_estimate_normals) and
// gicp.hip (gsr_estimate_covariances, gsr_regularize_covariances): ONE rotation body and ONE sweep count, so the eigenvector a
// covariance is regularised about is the one the normal is taken from.
#pragma once

#define GSR_NORMALS_SWEEPS 8      // cyclic Jacobi on a 3 x 3 symmetric matrix: quadratic once the off-diagonal is small; 5 - 6 reach 1e-16

#ifdef __HIPCC__
// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3: app, aqq, apq the plane's entries, akp / akq the two entries that
// couple the third index k to it, (v0p, v0q) .. (v2p, v2q) the rows of the eigenvector matrix's columns p and q
__device__ __forceinline__ void normals_rotate(double& app, double& aqq, double& apq, double& akp, double& akq, double& v0p,
                                               double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double kp = akp, kq = akq;
  akp = c * kp - s * kq;
  akq = s * kp + c * kq;
  double a, b;
  a = v0p; b = v0q; v0p = c * a - s * b; v0q = s * a + c * b;
  a = v1p; b = v1q; v1p = c * a - s * b; v1q = s * a + c * b;
  a = v2p; b = v2q; v2p = c * a - s * b; v2q = s * a + c * b;
}
#endif
