// horn_common.h - Horn's closed form (1987) for the rotation between two centred point sets, shared by the ICP update
// (registration.hip: k_icp_final, one thread per launch) and the hypothesis stage of the feature-matching RANSAC (features.hip:
// one thread per trial).  The rotation is the unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix built from
// the centred cross-covariance - a unit quaternion, so a reflection cannot come out - found by cyclic Jacobi with a fixed number
// of sweeps.  The Jacobi loops index the matrices at run time, which registers cannot be: the caller hands in where they live
// (LDS) through a small accessor type with `double& at(int i, int j)`.
#pragma once

#define GSR_ICP_SWEEPS 12          // cyclic Jacobi on a 4 x 4 symmetric matrix converges quadratically: 6 - 7 sweeps reach 1e-16

#ifdef __HIPCC__
// a plain [4][4] array (one solver per workgroup)
struct HornMat4 {
  double (*m)[4];
  __device__ __forceinline__ double& at(int i, int j) const { return m[i][j]; }
};
// one matrix per thread of a workgroup of STRIDE threads, element (i, j) of thread t at base[(4 i + j) STRIDE + t]: the lanes of
// a wave touch consecutive words
template <int STRIDE>
struct HornMat4Strided {
  double* base;      // already offset by the thread's index
  __device__ __forceinline__ double& at(int i, int j) const { return base[(4 * i + j) * STRIDE]; }
};

// M[a][b] = sum (q_a - qbar_a)(p_b - pbar_b) -> R (q -> p), the largest eigenvalue; false without a usable eigenvector (a NaN:
// sums that overflowed), R is then not written
template <class Mat>
__device__ __forceinline__ bool horn_rotation(const double (&M)[3][3], const Mat A, const Mat V, double (&R)[3][3], double& eig) {
  // Horn 1987: the quaternion (w, x, y, z) of the rotation that takes q to p maximises v^T N v
  A.at(0, 0) = M[0][0] + M[1][1] + M[2][2];
  A.at(1, 1) = M[0][0] - M[1][1] - M[2][2];
  A.at(2, 2) = -M[0][0] + M[1][1] - M[2][2];
  A.at(3, 3) = -M[0][0] - M[1][1] + M[2][2];
  A.at(0, 1) = A.at(1, 0) = M[1][2] - M[2][1];
  A.at(0, 2) = A.at(2, 0) = M[2][0] - M[0][2];
  A.at(0, 3) = A.at(3, 0) = M[0][1] - M[1][0];
  A.at(1, 2) = A.at(2, 1) = M[0][1] + M[1][0];
  A.at(1, 3) = A.at(3, 1) = M[2][0] + M[0][2];
  A.at(2, 3) = A.at(3, 2) = M[1][2] + M[2][1];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) V.at(i, j) = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < GSR_ICP_SWEEPS; sweep++) {
    for (int p = 0; p < 3; p++) {
      for (int q = p + 1; q < 4; q++) {
        const double apq = A.at(p, q);
        if (apq == 0.0) continue;
        const double theta = (A.at(q, q) - A.at(p, p)) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        A.at(p, p) -= t * apq;
        A.at(q, q) += t * apq;
        A.at(p, q) = A.at(q, p) = 0.0;
        for (int k = 0; k < 4; k++) {
          if (k != p && k != q) {
            const double akp = A.at(k, p), akq = A.at(k, q);
            A.at(k, p) = A.at(p, k) = c * akp - sn * akq;
            A.at(k, q) = A.at(q, k) = sn * akp + c * akq;
          }
          const double vkp = V.at(k, p), vkq = V.at(k, q);
          V.at(k, p) = c * vkp - sn * vkq;
          V.at(k, q) = sn * vkp + c * vkq;
        }
      }
    }
  }
  int best = 0;
  for (int k = 1; k < 4; k++)
    if (A.at(k, k) > A.at(best, best)) best = k;
  double w = V.at(0, best), x = V.at(1, best), y = V.at(2, best), z = V.at(3, best);
  const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
  eig = A.at(best, best);
  if (!(norm > 0.5 && norm < 2.0)) return false;      // (a NaN too: sums that overflowed)
  w /= norm; x /= norm; y /= norm; z /= norm;
  R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z);       R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);       R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);       R[2][1] = 2.0 * (y * z + w * x);       R[2][2] = 1.0 - 2.0 * (x * x + y * y);
  return true;
}
#endif
