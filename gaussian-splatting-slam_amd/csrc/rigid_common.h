// rigid_common.h - "q = T s" of include/gsr.h, shared by registration.hip (nearest-neighbour queries, gsr_transform_points, the ICP
// updates) and pointcloud2.hip (the pose a decoded PointCloud2 row is moved by): ONE body, so the bits agree by construction.
#pragma once

#ifdef __HIPCC__
// ---- q = (float)(R s + t) -----------------------------------------------------------------------------------------------------
struct RegT {
  double m[12];      // rows 0 .. 2 of the row-major 4 x 4
};
__device__ __forceinline__ RegT reg_load(const double* __restrict__ T) {
  RegT r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.m[i] = T ? T[i] : ((i % 5) == 0 ? 1.0 : 0.0);
  return r;
}
// component i = (float)(((T[i,0] x + T[i,1] y) + T[i,2] z) + T[i,3]): three products and three sums, each rounded to float64 on
// its own (no fused multiply-add), in this order, then ONE rounding to float32.  .w = 0.
__device__ __forceinline__ float4 reg_apply(const RegT& T, float x, float y, float z) {
  float q[3];
  const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double a = __dadd_rn(__dmul_rn(T.m[4 * i], dx), __dmul_rn(T.m[4 * i + 1], dy));
    q[i] = (float)__dadd_rn(__dadd_rn(a, __dmul_rn(T.m[4 * i + 2], dz)), T.m[4 * i + 3]);
  }
  return make_float4(q[0], q[1], q[2], 0.f);
}
#endif
