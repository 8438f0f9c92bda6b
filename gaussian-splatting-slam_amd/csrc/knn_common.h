// knn_common.h - what the exact neighbour searches share (knn.hip: a cloud against itself; registration.hip: one cloud against
// another): the sizes of the two-level box structure, the one rounding sequence of every squared distance, the Morton cell of a
// coordinate, and the host call that builds the structure over a cloud.
#pragma once

#include "gsr_common.h"

#define GSR_KNN_BOX 64
#define GSR_KNN_SUPER 64
#define GSR_KNN_BBOX_BLOCKS 1024

static inline size_t knn_nbox(size_t P) { return (P + GSR_KNN_BOX - 1) / GSR_KNN_BOX; }
static inline size_t knn_nsuper(size_t P) { return (knn_nbox(P) + GSR_KNN_SUPER - 1) / GSR_KNN_SUPER; }

// The buffers of one structure: bounding box, Morton sort (ping-pong keys / values, the sort's scratch), the points in sorted order
// (xyz, bits of the original row) and the AABBs of the 64-point boxes and the 64-box super-boxes.
struct GsrKnnBuild {
  float* bbox_part;      // gsr_knn_bbox_part_bytes()
  float* bbox;           // float[8]: min xyz, max xyz
  uint32_t* key[2];      // u32[P] each
  uint32_t* val[2];      // u32[P] each
  uint32_t* radix_tmp;   // gsr_radix_tmp_elems(P) words
  float4* pts;           // float4[P]
  float4 *box_lo, *box_hi;   // float4[knn_nbox(P)]
  float4 *sup_lo, *sup_hi;   // float4[knn_nsuper(P)]
};
// knn.hip: bounding box, 30-bit Morton codes, the stable sort, boxes, super-boxes - the launches gsr_knn_k starts with
void gsr_knn_build(int64_t P, const float* points, const GsrKnnBuild& b, hipStream_t st);

#ifdef __HIPCC__
#define KNN_INF __builtin_huge_valf()

__device__ __forceinline__ bool knn_finite(float x) { return fabsf(x) < KNN_INF; }   // false for NaN and +-inf

__device__ __forceinline__ float knn_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float knn_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ uint32_t knn_spread10(uint32_t x) {      // 10 bits -> every third bit of 30
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}
// (v - lo) / (hi - lo) on a 1024-cell axis; NaN (a flat axis: 0 / 0, a non-finite coordinate) and negatives give cell 0
__device__ __forceinline__ uint32_t knn_cell(float v, float lo, float hi) {
  const float t = (v - lo) / (hi - lo) * 1023.0f;
  return t >= 0.f ? (uint32_t)fminf(t, 1023.0f) : 0u;
}
// 30-bit Morton code of a point in the box bbox[0..2] .. bbox[3..5] (points outside it land in the cells of its faces)
__device__ __forceinline__ uint32_t knn_morton_code(float x, float y, float z, const float* __restrict__ bbox) {
  const uint32_t cx = knn_cell(x, bbox[0], bbox[3]);
  const uint32_t cy = knn_cell(y, bbox[1], bbox[4]);
  const uint32_t cz = knn_cell(z, bbox[2], bbox[5]);
  return knn_spread10(cx) | (knn_spread10(cy) << 1) | (knn_spread10(cz) << 2);
}

// the one rounding sequence of every squared distance, point or box (see the header of knn.hip: the pruning relies on it)
__device__ __forceinline__ float knn_sq(float dx, float dy, float dz) {
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __fmul_rn(dx, dx)));
}
__device__ __forceinline__ float knn_point_d2(const float4 q, const float4 p) {
  return knn_sq(__fsub_rn(q.x, p.x), __fsub_rn(q.y, p.y), __fsub_rn(q.z, p.z));
}
__device__ __forceinline__ float knn_box_d2(const float4 q, const float4 lo, const float4 hi) {
  // per axis max(q - hi, lo - q, 0) = |q - nearest point of the interval|; for a point p of the box |q - p| is at least that,
  // and stays so after rounding
  const float dx = fmaxf(0.f, fmaxf(__fsub_rn(q.x, hi.x), __fsub_rn(lo.x, q.x)));
  const float dy = fmaxf(0.f, fmaxf(__fsub_rn(q.y, hi.y), __fsub_rn(lo.y, q.y)));
  const float dz = fmaxf(0.f, fmaxf(__fsub_rn(q.z, hi.z), __fsub_rn(lo.z, q.z)));
  return knn_sq(dx, dy, dz);
}
#endif
