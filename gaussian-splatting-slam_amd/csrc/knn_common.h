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

// ---- a structure kept in ONE caller-owned blob (registration.hip: the target's index; normals.hip: the workspace): what a search
// reads first, the build's scratch behind it ----
struct GsrNnLayout {
  size_t bbox;                  // float[8] min xyz, max xyz; double[3] centre at + 64
  size_t pts;                   // float4[P]
  size_t box_lo, box_hi;        // float4[nbox]
  size_t sup_lo, sup_hi;        // float4[nsuper]
  size_t keep;                  // what a search reads ends here; the rest is the build's scratch
  size_t bbox_part, key_a, key_b, val_a, val_b, radix_tmp;
  size_t total;
};
static inline GsrNnLayout nn_layout(size_t P) {
  GsrNnLayout L;
  size_t o = 0;
  if (P == 0) P = 1;
  L.bbox = o;      o += 256;
  L.pts = o;       o += gsr_align(P * 16);
  L.box_lo = o;    o += gsr_align(knn_nbox(P) * 16);
  L.box_hi = o;    o += gsr_align(knn_nbox(P) * 16);
  L.sup_lo = o;    o += gsr_align(knn_nsuper(P) * 16);
  L.sup_hi = o;    o += gsr_align(knn_nsuper(P) * 16);
  L.keep = o;
  L.bbox_part = o; o += gsr_knn_bbox_part_bytes();
  L.key_a = o;     o += gsr_align(P * 4);
  L.key_b = o;     o += gsr_align(P * 4);
  L.val_a = o;     o += gsr_align(P * 4);
  L.val_b = o;     o += gsr_align(P * 4);
  L.radix_tmp = o; o += gsr_align(gsr_radix_tmp_elems(P) * 4);
  L.total = o;
  return L;
}
// the buffers of gsr_knn_build inside a blob of that layout
static inline GsrKnnBuild nn_build_views(char* blob, const GsrNnLayout& L) {
  GsrKnnBuild b;
  b.bbox_part = (float*)(blob + L.bbox_part);
  b.bbox = (float*)(blob + L.bbox);
  b.key[0] = (uint32_t*)(blob + L.key_a); b.key[1] = (uint32_t*)(blob + L.key_b);
  b.val[0] = (uint32_t*)(blob + L.val_a); b.val[1] = (uint32_t*)(blob + L.val_b);
  b.radix_tmp = (uint32_t*)(blob + L.radix_tmp);
  b.pts = (float4*)(blob + L.pts);
  b.box_lo = (float4*)(blob + L.box_lo); b.box_hi = (float4*)(blob + L.box_hi);
  b.sup_lo = (float4*)(blob + L.sup_lo); b.sup_hi = (float4*)(blob + L.sup_hi);
  return b;
}

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

// a row with a non-finite coordinate as the blob structures store it: NaN NaN NaN, the original row kept in .w - every distance
// to it is NaN, which fails every comparison: nobody's neighbour
__device__ __forceinline__ float4 knn_mask_non_finite(const float4 p) {
  if (knn_finite(p.x) && knn_finite(p.y) && knn_finite(p.z)) return p;
  const float nan = __builtin_nanf("");
  return make_float4(nan, nan, nan, p.w);
}

// knn_insert over K slots, ascending: d bubbles up the chain, every index a compile-time constant (registers, no scratch)
template <int K>
__device__ __forceinline__ void knn_insert_k(float d, float (&b)[K]) {
  if (d < b[K - 1]) {      // (false for NaN)
    float t = d;
#pragma unroll
    for (int i = 0; i < K - 1; i++) {
      const float hi = fmaxf(b[i], t);
      b[i] = fminf(b[i], t);
      t = hi;
    }
    b[K - 1] = fminf(b[K - 1], t);
  }
}
template <int K>
__device__ __forceinline__ void knn_reset_k(float (&b)[K], int pad) {      // `pad` = K - k leading slots at -inf, the rest +inf
#pragma unroll
  for (int i = 0; i < K; i++) b[i] = i < pad ? -KNN_INF : KNN_INF;
}
#endif
