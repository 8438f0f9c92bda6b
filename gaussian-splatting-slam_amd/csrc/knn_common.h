// knn_common.h - what the exact neighbour searches share (knn.hip, normals.hip, features.hip: a cloud against itself;
// registration.hip: one cloud against another): the sizes of the two-level box structure, the host call that builds it over a
// cloud, the one rounding sequence of every squared distance, the Morton cell of a coordinate, and THE sweep over the structure
// (knn_sweep, with the top-K bound and the member walk built on it) that every search kernel calls.
#pragma once

#include "gsr_common.h"

#define GSR_KNN_BOX 64
#define GSR_KNN_SUPER 64
#define GSR_NONE 0x7FFFFFFFu       // no row (yet): above every row (P <= 2^30 - 1)

static inline size_t knn_nbox(size_t P) { return (P + GSR_KNN_BOX - 1) / GSR_KNN_BOX; }
static inline size_t knn_nsuper(size_t P) { return (knn_nbox(P) + GSR_KNN_SUPER - 1) / GSR_KNN_SUPER; }

// One structure in ONE caller-owned blob (registration.hip: the target's index; normals.hip: the workspace; the head of the
// workspaces of knn.hip, colored.hip and features.hip), and the only description of that blob: what a search reads first - the
// bounding box, the points in Morton order (xyz, bits of the original row), the AABBs of the 64-point boxes and the 64-box
// super-boxes - then the build's scratch: the box partials, the Morton sort's ping-pong keys / values and its tables.
struct GsrNnWs {
  float* bbox;                  // float[8] min xyz, max xyz; double[3] centre at + 64 bytes
  float4* pts;                  // float4[P]
  float4 *box_lo, *box_hi;      // float4[knn_nbox(P)]
  float4 *sup_lo, *sup_hi;      // float4[knn_nsuper(P)]
  size_t keep;                  // bytes from the blob's start that a search reads; behind them the build's scratch
  float* bbox_part;             // float[GSR_KNN_BBOX_PART]
  uint32_t* key[2];             // u32[P] each
  uint32_t* val[2];             // u32[P] each
  uint32_t* radix_tmp;          // gsr_radix_tmp_elems(P) words
};
// carves the structure of P points at the carver's position (a workspace that holds more goes on carving behind it)
static inline GsrNnWs nn_carve(GsrCarve& c, size_t P) {
  GsrNnWs w;
  if (P == 0) P = 1;
  const size_t start = c.o;
  w.bbox = c.take<float>(64);
  w.pts = c.take<float4>(P);
  w.box_lo = c.take<float4>(knn_nbox(P));
  w.box_hi = c.take<float4>(knn_nbox(P));
  w.sup_lo = c.take<float4>(knn_nsuper(P));
  w.sup_hi = c.take<float4>(knn_nsuper(P));
  w.keep = c.o - start;
  w.bbox_part = c.take<float>(GSR_KNN_BBOX_PART);
  for (int i = 0; i < 2; i++) w.key[i] = c.take<uint32_t>(P);
  for (int i = 0; i < 2; i++) w.val[i] = c.take<uint32_t>(P);
  w.radix_tmp = c.take<uint32_t>(gsr_radix_tmp_elems(P));
  return w;
}
// a blob that holds the structure and nothing else
struct GsrNnBlob { GsrNnWs nn; size_t total; };
static inline GsrNnBlob nn_ws(const void* blob, size_t P) {
  GsrCarve c(blob);
  GsrNnBlob w;
  w.nn = nn_carve(c, P);
  w.total = c.o;
  return w;
}
// knn.hip: bounding box, 30-bit Morton codes, the stable sort, boxes, super-boxes - the launches every search starts with.
// qflag (or NULL): u32[P], 1 at the sorted positions whose original row is >= first_query
void gsr_knn_build(int64_t P, const float* points, const GsrNnWs& b, hipStream_t st, uint32_t first_query = 0u,
                   uint32_t* qflag = nullptr);

// what a search kernel reads of a built structure, passed to it by value
struct GsrKnnTree {
  const float4 *pts, *box_lo, *box_hi, *sup_lo, *sup_hi;
  uint32_t P, nbox, nsuper;
};
static inline GsrKnnTree knn_tree(const GsrNnWs& b, size_t P) {
  return GsrKnnTree{b.pts, b.box_lo, b.box_hi, b.sup_lo, b.sup_hi, (uint32_t)P, (uint32_t)knn_nbox(P), (uint32_t)knn_nsuper(P)};
}
// the smallest compile-time list size K in {4, 8, 16, 32} that holds k (<= GSR_KNN_K_MAX) neighbours: runs LAUNCH(K)
#define GSR_KNN_PICK_K(k, LAUNCH) \
  do {                            \
    if ((k) <= 4) LAUNCH(4);      \
    else if ((k) <= 8) LAUNCH(8); \
    else if ((k) <= 16) LAUNCH(16); \
    else LAUNCH(32);              \
  } while (0)

#ifdef __HIPCC__
// (KNN_INF, knn_finite: gsr_common.h)
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

// the one rounding sequence of every squared distance, point or box (the pruning of knn_sweep below relies on it)
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

// ---- the sweep ------------------------------------------------------------------------------------------------------------------
// One thread per query `me`: all super-box AABBs staged through the caller's s_lo / s_hi (STAGE entries each; STAGE = the
// workgroup's size, whose every thread calls this - two barriers per round), then the 64 boxes of a super-box and the 64 points
// of a box, descending only where the AABB distance does not exceed radius(); visit(j, pts[j]) sees every point of a surviving box,
// in sorted order.  radius() is evaluated again at every box test, so a visit that lowers it prunes from the next box on.
// The structure only prunes.  A box is skipped when its AABB distance is GREATER than the radius - `!(d <= r)`, never `d < r`: a
// tie is entered - and that distance is formed with the same rounding sequence as a point distance (differences, then
// fma(dz,dz, fma(dy,dy, dx*dx))): rounding is monotone, so the fp32 AABB distance never exceeds the fp32 distance of a point
// inside - no point within the radius can be lost to rounding.  What a query answers is therefore a function of a multiset that
// does not depend on the traversal.  A NaN distance (a non-finite `me`, an all-NaN box) fails `<=`: skipped.
// The caller owns the LDS: two sweeps of one kernel share one allocation.  The callables capture per-thread lists and sums by
// reference; everything is inlined, so those stay in registers.
template <int STAGE, typename Radius, typename Visit>
__device__ __forceinline__ void knn_sweep(const GsrKnnTree& t, const float4 me, const bool active, float4* __restrict__ s_lo,
                                          float4* __restrict__ s_hi, Radius radius, Visit visit) {
  for (uint32_t base = 0; base < t.nsuper; base += (uint32_t)STAGE) {
    __syncthreads();
    if (base + threadIdx.x < t.nsuper) {
      s_lo[threadIdx.x] = t.sup_lo[base + threadIdx.x];
      s_hi[threadIdx.x] = t.sup_hi[base + threadIdx.x];
    }
    __syncthreads();
    if (!active) continue;
    const uint32_t n = min((uint32_t)STAGE, t.nsuper - base);
    for (uint32_t s = 0; s < n; s++) {
      if (!(knn_box_d2(me, s_lo[s], s_hi[s]) <= radius())) continue;
      const uint32_t bb = (base + s) * (uint32_t)GSR_KNN_SUPER, be = min(t.nbox, bb + (uint32_t)GSR_KNN_SUPER);
      for (uint32_t b = bb; b < be; b++) {
        if (!(knn_box_d2(me, t.box_lo[b], t.box_hi[b]) <= radius())) continue;
        const uint32_t jb = b * (uint32_t)GSR_KNN_BOX, je = min(t.P, jb + (uint32_t)GSR_KNN_BOX);
        for (uint32_t j = jb; j < je; j++) visit(j, t.pts[j]);
      }
    }
  }
}

// The top-K bound of the row at sorted position `pos` (me = pts[pos]): on return b holds the k smallest d2 to the OTHER rows that
// are <= cut, ascending behind K - k slots of -inf, and the value is min(d_k, cut), d_k the k-th smallest d2 (+inf with fewer than
// k other finite rows).  The 2k neighbours in Morton order seed an upper bound of d_k; the sweep starts from an empty list again,
// so no candidate is counted twice, and prunes at min(list[K - 1], seed, cut): with d_k <= cut all k smallest values lie below
// the cut and are seen; otherwise the last slot ends above the cut or at +inf, and the minimum is the cut either way.
template <int K, int STAGE>
__device__ __forceinline__ float knn_topk_bound(const GsrKnnTree& t, const float4 me, const uint32_t pos, const bool active,
                                                const int k, const float cut, float4* __restrict__ s_lo,
                                                float4* __restrict__ s_hi, float (&b)[K]) {
  const int pad = K - k;
  knn_reset_k<K>(b, pad);
  if (active) {
    const uint32_t kk = (uint32_t)k;
    const uint32_t j0 = pos >= kk ? pos - kk : 0u, j1 = min(t.P - 1u, pos + kk);
    for (uint32_t j = j0; j <= j1; j++)
      if (j != pos) knn_insert_k<K>(knn_point_d2(me, t.pts[j]), b);
  }
  const float seed = fminf(b[K - 1], cut);
  knn_reset_k<K>(b, pad);
  knn_sweep<STAGE>(
      t, me, active, s_lo, s_hi, [&]() __attribute__((always_inline)) { return fminf(b[K - 1], seed); },
      [&](const uint32_t j, const float4 p) __attribute__((always_inline)) {
        if (j != pos) knn_insert_k<K>(knn_point_d2(me, p), b);
      });
  return fminf(b[K - 1], cut);
}

// The members of the row at sorted position `pos`: every j != pos with d2(pos, j) <= bound (rows tied at the bound all are; a NaN
// is none), in sorted order; body(j, fx, fy, fz) sees the float32 differences p_pos - p_j
template <int STAGE, typename Body>
__device__ __forceinline__ void knn_member_walk(const GsrKnnTree& t, const float4 me, const uint32_t pos, const bool active,
                                                const float bound, float4* __restrict__ s_lo, float4* __restrict__ s_hi,
                                                Body body) {
  knn_sweep<STAGE>(
      t, me, active, s_lo, s_hi, [&]() __attribute__((always_inline)) { return bound; },
      [&](const uint32_t j, const float4 p) __attribute__((always_inline)) {
        const float fx = __fsub_rn(me.x, p.x), fy = __fsub_rn(me.y, p.y), fz = __fsub_rn(me.z, p.z);
        if (j == pos || !(knn_sq(fx, fy, fz) <= bound)) return;
        body(j, fx, fy, fz);
      });
}
#endif
