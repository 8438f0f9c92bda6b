// icp_common.h - what every ICP update of include/gsr.h does alike, shared by registration.hip (gsr_icp_update, gsr_icp_update_plane,
// gsr_icp_update_colored) and gicp.hip (gsr_icp_update_generalized): ONE rule for which rows form a pair, ONE kernel for the shift
// c the sums are formed about, ONE host prelude (the workspace check, the grid of the partial kernel, the shift launch) - so the
// pairs, the shift and the workspace layout agree by construction.
#pragma once
#include "knn_common.h"
#include "rigid_common.h"
#include "solve6_common.h"

#ifdef __HIPCC__
// the pair of row i, or false: no correspondence, an index outside the target, a non-finite point on either side
__device__ __forceinline__ bool icp_pair(uint32_t i, const float* __restrict__ src, uint32_t Pt, const float* __restrict__ tgt,
                                         const int32_t* __restrict__ idx, const RegT& T, float4& q, float4& p) {
  const int32_t k = idx[i];
  if (k < 0 || (uint32_t)k >= Pt) return false;
  q = reg_apply(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]);
  p = make_float4(tgt[3 * (size_t)k], tgt[3 * (size_t)k + 1], tgt[3 * (size_t)k + 2], 0.f);
  return knn_finite(q.x) && knn_finite(q.y) && knn_finite(q.z) && knn_finite(p.x) && knn_finite(p.y) && knn_finite(p.z);
}

// one workgroup: the target point of the first valid row -> shift[0..2], shift[3] = 1 (no valid row: zeros).  (static: each file
// launches its own copy)
static __global__ __launch_bounds__(256) void k_icp_shift(uint32_t Ps, const float* __restrict__ src, uint32_t Pt,
                                                          const float* __restrict__ tgt, const int32_t* __restrict__ idx,
                                                          const double* __restrict__ T_dev, double* __restrict__ shift) {
  __shared__ uint32_t s_first;
  const RegT T = reg_load(T_dev);
  if (threadIdx.x == 0) s_first = 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t base = 0; base < Ps; base += 256u) {      // (uniform over the workgroup)
    const uint32_t i = base + threadIdx.x;
    float4 q, p;
    if (i < Ps && icp_pair(i, src, Pt, tgt, idx, T, q, p)) atomicMin(&s_first, i);      // (integer minimum: order-independent)
    __syncthreads();
    const uint32_t found = s_first;
    __syncthreads();      // (everybody has read it before the next round may lower it)
    if (found != 0xFFFFFFFFu) break;
  }
  if (threadIdx.x != 0) return;
  const uint32_t f = s_first;
  if (f == 0xFFFFFFFFu) {
    shift[0] = shift[1] = shift[2] = shift[3] = 0.0;
    return;
  }
  const size_t k = (size_t)idx[f];
  shift[0] = (double)tgt[3 * k];
  shift[1] = (double)tgt[3 * k + 1];
  shift[2] = (double)tgt[3 * k + 2];
  shift[3] = 1.0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct IcpRun {
  hipStream_t st;
  uint32_t ns, nt, sblk;
  double *shift, *part;
};
// after the entry's own argument check: the workspace check in the entry's name, the two parts of the workspace, the grid of the
// partial kernel, and the shift launch.  GSR_OK, or the error to return
static int icp_begin(const char* entry, int sums, int64_t Ps, const float* source, int64_t Pt, const float* target,
                     const int32_t* idx, const double* T_dev, void* workspace, size_t workspace_bytes, void* stream, IcpRun& r) {
  const GsrGnWs w = gn_ws(workspace, sums, true);
  if (!gsr_workspace_fits(entry, workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  r.st = (hipStream_t)stream;
  r.shift = w.shift;
  r.part = w.part;
  r.ns = (uint32_t)Ps;
  r.nt = (uint32_t)Pt;
  r.sblk = gn_partial_blocks(r.ns);
  GSR_LAUNCH("icp_shift", k_icp_shift, dim3(1), dim3(256), 0, r.st, r.ns, source, r.nt, target, idx, T_dev, r.shift);
  return GSR_OK;
}
#endif
