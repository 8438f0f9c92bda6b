// Per-view exposure on the device (include/gsr.h, gsr_exposure_forward / gsr_exposure_backward): the `use_trained_exp` branch of
// reference gaussian_renderer/__init__.py:141-144 and the alpha-mask multiply of train.py:109-111 as ONE elementwise launch, and
// their backward as one streaming launch plus a one-workgroup finalize that may also take the exposure optimizer's step.
//
//   out[j,p] = m[p] ( sum_k E[k][j] I[k,p] + E[j][3] )          E [3,4] row-major, I [3,n] planar, m [n] or absent (= 1)
//
// The 3x3 part acts TRANSPOSED on the pixel (the reference multiplies the pixel row vector from the right) while the bias of
// channel j is column 3 of ROW j: the reference's convention, kept as it is.
//
// Memory-bound streaming kernels (28 B in / 12 B out per pixel forward, 40 B in / 12 B out backward): 16-B accesses per lane when
// every plane base is 16-byte aligned (n % 4 == 0 and aligned tensors), 4-B accesses otherwise - planes 1 and 2 of a contiguous
// [3,H,W] tensor with an odd H W sit at odd word offsets.  E is twelve wave-uniform loads from device memory: nothing is read back
// by the host.  The twelve exposure gradients are summed per thread, per wave (shuffles), per workgroup (LDS), written as one row
// of partials per workgroup and added by ONE workgroup in index order: no float atomics, the same bits every run.
#include "gsr_common.h"

#define EXP_BLOCKS 1024      // most workgroups of the streaming launches = rows of the partials scratch
#define EXP_THREADS 256
#define EXP_FIN_THREADS 768  // finalize: twelve waves, one per exposure entry

namespace {

struct Exposure {
  float e[12];
};

__device__ __forceinline__ Exposure load_exposure(const float* __restrict__ E) {
  Exposure x;
#pragma unroll
  for (int i = 0; i < 12; i++) x.e[i] = E[i];
  return x;
}

// one pixel forward: o[j] = m (E[0][j] a + E[1][j] b + E[2][j] c + E[j][3])
__device__ __forceinline__ void exposure_px(const Exposure& x, float a, float b, float c, float m, float& o0, float& o1, float& o2) {
  o0 = m * (x.e[0] * a + x.e[4] * b + x.e[8] * c + x.e[3]);
  o1 = m * (x.e[1] * a + x.e[5] * b + x.e[9] * c + x.e[7]);
  o2 = m * (x.e[2] * a + x.e[6] * b + x.e[10] * c + x.e[11]);
}

template <bool VEC>
__global__ __launch_bounds__(EXP_THREADS) void k_exposure_fwd(const float* __restrict__ img, const float* __restrict__ E,
                                                              const float* __restrict__ mask, long long n,
                                                              float* __restrict__ out) {
  const Exposure x = load_exposure(E);
  const long long stride = (long long)gridDim.x * EXP_THREADS;
  const long long t0 = (long long)blockIdx.x * EXP_THREADS + threadIdx.x;
  if (VEC) {
    const long long n4 = n >> 2;      // (n % 4 == 0 on this path)
    for (long long q = t0; q < n4; q += stride) {
      const long long p = q << 2;
      const gsr_f4 a = gsr_ld_stream(img + p), b = gsr_ld_stream(img + n + p), c = gsr_ld_stream(img + 2 * n + p);
      const gsr_f4 m = mask ? gsr_ld_stream(mask + p) : gsr_f4{1.f, 1.f, 1.f, 1.f};
      float o0[4], o1[4], o2[4];
#pragma unroll
      for (int i = 0; i < 4; i++) exposure_px(x, a[i], b[i], c[i], m[i], o0[i], o1[i], o2[i]);
      *reinterpret_cast<gsr_f4*>(out + p) = gsr_f4{o0[0], o0[1], o0[2], o0[3]};
      *reinterpret_cast<gsr_f4*>(out + n + p) = gsr_f4{o1[0], o1[1], o1[2], o1[3]};
      *reinterpret_cast<gsr_f4*>(out + 2 * n + p) = gsr_f4{o2[0], o2[1], o2[2], o2[3]};
    }
  } else {
    for (long long p = t0; p < n; p += stride) {
      float o0, o1, o2;
      exposure_px(x, img[p], img[n + p], img[2 * n + p], mask ? mask[p] : 1.f, o0, o1, o2);
      out[p] = o0;
      out[n + p] = o1;
      out[2 * n + p] = o2;
    }
  }
}

// one pixel backward: d[k] = m sum_j E[k][j] g[j] (when asked for); acc[4 k + j] += m I[k] g[j], acc[4 j + 3] += m g[j]
template <bool WANT_I, bool WANT_E>
__device__ __forceinline__ void exposure_px_bwd(const Exposure& x, float a, float b, float c, float m, float g0, float g1,
                                                float g2, float& d0, float& d1, float& d2, float* acc) {
  if (WANT_I) {
    d0 = m * (x.e[0] * g0 + x.e[1] * g1 + x.e[2] * g2);
    d1 = m * (x.e[4] * g0 + x.e[5] * g1 + x.e[6] * g2);
    d2 = m * (x.e[8] * g0 + x.e[9] * g1 + x.e[10] * g2);
  }
  if (WANT_E) {
    const float m0 = m * g0, m1 = m * g1, m2 = m * g2;
    acc[0] += a * m0; acc[1] += a * m1; acc[2] += a * m2;  acc[3] += m0;
    acc[4] += b * m0; acc[5] += b * m1; acc[6] += b * m2;  acc[7] += m1;
    acc[8] += c * m0; acc[9] += c * m1; acc[10] += c * m2; acc[11] += m2;
  }
}

// partials: [gridDim.x][12] - every workgroup of the launch writes its row
template <bool VEC, bool WANT_I, bool WANT_E>
__global__ __launch_bounds__(EXP_THREADS) void k_exposure_bwd(const float* __restrict__ img, const float* __restrict__ E,
                                                              const float* __restrict__ mask, const float* __restrict__ g,
                                                              long long n, float* __restrict__ dimg,
                                                              float* __restrict__ partials) {
  const Exposure x = load_exposure(E);
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; i++) acc[i] = 0.f;
  const long long stride = (long long)gridDim.x * EXP_THREADS;
  const long long t0 = (long long)blockIdx.x * EXP_THREADS + threadIdx.x;
  if (VEC) {
    const long long n4 = n >> 2;
    for (long long q = t0; q < n4; q += stride) {
      const long long p = q << 2;
      gsr_f4 a = {0.f, 0.f, 0.f, 0.f}, b = a, c = a;
      if (WANT_E) {
        a = gsr_ld_stream(img + p);
        b = gsr_ld_stream(img + n + p);
        c = gsr_ld_stream(img + 2 * n + p);
      }
      const gsr_f4 g0 = gsr_ld_stream(g + p), g1 = gsr_ld_stream(g + n + p), g2 = gsr_ld_stream(g + 2 * n + p);
      const gsr_f4 m = mask ? gsr_ld_stream(mask + p) : gsr_f4{1.f, 1.f, 1.f, 1.f};
      float d0[4], d1[4], d2[4];
#pragma unroll
      for (int i = 0; i < 4; i++)
        exposure_px_bwd<WANT_I, WANT_E>(x, a[i], b[i], c[i], m[i], g0[i], g1[i], g2[i], d0[i], d1[i], d2[i], acc);
      if (WANT_I) {
        *reinterpret_cast<gsr_f4*>(dimg + p) = gsr_f4{d0[0], d0[1], d0[2], d0[3]};
        *reinterpret_cast<gsr_f4*>(dimg + n + p) = gsr_f4{d1[0], d1[1], d1[2], d1[3]};
        *reinterpret_cast<gsr_f4*>(dimg + 2 * n + p) = gsr_f4{d2[0], d2[1], d2[2], d2[3]};
      }
    }
  } else {
    for (long long p = t0; p < n; p += stride) {
      float a = 0.f, b = 0.f, c = 0.f, d0, d1, d2;
      if (WANT_E) {
        a = img[p];
        b = img[n + p];
        c = img[2 * n + p];
      }
      exposure_px_bwd<WANT_I, WANT_E>(x, a, b, c, mask ? mask[p] : 1.f, g[p], g[n + p], g[2 * n + p], d0, d1, d2, acc);
      if (WANT_I) {
        dimg[p] = d0;
        dimg[n + p] = d1;
        dimg[2 * n + p] = d2;
      }
    }
  }
  if (!WANT_E) return;
  // thread -> wave (shuffles) -> workgroup (LDS), every step in a fixed order
  __shared__ float red[EXP_THREADS / 64][12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    float v = acc[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    acc[i] = v;
  }
  const int lane = gsr_lane(), wave = (int)threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; i++) red[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < EXP_THREADS / 64; w++) s += red[w][threadIdx.x];
    partials[(size_t)blockIdx.x * 12 + threadIdx.x] = s;
  }
}

// Wave c adds entry c of the nblk rows of partials: lane l takes rows l, l + 64, ... in order, then the wave's shuffle tree.
// dE (optional) receives the twelve sums.  With an Adam state (device memory: the header, then exp_avg and exp_avg_sq of all
// `views` rows) the launch then applies one torch.optim.Adam step to the WHOLE [views,3,4] tensor with the gradient = the sums on
// row `row` and zero on every other row - rows seen earlier keep moving on their decaying moments, as under a dense optimizer.
// The bias corrections come from the stored step count in float64, the element update is adam_elem<1> (gsr_common.h).
__global__ __launch_bounds__(EXP_FIN_THREADS) void k_exposure_finalize(const float* __restrict__ partials, int nblk,
                                                                       float* __restrict__ dE, float* __restrict__ exposures,
                                                                       int views, int row, gsr_exposure_adam* adam, double lr,
                                                                       double beta1, double beta2, double eps) {
  __shared__ float sums[12];
  const int lane = gsr_lane(), c = (int)threadIdx.x >> 6;
  float s = 0.f;
  for (int r = lane; r < nblk; r += 64) s += partials[(size_t)r * 12 + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    sums[c] = s;
    if (dE) dE[c] = s;
  }
  if (!adam) return;
  const int64_t step = adam->step;      // (read by every thread before the barrier, written by thread 0 behind it)
  __syncthreads();
  const double t = (double)(step + 1);
  GsrAdamArgs A;
  A.beta1 = (float)beta1;
  A.beta2 = (float)beta2;
  A.omb1 = (float)(1.0 - beta1);
  A.omb2 = (float)(1.0 - beta2);
  A.eps = (float)eps;
  A.lr[0] = (float)lr;
  A.step_size[0] = (float)(lr / (1.0 - pow(beta1, t)));
  A.inv_bc2_sqrt[0] = (float)(1.0 / sqrt(1.0 - pow(beta2, t)));
  float* m_all = reinterpret_cast<float*>(adam + 1);
  float* v_all = m_all + (size_t)views * 12;
  for (int i = (int)threadIdx.x; i < views * 12; i += EXP_FIN_THREADS) {
    const float g = (i / 12 == row) ? sums[i % 12] : 0.f;
    float p = exposures[i], m = m_all[i], v = v_all[i];
    adam_elem<1>(p, m, v, g, A, 0);
    exposures[i] = p;
    m_all[i] = m;
    v_all[i] = v;
  }
  if (threadIdx.x == 0) adam->step = step + 1;
}

inline int exposure_grid(long long items) {
  const long long b = (items + EXP_THREADS - 1) / EXP_THREADS;
  return (int)(b < 1 ? 1 : (b > EXP_BLOCKS ? EXP_BLOCKS : b));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int32_t gsr_exposure_blocks(void) { return EXP_BLOCKS; }

extern "C" int gsr_exposure_forward(int64_t n, const float* image, const float* exposure, const float* mask, float* out,
                                    void* stream) {
  if (n <= 0 || !image || !exposure || !out) {
    gsr_set_error("exposure_forward: bad arguments");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (n & 3) == 0 && aligned16(image) && aligned16(out) && aligned16(mask);
  if (vec)
    GSR_LAUNCH("exposure_fwd", k_exposure_fwd<true>, dim3(exposure_grid(n >> 2)), dim3(EXP_THREADS), 0, st, image, exposure, mask,
               (long long)n, out);
  else
    GSR_LAUNCH("exposure_fwd", k_exposure_fwd<false>, dim3(exposure_grid(n)), dim3(EXP_THREADS), 0, st, image, exposure, mask,
               (long long)n, out);
  return gsr_launch_status("exposure forward launch");
}

template <bool VEC>
static void launch_exposure_bwd(int grid, hipStream_t st, const float* image, const float* exposure, const float* mask,
                                const float* g, long long n, float* dimg, float* partials, bool want_e) {
  if (dimg && want_e)
    GSR_LAUNCH("exposure_bwd", (k_exposure_bwd<VEC, true, true>), dim3(grid), dim3(EXP_THREADS), 0, st, image, exposure, mask, g,
               n, dimg, partials);
  else if (dimg)
    GSR_LAUNCH("exposure_bwd", (k_exposure_bwd<VEC, true, false>), dim3(grid), dim3(EXP_THREADS), 0, st, image, exposure, mask, g,
               n, dimg, partials);
  else
    GSR_LAUNCH("exposure_bwd", (k_exposure_bwd<VEC, false, true>), dim3(grid), dim3(EXP_THREADS), 0, st, image, exposure, mask, g,
               n, dimg, partials);
}

extern "C" int gsr_exposure_backward(int64_t n, const float* image, const float* exposure, const float* mask,
                                     const float* dL_dout, float* dL_dimage, float* partials, float* dL_dexposure,
                                     float* exposures, int32_t views, int32_t row, gsr_exposure_adam* adam, double lr,
                                     double beta1, double beta2, double eps, void* stream) {
  const bool want_e = dL_dexposure != nullptr || adam != nullptr;
  if (n <= 0 || !image || !exposure || !dL_dout || (want_e && !partials)) {
    gsr_set_error("exposure_backward: bad arguments");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (adam && (!exposures || views <= 0 || row < 0 || row >= views || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) ||
               !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))) {
    gsr_set_error("exposure_backward: an Adam state needs the [views,3,4] tensor, 0 <= row < views, lr >= 0, betas in [0, 1), "
                  "eps >= 0");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!dL_dimage && !want_e) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (n & 3) == 0 && aligned16(image) && aligned16(dL_dout) && aligned16(mask) && aligned16(dL_dimage);
  const int grid = exposure_grid(vec ? (n >> 2) : n);
  if (vec)
    launch_exposure_bwd<true>(grid, st, image, exposure, mask, dL_dout, (long long)n, dL_dimage, partials, want_e);
  else
    launch_exposure_bwd<false>(grid, st, image, exposure, mask, dL_dout, (long long)n, dL_dimage, partials, want_e);
  if (want_e)
    GSR_LAUNCH("exposure_finalize", k_exposure_finalize, dim3(1), dim3(EXP_FIN_THREADS), 0, st, (const float*)partials, grid,
               dL_dexposure, exposures, (int)views, (int)row, adam, lr, beta1, beta2, eps);
  return gsr_launch_status("exposure backward launch");
}
