// colored.hip - the per-point colour gradient of a coloured point cloud: what Open3D's registration_colored_icp prepares on the
// target (InitializePointCloudForColoredICP; Park, Zhou, Koltun 2017) before the joint geometric / photometric update of
// csrc/registration.hip (gsr_icp_update_colored) uses it.
//
// gsr_color_gradient: rows whose point, normal or colour has a non-finite component become NaN NaN NaN BEFORE the structure of
//   knn.hip (knn_common.h) is built over the cloud - they take no part in the bounding box, the sort or the boxes, every distance
//   to them is NaN and fails every comparison: nobody's neighbour.  Then ONE launch, one thread per row in Morton order, the two
//   sweeps of k_normals (normals.hip) over the same boxes and one LDS allocation:
//   1. the bound.  k = max_nn - 1; knn_topk_bound, cut at r2, gives min(r2, d_k).
//   2. the sums.  knn_member_walk: every row j != i with d2(i,j) <= bound is a member (rows tied at the bound all are).  delta =
//      p_j - p_i per component in float32, promoted; u = delta - (delta.n) n, the member's offset in the tangent plane of row i;
//      b = I_j - I_i, the member's colour gathered through its original row (the w of the sorted float4); u u^T (six sums) and u b
//      (three) in float64, in sorted-position order: fixed for a given input, so two runs give the same bits.
//   Then the constraint row (n_i - 1) n with right-hand side 0 (the gradient has no component along the normal), the 3 x 3
//   LDL^T in registers - every index a compile-time constant, no scratch - and one rounding to float32.
//   The top-K registers of sweep 1 are dead in sweep 2, where the nine float64 sums live: one launch holds both.
#include "knn_common.h"

#define GSR_GRADIENT_PIVOT_MIN 1e-12    // LDL^T: a pivot at or below this share of its diagonal entry is no pivot (registration.hip)

struct GradientWs {
  GsrNnWs nn;
  float* masked;     // float[P][3]: the points, NaN NaN NaN where point, normal or colour is not finite - what the structure is built over
  size_t total;
};
static GradientWs gradient_ws(void* base, size_t P) {
  GsrCarve c(base);
  GradientWs w;
  if (P == 0) P = 1;
  w.nn = nn_carve(c, P);
  w.masked = c.take<float>(3 * P);
  w.total = c.o;
  return w;
}

__device__ __forceinline__ bool gradient_finite3(const float* __restrict__ a, size_t i) {
  return knn_finite(a[3 * i]) && knn_finite(a[3 * i + 1]) && knn_finite(a[3 * i + 2]);
}
// I = (r + g + b) / 3 in float64, left to right
__device__ __forceinline__ double gradient_intensity(const float* __restrict__ colors, size_t row) {
  return (((double)colors[3 * row] + (double)colors[3 * row + 1]) + (double)colors[3 * row + 2]) / 3.0;
}

// the cloud the structure is built over (all three components NaN: the sorted copy needs no second pass)
__global__ __launch_bounds__(256) void k_gradient_mask(uint32_t P, const float* __restrict__ points, const float* __restrict__ colors,
                                                       const float* __restrict__ normals, float* __restrict__ masked) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  if (!(knn_finite(x) && knn_finite(y) && knn_finite(z) && gradient_finite3(colors, i) && gradient_finite3(normals, i)))
    x = y = z = __builtin_nanf("");
  masked[3 * (size_t)i] = x;
  masked[3 * (size_t)i + 1] = y;
  masked[3 * (size_t)i + 2] = z;
}

template <int K>
__global__ __launch_bounds__(256) void k_color_gradient(GsrKnnTree t, int k, float r2, const float* __restrict__ colors,
                                                        const float* __restrict__ normals, float* __restrict__ gradient,
                                                        int32_t* __restrict__ count_out, uint8_t* __restrict__ status_out) {
  __shared__ float4 s_lo[256], s_hi[256];
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const bool active = q < t.P;
  const uint32_t pos = active ? q : 0u;
  const float4 me = t.pts[pos];          // (pos < P always: P >= 1)
  const size_t row = (size_t)__float_as_uint(me.w);
  const bool finite = knn_finite(me.x);      // (a masked row is NaN in every component)
  // ---- sweep 1: min(r2, d_k) ----
  float bound;
  {
    float b[K];
    bound = knn_topk_bound<K, 256>(t, me, pos, active, k, r2, s_lo, s_hi, b);
  }
  // ---- sweep 2: the sums over { j != i : d2 <= bound } ----
  const double nx = (double)normals[3 * row], ny = (double)normals[3 * row + 1], nz = (double)normals[3 * row + 2];
  const double mine = gradient_intensity(colors, row);
  double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  uint32_t members = 0u;
  knn_member_walk<256>(t, me, pos, active, bound, s_lo, s_hi,
                       [&](const uint32_t j, const float fx, const float fy, const float fz) __attribute__((always_inline)) {
                         // delta = p_j - p_i = -(p_i - p_j), exactly
                         const double dx = -(double)fx, dy = -(double)fy, dz = -(double)fz;
                         const double along = (dx * nx + dy * ny) + dz * nz;
                         const double ux = dx - along * nx, uy = dy - along * ny, uz = dz - along * nz;
                         const double b = gradient_intensity(colors, (size_t)__float_as_uint(t.pts[j].w)) - mine;
                         members++;
                         axx += ux * ux; axy += ux * uy; axz += ux * uz;
                         ayy += uy * uy; ayz += uy * uz; azz += uz * uz;
                         gx += ux * b; gy += uy * b; gz += uz * b;
                       });
  if (!active) return;
  const uint32_t count = finite ? members + 1u : 0u;
  if (count_out) count_out[row] = (int32_t)count;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  uint8_t status = 0;
  if (!finite) {
    ox = oy = oz = __builtin_nanf("");
    status = 3;
  } else if (count < 4u) {
    status = 1;
  } else {
    // the constraint row w n, w = n_i - 1, right-hand side 0
    const double w = (double)(count - 1u), w2 = w * w;
    axx += w2 * (nx * nx); axy += w2 * (nx * ny); axz += w2 * (nx * nz);
    ayy += w2 * (ny * ny); ayz += w2 * (ny * nz); azz += w2 * (nz * nz);
    // A = L D L^T, L unit lower triangular; every pivot is held against its own diagonal entry
    const double inf = (double)KNN_INF;
    const double d0 = axx;
    bool ok = fabs(d0) < inf && d0 > GSR_GRADIENT_PIVOT_MIN * axx;
    const double l10 = axy / d0, l20 = axz / d0;
    const double d1 = ayy - l10 * l10 * d0;
    ok = ok && fabs(d1) < inf && d1 > GSR_GRADIENT_PIVOT_MIN * ayy;
    const double l21 = (ayz - l20 * l10 * d0) / d1;
    const double d2 = (azz - l20 * l20 * d0) - l21 * l21 * d1;
    ok = ok && fabs(d2) < inf && d2 > GSR_GRADIENT_PIVOT_MIN * azz;
    if (!ok) {
      status = 2;
    } else {
      const double y0 = gx, y1 = gy - l10 * y0, y2 = (gz - l20 * y0) - l21 * y1;
      const double x2 = y2 / d2;
      const double x1 = y1 / d1 - l21 * x2;
      const double x0 = (y0 / d0 - l10 * x1) - l20 * x2;
      ox = (float)x0; oy = (float)x1; oz = (float)x2;
    }
  }
  gradient[3 * row] = ox;
  gradient[3 * row + 1] = oy;
  gradient[3 * row + 2] = oz;
  if (status_out) status_out[row] = status;
}

extern "C" {

size_t gsr_color_gradient_workspace_bytes(int64_t P) { return gradient_ws(nullptr, (size_t)(P < 1 ? 1 : P)).total; }

int gsr_color_gradient(int64_t P, const float* points, const float* colors, const float* normals, float radius, int32_t max_nn,
                       float* gradient, int32_t* count_out, uint8_t* status_out, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (gsr_bad_size(P) || !points || !colors || !normals || !gradient || !workspace || max_nn < 4 || max_nn > GSR_KNN_K_MAX + 1 ||
      !(radius > 0.f)) {
    gsr_set_error("color_gradient: bad arguments (P = %lld, radius = %g: expected > 0, max_nn = %d: expected 4 .. %d)",
                  (long long)P, (double)radius, (int)max_nn, GSR_KNN_K_MAX + 1);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GradientWs w = gradient_ws(workspace, (size_t)P);
  if (!gsr_workspace_fits("color_gradient", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const GsrKnnTree t = knn_tree(w.nn, (size_t)P);
  const uint32_t nblk = (t.P + 255u) / 256u;
  GSR_LAUNCH("gradient_mask", k_gradient_mask, dim3(nblk), dim3(256), 0, st, t.P, points, colors, normals, w.masked);
  gsr_knn_build(P, w.masked, w.nn, st);
  const float r2 = radius * radius;      // the float32 square (+inf stays, and a large radius may become, +inf)
  const int k = (int)max_nn - 1;
#define GRADIENT_K(K) \
  GSR_LAUNCH("color_gradient_k" #K, k_color_gradient<K>, dim3(nblk), dim3(256), 0, st, t, k, r2, colors, normals, gradient, \
             count_out, status_out)
  GSR_KNN_PICK_K(k, GRADIENT_K);
#undef GRADIENT_K
  return gsr_launch_status("color_gradient launch");
}

}  // extern "C"
