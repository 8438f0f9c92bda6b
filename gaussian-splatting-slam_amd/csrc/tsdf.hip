// tsdf.hip - TSDF fusion on the device: depth frames into a block-sparse truncated signed distance volume, out as an oriented
// cloud and a triangle soup.  The volume, the four stages and their arithmetic are stated once, in
// include/gsr.h; this file follows that text.
//
//   k_tsdf_touch        one lane per pixel: unproject in float64, write the <= 27 keys of the blocks the box p +- sdf_trunc meets
//   k_tsdf_integrate    one workgroup per touched block, voxels lane and lane + 256: project, gather depth / colour, running average
//   k_tsdf_points       one workgroup per block in key order: 27 neighbour rows by binary search, tsdf of block + halo in LDS
//                       (NaN = unobserved or missing), count sign-change edges per voxel, workgroup scan, emit
//   k_tsdf_triangles    the same staging on 0 .. 8: marching tetrahedra over the six Kuhn tetrahedra of every cube
// Both extract kernels run twice (count, then emit at the offsets gsr_scan_u32 made of the block counts): the order of the output
// is fixed by the scan, not by the scheduler.  No atomics, no hash table, no workgroup waits on another.
#include "gsr_common.h"

#include <math.h>

namespace {

#define TSDF_HALO 11                       // -1 .. 9 per axis
#define TSDF_HALO_N (TSDF_HALO * TSDF_HALO * TSDF_HALO)
#define TSDF_BIAS (1 << 20)

struct TsdfVol {
  double origin[3];
  double vs;
  float trunc, depth_trunc, max_weight;
};

struct TsdfCam {
  double R[9];     // world-to-camera rotation, row-major
  double t[3];
  float fx, fy, cx, cy;
  int W, H;
};

struct TsdfStore {
  const long long* keys_sorted;
  const int* row_of_sorted;
  const float* tsdf;
  const float* weight;
  const float* color;
  int B;
  float min_weight;
};

__device__ __forceinline__ bool tsdf_in_range(int b) { return b >= -TSDF_BIAS && b < TSDF_BIAS; }
__device__ __forceinline__ long long tsdf_key(int bx, int by, int bz) {
  return ((long long)(bx + TSDF_BIAS) << 42) | ((long long)(by + TSDF_BIAS) << 21) | (long long)(bz + TSDF_BIAS);
}
__device__ __forceinline__ void tsdf_decode(long long key, int& bx, int& by, int& bz) {
  bx = (int)((key >> 42) & 0x1FFFFF) - TSDF_BIAS;
  by = (int)((key >> 21) & 0x1FFFFF) - TSDF_BIAS;
  bz = (int)(key & 0x1FFFFF) - TSDF_BIAS;
}
// float32 world position of a voxel centre from its global integer coordinate: product and sum rounded to float64 one by one (no
// fused multiply-add, so a float64 restatement gives the same bits), one rounding to float32
__device__ __forceinline__ float tsdf_centre(double origin, double vs, int g) {
  return (float)__dadd_rn(origin, __dmul_rn((double)g + 0.5, vs));
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsdf_touch(const TsdfVol V, const TsdfCam C, const float* __restrict__ depth,
                                                    const float* __restrict__ mask, long long* __restrict__ keys) {
  const int n = C.W * C.H;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long* out = keys + i;          // slot s of this pixel: out[s n]; the sentinel first, then the slots in use (same lane, in order)
#pragma unroll
  for (int s = 0; s < GSR_TSDF_TOUCH_SLOTS; s++) out[(size_t)s * (size_t)n] = GSR_TSDF_NO_KEY;
  const float d = depth[i];
  if ((!mask || mask[i] != 0.f) && d > 0.f && d <= V.depth_trunc) {
    const int u = i % C.W, v = i / C.W;
    const double dd = (double)d;
    const double q0 = ((double)u - (double)C.cx) / (double)C.fx * dd - C.t[0];
    const double q1 = ((double)v - (double)C.cy) / (double)C.fy * dd - C.t[1];
    const double q2 = dd - C.t[2];
    int lo[3], cnt[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double p = C.R[a] * q0 + C.R[3 + a] * q1 + C.R[6 + a] * q2;      // R^T q
      const double side = 8.0 * V.vs;
      const double l = floor((p - (double)V.trunc - V.origin[a]) / side), h = floor((p + (double)V.trunc - V.origin[a]) / side);
      if (!(l >= -(double)TSDF_BIAS - 4.0 && h < (double)TSDF_BIAS + 4.0)) {   // (false for NaN) far outside: nothing to name
        ok = false;
        lo[a] = cnt[a] = 0;
      } else {
        lo[a] = (int)l;
        const int c = (int)h - lo[a] + 1;
        cnt[a] = c < 1 ? 1 : (c > 3 ? 3 : c);
      }
    }
    if (ok) {
      int s = 0;
      for (int ix = 0; ix < cnt[0]; ix++)
        for (int iy = 0; iy < cnt[1]; iy++)
          for (int iz = 0; iz < cnt[2]; iz++) {
            const int bx = lo[0] + ix, by = lo[1] + iy, bz = lo[2] + iz;
            if (tsdf_in_range(bx) && tsdf_in_range(by) && tsdf_in_range(bz)) out[(size_t)s * (size_t)n] = tsdf_key(bx, by, bz);
            s++;
          }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsdf_integrate(const TsdfVol V, const TsdfCam C, const float* __restrict__ depth,
                                                        const float* __restrict__ mask, const float* __restrict__ color,
                                                        const long long* __restrict__ keys, const int* __restrict__ rows,
                                                        const int n_rows, float* __restrict__ tsdf, float* __restrict__ weight,
                                                        float* __restrict__ col) {
  const int row = rows[blockIdx.x];
  if (row < 0 || row >= n_rows) return;
  int b[3];
  tsdf_decode(keys[blockIdx.x], b[0], b[1], b[2]);
  // centre of voxel (0, 0, 0) in camera space and the three voxel steps: float64, rounded once (the same in every lane)
  double w[3];
#pragma unroll
  for (int a = 0; a < 3; a++) w[a] = V.origin[a] + ((double)(8 * b[a]) + 0.5) * V.vs;
  float c[3], sx[3], sy[3], sz[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c[k] = (float)(C.R[3 * k] * w[0] + C.R[3 * k + 1] * w[1] + C.R[3 * k + 2] * w[2] + C.t[k]);
    sx[k] = (float)(C.R[3 * k] * V.vs);
    sy[k] = (float)(C.R[3 * k + 1] * V.vs);
    sz[k] = (float)(C.R[3 * k + 2] * V.vs);
  }
  const size_t plane = (size_t)C.W * (size_t)C.H;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int lin = (int)threadIdx.x + 256 * h;
    const float lx = (float)(lin & 7), ly = (float)((lin >> 3) & 7), lz = (float)(lin >> 6);
    const float x = c[0] + lx * sx[0] + ly * sy[0] + lz * sz[0];
    const float y = c[1] + lx * sx[1] + ly * sy[1] + lz * sz[1];
    const float z = c[2] + lx * sx[2] + ly * sy[2] + lz * sz[2];
    if (!(z > 0.f)) continue;
    const float qx = x / z, qy = y / z;
    const float uf = floorf(C.fx * qx + C.cx + 0.5f), vf = floorf(C.fy * qy + C.cy + 0.5f);
    if (!(uf >= 0.f && uf < (float)C.W && vf >= 0.f && vf < (float)C.H)) continue;      // (false for NaN)
    const size_t pix = (size_t)(int)vf * (size_t)C.W + (size_t)(int)uf;
    if (mask && mask[pix] == 0.f) continue;
    const float d = depth[pix];
    if (!(d > 0.f && d <= V.depth_trunc)) continue;
    const float sdf = (d - z) * sqrtf(1.0f + qx * qx + qy * qy);
    if (!(sdf > -V.trunc)) continue;
    const float f = fminf(1.0f, sdf / V.trunc);
    const size_t idx = (size_t)row * GSR_TSDF_BLOCK_VOXELS + (size_t)lin;
    const float wt = weight[idx], w1 = wt + 1.0f;
    tsdf[idx] = (tsdf[idx] * wt + f) / w1;
    if (color) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) col[idx * 3 + ch] = (col[idx * 3 + ch] * wt + color[(size_t)ch * plane + pix]) / w1;
    }
    weight[idx] = fminf(w1, V.max_weight);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Staging shared by the two extract kernels: the rows of the 27 neighbour blocks (lanes 0 .. 26; -1 = absent) and the tsdf of the
// local coordinates lo .. hi per axis (of -1 .. 9) as sh_f[(lx + 1) + 11 (ly + 1) + 121 (lz + 1)], NaN where the voxel is
// unobserved, its block absent, or outside lo .. hi.
__device__ __forceinline__ void tsdf_stage(const TsdfStore& S, const int lo, const int hi, float* sh_f, int* sh_rows, int (&b)[3]) {
  tsdf_decode(S.keys_sorted[blockIdx.x], b[0], b[1], b[2]);
  if (threadIdx.x < 27) {
    const int t = (int)threadIdx.x;
    const int nx = b[0] + t % 3 - 1, ny = b[1] + (t / 3) % 3 - 1, nz = b[2] + t / 9 - 1;
    int row = -1;
    if (tsdf_in_range(nx) && tsdf_in_range(ny) && tsdf_in_range(nz)) {
      const long long k = tsdf_key(nx, ny, nz);
      int l = 0, h = S.B;
      while (l < h) {
        const int m = (l + h) >> 1;
        if (S.keys_sorted[m] < k) l = m + 1;
        else h = m;
      }
      if (l < S.B && S.keys_sorted[l] == k) {
        row = S.row_of_sorted[l];
        if (row < 0 || row >= S.B) row = -1;
      }
    }
    sh_rows[t] = row;
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < TSDF_HALO_N; idx += 256) {
    const int lx = idx % TSDF_HALO - 1, ly = (idx / TSDF_HALO) % TSDF_HALO - 1, lz = idx / (TSDF_HALO * TSDF_HALO) - 1;
    float val = __builtin_nanf("");
    if (lx >= lo && lx <= hi && ly >= lo && ly <= hi && lz >= lo && lz <= hi) {
      const int nb = (lx < 0 ? 0 : (lx < 8 ? 1 : 2)) + 3 * (ly < 0 ? 0 : (ly < 8 ? 1 : 2)) + 9 * (lz < 0 ? 0 : (lz < 8 ? 1 : 2));
      const int row = sh_rows[nb];
      if (row >= 0) {
        const size_t at = (size_t)row * GSR_TSDF_BLOCK_VOXELS + (size_t)((lx & 7) + 8 * (ly & 7) + 64 * (lz & 7));
        if (S.weight[at] > S.min_weight) val = S.tsdf[at];
      }
    }
    sh_f[idx] = val;
  }
  __syncthreads();
}

// colour of the voxel at local coordinates (lx, ly, lz) in -1 .. 9 (its block is present: the caller saw it observed)
__device__ __forceinline__ const float* tsdf_color_at(const TsdfStore& S, const int* sh_rows, int lx, int ly, int lz) {
  const int nb = (lx < 0 ? 0 : (lx < 8 ? 1 : 2)) + 3 * (ly < 0 ? 0 : (ly < 8 ? 1 : 2)) + 9 * (lz < 0 ? 0 : (lz < 8 ? 1 : 2));
  const int row = sh_rows[nb];
  return S.color + ((size_t)(row < 0 ? 0 : row) * GSR_TSDF_BLOCK_VOXELS + (size_t)((lx & 7) + 8 * (ly & 7) + 64 * (lz & 7))) * 3;
}

__device__ __forceinline__ int tsdf_halo_index(int lx, int ly, int lz) {
  return (lx + 1) + TSDF_HALO * (ly + 1) + TSDF_HALO * TSDF_HALO * (lz + 1);
}

// exclusive prefix of `v` over the 256 threads in thread order; `total` in every thread.  sh_w: 4 words of LDS.
__device__ __forceinline__ uint32_t tsdf_block_scan(uint32_t v, uint32_t* sh_w, uint32_t& total) {
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o, 64);
    if (gsr_lane() >= o) inc += up;
  }
  if (gsr_lane() == 63) sh_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  const int wv = (int)(threadIdx.x >> 6);
  uint32_t base = 0;
  for (int k = 0; k < wv; k++) base += sh_w[k];
  total = sh_w[0] + sh_w[1] + sh_w[2] + sh_w[3];
  return base + inc - v;
}

// gradient of tsdf in voxel units at halo index `at`
__device__ __forceinline__ void tsdf_gradient(const float* sh_f, const int at, float (&g)[3]) {
  const float f0 = sh_f[at];
  const int stride[3] = {1, TSDF_HALO, TSDF_HALO * TSDF_HALO};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float fp = sh_f[at + stride[a]], fm = sh_f[at - stride[a]];
    const bool hp = fp == fp, hm = fm == fm;
    g[a] = (hp && hm) ? 0.5f * (fp - fm) : (hp ? fp - f0 : (hm ? f0 - fm : 0.f));
  }
}

template <bool EMIT>
__global__ void __launch_bounds__(256) k_tsdf_points(const TsdfVol V, const TsdfStore S, uint32_t* __restrict__ block_count,
                                                     const uint32_t* __restrict__ block_offs, const long long capacity,
                                                     float* __restrict__ points, float* __restrict__ normals,
                                                     float* __restrict__ colors) {
  __shared__ float sh_f[TSDF_HALO_N];
  __shared__ int sh_rows[27];
  __shared__ uint32_t sh_w[4];
  int b[3];
  tsdf_stage(S, -1, 9, sh_f, sh_rows, b);
  const int stride[3] = {1, TSDF_HALO, TSDF_HALO * TSDF_HALO};
  uint32_t edges[2];
  uint32_t n = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int lin = 2 * (int)threadIdx.x + h;
    const int at = tsdf_halo_index(lin & 7, (lin >> 3) & 7, lin >> 6);
    const float fi = sh_f[at];
    uint32_t m = 0;
    if (fi == fi) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float fj = sh_f[at + stride[a]];
        if (fj == fj && ((fi < 0.f) != (fj < 0.f))) m |= 1u << a;
      }
    }
    edges[h] = m;
    n += __popc(m);
  }
  uint32_t total;
  uint32_t o = tsdf_block_scan(n, sh_w, total);
  if (!EMIT) {
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
    return;
  }
  long long at_out = (long long)block_offs[blockIdx.x] + (long long)o;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int lin = 2 * (int)threadIdx.x + h;
    const int l[3] = {lin & 7, (lin >> 3) & 7, lin >> 6};
    const int at = tsdf_halo_index(l[0], l[1], l[2]);
    for (int a = 0; a < 3; a++) {
      if (!(edges[h] & (1u << a))) continue;
      if (at_out < capacity) {
        const float flo = sh_f[at], fhi = sh_f[at + stride[a]];
        const float t = flo / (flo - fhi);
        float glo[3], ghi[3], nrm[3];
        tsdf_gradient(sh_f, at, glo);
        tsdf_gradient(sh_f, at + stride[a], ghi);
        float n2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          nrm[k] = glo[k] + t * (ghi[k] - glo[k]);
          n2 += nrm[k] * nrm[k];
        }
        const float len = sqrtf(n2);
        const int j[3] = {l[0] + (a == 0), l[1] + (a == 1), l[2] + (a == 2)};
        const float* clo = tsdf_color_at(S, sh_rows, l[0], l[1], l[2]);
        const float* chi = tsdf_color_at(S, sh_rows, j[0], j[1], j[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float plo = tsdf_centre(V.origin[k], V.vs, 8 * b[k] + l[k]);
          const float phi = tsdf_centre(V.origin[k], V.vs, 8 * b[k] + j[k]);
          points[at_out * 3 + k] = plo + t * (phi - plo);
          normals[at_out * 3 + k] = len > 0.f ? nrm[k] / len : 0.f;
          const float c0 = clo[k], c1 = chi[k];
          colors[at_out * 3 + k] = c0 + t * (c1 - c0);
        }
      }
      at_out++;
    }
  }
}

// The six Kuhn tetrahedra: the order (a, b, c) in which the axes are stepped from corner 0 to corner 7, and the sign of
// det[v1 - v0, v2 - v0, v3 - v0] = the parity of that order.
__constant__ int c_kuhn[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__constant__ int c_kuhn_sign[6] = {1, -1, -1, 1, 1, -1};

// The triangles of one tetrahedron whose vertex k is inside where bit k of `m` is set: `e` receives per triangle three edges, each
// (k_from << 2) | k_to with k_from < k_to in path order; returns the number of triangles.  sigma: the tetrahedron's orientation.
__device__ __forceinline__ int tsdf_tet_triangles(const int m, const int sigma, int (&e)[2][3]) {
  const int n_in = __popc((unsigned)m);
  if (n_in == 0 || n_in == 4) return 0;
  auto edge = [](int p, int q) { return p < q ? ((p << 2) | q) : ((q << 2) | p); };
  if (n_in == 1 || n_in == 3) {
    const int single = n_in == 1 ? m : (~m & 15);
    const int k = __ffs(single) - 1;
    int o[3], c = 0;
    for (int q = 0; q < 4; q++)
      if (q != k) o[c++] = q;
    int sign = (k & 1) ? -sigma : sigma;       // parity of (k, the others ascending)
    if (n_in == 3) sign = -sign;
    e[0][0] = edge(k, o[0]);
    e[0][1] = edge(k, sign > 0 ? o[1] : o[2]);
    e[0][2] = edge(k, sign > 0 ? o[2] : o[1]);
    return 1;
  }
  int in[2], out[2], ci = 0, co = 0;
  for (int q = 0; q < 4; q++) {
    if (m & (1 << q)) in[ci++] = q;
    else out[co++] = q;
  }
  const int A = in[0], B = in[1], Cc = out[0], D = out[1];
  const int inv = (A > Cc) + (A > D) + (B > Cc) + (B > D);      // inversions of (A, B, C, D): A < B and C < D
  const int sign = (inv & 1) ? -sigma : sigma;
  const int AC = edge(A, Cc), AD = edge(A, D), BD = edge(B, D), BC = edge(B, Cc);
  if (sign > 0) {
    e[0][0] = AC, e[0][1] = AD, e[0][2] = BD;
    e[1][0] = AC, e[1][1] = BD, e[1][2] = BC;
  } else {
    e[0][0] = AC, e[0][1] = BD, e[0][2] = AD;
    e[1][0] = AC, e[1][1] = BC, e[1][2] = BD;
  }
  return 2;
}

template <bool EMIT>
__global__ void __launch_bounds__(256) k_tsdf_triangles(const TsdfVol V, const TsdfStore S, uint32_t* __restrict__ block_count,
                                                        const uint32_t* __restrict__ block_offs, const long long capacity,
                                                        float* __restrict__ positions, float* __restrict__ colors) {
  __shared__ float sh_f[TSDF_HALO_N];
  __shared__ int sh_rows[27];
  __shared__ uint32_t sh_w[4];
  int b[3];
  tsdf_stage(S, 0, 8, sh_f, sh_rows, b);
  int inside[2];       // bit c: corner c has tsdf < 0; -1: the cube is not used
  uint32_t n = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int lin = 2 * (int)threadIdx.x + h;
    const int l[3] = {lin & 7, (lin >> 3) & 7, lin >> 6};
    int m = 0;
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float f = sh_f[tsdf_halo_index(l[0] + (c & 1), l[1] + ((c >> 1) & 1), l[2] + (c >> 2))];
      all = all && (f == f);
      if (f < 0.f) m |= 1 << c;
    }
    inside[h] = all ? m : -1;
    if (all && m != 0 && m != 255) {
      for (int tet = 0; tet < 6; tet++) {
        const int c1 = 1 << c_kuhn[tet][0], c2 = c1 | (1 << c_kuhn[tet][1]);
        const int n_in = (m & 1) + ((m >> c1) & 1) + ((m >> c2) & 1) + ((m >> 7) & 1);
        n += (n_in == 2) ? 2u : ((n_in == 1 || n_in == 3) ? 1u : 0u);
      }
    }
  }
  uint32_t total;
  uint32_t o = tsdf_block_scan(n, sh_w, total);
  if (!EMIT) {
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
    return;
  }
  long long at_out = (long long)block_offs[blockIdx.x] + (long long)o;
#pragma unroll 1
  for (int h = 0; h < 2; h++) {
    const int m = inside[h];
    if (m <= 0 || m == 255) continue;
    const int lin = 2 * (int)threadIdx.x + h;
    const int l[3] = {lin & 7, (lin >> 3) & 7, lin >> 6};
#pragma unroll 1
    for (int tet = 0; tet < 6; tet++) {
      int corner[4];
      corner[0] = 0;
      corner[1] = 1 << c_kuhn[tet][0];
      corner[2] = corner[1] | (1 << c_kuhn[tet][1]);
      corner[3] = 7;
      int tm = 0;
      for (int k = 0; k < 4; k++) tm |= ((m >> corner[k]) & 1) << k;
      int e[2][3];
      const int nt = tsdf_tet_triangles(tm, c_kuhn_sign[tet], e);
      for (int tri = 0; tri < nt; tri++) {
        if (at_out < capacity) {
          for (int vtx = 0; vtx < 3; vtx++) {
            const int clo = corner[e[tri][vtx] >> 2], chi = corner[e[tri][vtx] & 3];
            const int a[3] = {l[0] + (clo & 1), l[1] + ((clo >> 1) & 1), l[2] + (clo >> 2)};
            const int j[3] = {l[0] + (chi & 1), l[1] + ((chi >> 1) & 1), l[2] + (chi >> 2)};
            const float flo = sh_f[tsdf_halo_index(a[0], a[1], a[2])], fhi = sh_f[tsdf_halo_index(j[0], j[1], j[2])];
            const float t = flo / (flo - fhi);
            const float* col_lo = tsdf_color_at(S, sh_rows, a[0], a[1], a[2]);
            const float* col_hi = tsdf_color_at(S, sh_rows, j[0], j[1], j[2]);
            const long long w = (at_out * 3 + vtx) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
              const float plo = tsdf_centre(V.origin[k], V.vs, 8 * b[k] + a[k]);
              const float phi = tsdf_centre(V.origin[k], V.vs, 8 * b[k] + j[k]);
              positions[w + k] = plo + t * (phi - plo);
              const float c0 = col_lo[k], c1 = col_hi[k];
              colors[w + k] = c0 + t * (c1 - c0);
            }
          }
        }
        at_out++;
      }
    }
  }
}

__global__ void k_tsdf_total(const uint32_t* __restrict__ count, const uint32_t* __restrict__ offs, const int B,
                             long long* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (long long)offs[B - 1] + (long long)count[B - 1];
}

// ---------------------------------------------------------------------------------------------------------------------------------
bool finite_d(double v) { return fabs(v) < (double)KNN_INF * 1e270; }       // false for NaN and +-inf
bool finite_f(float v) { return fabsf(v) < KNN_INF; }

bool volume_ok(const gsr_tsdf_volume* v, const char* who) {
  if (!v) {
    gsr_set_error("%s: NULL volume", who);
    return false;
  }
  const bool ok = finite_d(v->origin[0]) && finite_d(v->origin[1]) && finite_d(v->origin[2]) && finite_d(v->voxel_size) &&
                  v->voxel_size > 0.0 && finite_f(v->sdf_trunc) && (double)v->sdf_trunc >= v->voxel_size &&
                  (double)v->sdf_trunc <= 8.0 * v->voxel_size && v->depth_trunc > 0.f && v->max_weight >= 1.f;
  if (!ok)
    gsr_set_error("%s: bad volume (voxel_size = %g, sdf_trunc = %g: expected voxel_size .. 8 voxel_size, depth_trunc = %g, "
                  "max_weight = %g, origin = %g %g %g)", who, v->voxel_size, (double)v->sdf_trunc, (double)v->depth_trunc,
                  (double)v->max_weight, v->origin[0], v->origin[1], v->origin[2]);
  return ok;
}

bool frame_ok(const gsr_tsdf_frame* f, const char* who) {
  if (!f) {
    gsr_set_error("%s: NULL frame", who);
    return false;
  }
  bool ok = f->width >= 1 && f->height >= 1 && (int64_t)f->width * (int64_t)f->height <= ((int64_t)1 << 26) && f->depth != nullptr;
  for (int i = 0; i < 4; i++) ok = ok && finite_f(f->K[i]);
  ok = ok && f->K[0] > 0.f && f->K[1] > 0.f;
  for (int i = 0; i < 12; i++) ok = ok && finite_d(f->w2c[i]);
  if (!ok)
    gsr_set_error("%s: bad frame (%d x %d, K = %g %g %g %g, depth %s; K and w2c must be finite, fx, fy > 0)", who, f->width, f->height,
                  (double)f->K[0], (double)f->K[1], (double)f->K[2], (double)f->K[3], f->depth ? "given" : "NULL");
  return ok;
}

TsdfVol make_vol(const gsr_tsdf_volume* v) {
  TsdfVol V;
  for (int a = 0; a < 3; a++) V.origin[a] = v->origin[a];
  V.vs = v->voxel_size;
  V.trunc = v->sdf_trunc;
  V.depth_trunc = v->depth_trunc;
  V.max_weight = v->max_weight;
  return V;
}

TsdfCam make_cam(const gsr_tsdf_frame* f) {
  TsdfCam C;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) C.R[3 * r + c] = f->w2c[4 * r + c];
    C.t[r] = f->w2c[4 * r + 3];
  }
  C.fx = f->K[0], C.fy = f->K[1], C.cx = f->K[2], C.cy = f->K[3];
  C.W = f->width, C.H = f->height;
  return C;
}

// the workspace of the two extract calls: per block its count of outputs, their exclusive scan, the scan's scratch
struct TsdfExtractWs {
  uint32_t *count, *offs, *scan_tmp;      // u32[B], u32[B], gsr_scan_tmp_elems(B) words
  size_t total;
};
TsdfExtractWs extract_ws(void* base, size_t B) {
  GsrCarve c(base);
  TsdfExtractWs w;
  w.count = c.take<uint32_t>(B);
  w.offs = c.take<uint32_t>(B);
  w.scan_tmp = c.take<uint32_t>(gsr_scan_tmp_elems(B));
  w.total = c.o;
  return w;
}

// the checks the two extract calls share; -> 0, or the error code
int extract_check(const char* who, const gsr_tsdf_volume* vol, int64_t B, const void* keys_sorted, const void* row_of_sorted,
                  const void* tsdf, const void* weight, const void* color, float min_weight, int64_t capacity, bool outputs,
                  const void* count_dev, const void* workspace, size_t workspace_bytes) {
  if (!volume_ok(vol, who)) return GSR_ERR_INVALID_ARGUMENT;
  if (B < 0 || B > GSR_TSDF_MAX_BLOCKS || !count_dev || capacity < 0 || (capacity > 0 && !outputs) || !(min_weight >= 0.f) ||
      (B > 0 && (!keys_sorted || !row_of_sorted || !tsdf || !weight || !color || !workspace))) {
    gsr_set_error("%s: bad arguments (B = %lld: expected 0 .. %d, capacity = %lld, min_weight = %g)", who, (long long)B,
                  GSR_TSDF_MAX_BLOCKS, (long long)capacity, (double)min_weight);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (B > 0 && !gsr_workspace_fits(who, workspace, workspace_bytes, extract_ws(nullptr, (size_t)B).total))
    return GSR_ERR_STATE_TOO_SMALL;
  return 0;
}

}  // namespace

extern "C" {

int gsr_tsdf_touch(const gsr_tsdf_volume* vol, const gsr_tsdf_frame* frame, int64_t* keys_out, void* stream) {
  if (!volume_ok(vol, "tsdf_touch") || !frame_ok(frame, "tsdf_touch")) return GSR_ERR_INVALID_ARGUMENT;
  if (!keys_out) {
    gsr_set_error("tsdf_touch: NULL keys_out");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = (hipStream_t)stream;
  const int n = frame->width * frame->height;
  GSR_LAUNCH("tsdf_touch", k_tsdf_touch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, make_vol(vol), make_cam(frame),
             frame->depth, frame->mask, (long long*)keys_out);
  return gsr_launch_status("tsdf_touch launch");
}

int gsr_tsdf_integrate(const gsr_tsdf_volume* vol, const gsr_tsdf_frame* frame, int64_t n_blocks, const int64_t* keys,
                       const int32_t* rows, int64_t n_rows, float* tsdf, float* weight, float* color, void* stream) {
  if (!volume_ok(vol, "tsdf_integrate") || !frame_ok(frame, "tsdf_integrate")) return GSR_ERR_INVALID_ARGUMENT;
  if (n_blocks < 0 || n_blocks > GSR_TSDF_MAX_BLOCKS || n_rows < 0 || n_rows > GSR_TSDF_MAX_BLOCKS || n_blocks > n_rows ||
      (n_blocks > 0 && (!keys || !rows || !tsdf || !weight)) || (n_blocks > 0 && frame->color && !color)) {
    gsr_set_error("tsdf_integrate: bad arguments (n_blocks = %lld, n_rows = %lld: expected n_blocks <= n_rows <= %d)",
                  (long long)n_blocks, (long long)n_rows, GSR_TSDF_MAX_BLOCKS);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (n_blocks == 0) return GSR_OK;
  hipStream_t st = (hipStream_t)stream;
  GSR_LAUNCH("tsdf_integrate", k_tsdf_integrate, dim3((unsigned)n_blocks), dim3(256), 0, st, make_vol(vol), make_cam(frame),
             frame->depth, frame->mask, frame->color, (const long long*)keys, (const int*)rows, (int)n_rows, tsdf, weight, color);
  return gsr_launch_status("tsdf_integrate launch");
}

size_t gsr_tsdf_extract_workspace_bytes(int64_t B) {
  return extract_ws(nullptr, (size_t)(B < 1 ? 1 : (B > GSR_TSDF_MAX_BLOCKS ? GSR_TSDF_MAX_BLOCKS : B))).total;
}

int gsr_tsdf_extract_points(const gsr_tsdf_volume* vol, int64_t B, const int64_t* keys_sorted, const int32_t* row_of_sorted,
                            const float* tsdf, const float* weight, const float* color, float min_weight, int64_t capacity,
                            float* points, float* normals, float* colors, int64_t* count_dev, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const int rc = extract_check("tsdf_extract_points", vol, B, keys_sorted, row_of_sorted, tsdf, weight, color, min_weight, capacity,
                               points && normals && colors, count_dev, workspace, workspace_bytes);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) return gsr_check(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st), "tsdf_extract_points memset");
  const TsdfExtractWs w = extract_ws(workspace, (size_t)B);
  const TsdfVol V = make_vol(vol);
  const TsdfStore S = {(const long long*)keys_sorted, (const int*)row_of_sorted, tsdf, weight, color, (int)B, min_weight};
  GSR_LAUNCH("tsdf_points_count", k_tsdf_points<false>, dim3((unsigned)B), dim3(256), 0, st, V, S, w.count, (const uint32_t*)w.offs,
             (long long)0, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  gsr_scan_u32(w.count, nullptr, w.offs, (size_t)B, 0, w.scan_tmp, st);
  GSR_LAUNCH("tsdf_total", k_tsdf_total, dim3(1), dim3(64), 0, st, (const uint32_t*)w.count, (const uint32_t*)w.offs, (int)B,
             (long long*)count_dev);
  if (capacity > 0)
    GSR_LAUNCH("tsdf_points_emit", k_tsdf_points<true>, dim3((unsigned)B), dim3(256), 0, st, V, S, w.count, (const uint32_t*)w.offs,
               (long long)capacity, points, normals, colors);
  return gsr_launch_status("tsdf_extract_points launch");
}

int gsr_tsdf_extract_triangles(const gsr_tsdf_volume* vol, int64_t B, const int64_t* keys_sorted, const int32_t* row_of_sorted,
                               const float* tsdf, const float* weight, const float* color, float min_weight, int64_t capacity,
                               float* positions, float* colors, int64_t* count_dev, void* workspace, size_t workspace_bytes,
                               void* stream) {
  const int rc = extract_check("tsdf_extract_triangles", vol, B, keys_sorted, row_of_sorted, tsdf, weight, color, min_weight,
                               capacity, positions && colors, count_dev, workspace, workspace_bytes);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) return gsr_check(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st), "tsdf_extract_triangles memset");
  const TsdfExtractWs w = extract_ws(workspace, (size_t)B);
  const TsdfVol V = make_vol(vol);
  const TsdfStore S = {(const long long*)keys_sorted, (const int*)row_of_sorted, tsdf, weight, color, (int)B, min_weight};
  GSR_LAUNCH("tsdf_triangles_count", k_tsdf_triangles<false>, dim3((unsigned)B), dim3(256), 0, st, V, S, w.count,
             (const uint32_t*)w.offs, (long long)0, (float*)nullptr, (float*)nullptr);
  gsr_scan_u32(w.count, nullptr, w.offs, (size_t)B, 0, w.scan_tmp, st);
  GSR_LAUNCH("tsdf_total", k_tsdf_total, dim3(1), dim3(64), 0, st, (const uint32_t*)w.count, (const uint32_t*)w.offs, (int)B,
             (long long*)count_dev);
  if (capacity > 0)
    GSR_LAUNCH("tsdf_triangles_emit", k_tsdf_triangles<true>, dim3((unsigned)B), dim3(256), 0, st, V, S, w.count,
               (const uint32_t*)w.offs, (long long)capacity, positions, colors);
  return gsr_launch_status("tsdf_extract_triangles launch");
}

}  // extern "C"
