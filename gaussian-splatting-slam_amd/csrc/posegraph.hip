// posegraph.hip - edges in, corrections out (include/gsr.h, "pose graph").
//
// gsr_registration_information: Open3D's GetInformationMatrixFromPointClouds as a device reduction over the correspondences - the
// partial-sum rows of gsr_common.h (at most GSR_GN_BLOCKS workgroups, a fixed butterfly, no float atomics).
//
// gsr_posegraph_linearize / _solve / _optimize: three entries over ONE set of device functions (pg_edges, pg_nodes,
// pg_pcg).  Every launch is ONE workgroup of 256 lanes: a pose graph is small and latency-bound, and one workgroup needs no
// grid-wide synchronisation, no cooperative launch and no waiting of one workgroup on another.  Work is strided over edges and
// nodes (thread t owns nodes t, t + 256, ... in every phase), phases are separated by __syncthreads(), iterates live in the
// workspace; LDS holds the four wave sums of a reduction and nothing else, so N and E are bounded by their int32 range, not by LDS.
// Every loop is bounded by max_iteration, cg_max_iteration or a count: a launch cannot hang.  All arithmetic is float64.
//
// DETERMINISM: a node sums its incident edges in ascending edge index through the CSR of gsr_posegraph_topology; a dot product is
// each thread's own nodes in order, the fixed butterfly of gsr_wave_sum, then the four wave sums in order.  Every thread holds the
// same bits of every scalar, so control flow is uniform, and two runs give identical bits.
//
// The 6 x 6 factorisation, its pivot rule and M(delta) are the bodies of solve6_common.h: the ICP and odometry updates and the pose
// graph agree by construction.
#include "gsr_common.h"
#include "solve6_common.h"

#define PG_EDGE 35      // e[6] r w W[21] g[6]
#define PG_NODE 27      // H_ii[21] b[6]
#define PG_INFO_SUMS 22 // n, the upper triangle of sum G^T G

namespace {

// the topology blob (built on the host, read on the device): edge ends, the CSR of every node's incident edges, the fixed flags
struct PgTopo {
  int32_t *s, *t;      // int32[E] each (one element when E = 0)
  int32_t* ptr;        // int32[N + 1]
  int32_t* adj;        // int32[2 E]
  int32_t* fixed;      // int32[N]
  size_t total;
};
inline PgTopo pg_topo(const void* base, size_t N, size_t E) {
  GsrCarve c(base);
  PgTopo w;
  w.s = c.take<int32_t>(E ? E : 1);
  w.t = c.take<int32_t>(E ? E : 1);
  w.ptr = c.take<int32_t>(N + 1);
  w.adj = c.take<int32_t>(E ? 2 * E : 1);
  w.fixed = c.take<int32_t>(N);
  w.total = c.o;
  return w;
}
// the workspace of a solve or an optimisation: the trial poses, the edge and node records, the factors, the PCG's iterates
struct PgWs {
  double *Xn, *erec, *nrec, *fac, *x, *r, *z, *p, *Ap;
  size_t total;
};
inline PgWs pg_ws(void* base, size_t N, size_t E) {
  GsrCarve c(base);
  PgWs w;
  w.Xn = c.take<double>(N * 16);
  w.erec = c.take<double>((E ? E : 1) * PG_EDGE);
  w.nrec = c.take<double>(N * PG_NODE);
  w.fac = c.take<double>(N * 21);
  w.x = c.take<double>(N * 6);
  w.r = c.take<double>(N * 6);
  w.z = c.take<double>(N * 6);
  w.p = c.take<double>(N * 6);
  w.Ap = c.take<double>(N * 6);
  w.total = c.o;
  return w;
}
inline bool pg_bad_sizes(int64_t N, int64_t E) { return N < 1 || N > 0x3FFFFFFF || E < 0 || E > 0x3FFFFFFF; }

struct PgCtx {
  int N, E;
  const int32_t *es, *et, *ptr, *adj, *fixed;
  const double *eT, *eL;      // [E,16], [E,36]
  const uint8_t* unc;         // [E]
  double mu;
  double *erec, *nrec;        // [E,PG_EDGE], [N,PG_NODE]
  double *fac, *x, *r, *z, *p, *Ap, *Xn;
};

// ---- reductions: the same bits in every thread ---------------------------------------------------------------------------------
__device__ __forceinline__ double pg_sum(double v) {
  __shared__ double sh[4];
  v = gsr_wave_sum(v);
  if (gsr_lane() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();      // the array is free again; global writes before the call are visible to the workgroup after it
  return v;
}
__device__ __forceinline__ double pg_max(double v) {
  __shared__ double sh[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if (gsr_lane() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return v;
}

// ---- small algebra ------------------------------------------------------------------------------------------------------------
// y (+)= sign W v, W symmetric, its upper triangle stored row by row
__device__ __forceinline__ void pg_sym_mul(const double* __restrict__ W, const double (&v)[6], double (&y)[6], double sign) {
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = a; b < 6; b++) {
      const double w = sign * W[o++];
      y[a] += w * v[b];
      if (b != a) y[b] += w * v[a];
    }
  }
}
// vec6, the inverse of M: the angles of R = Rz Ry Rx and the last column
__device__ __forceinline__ void pg_vec6(const double (&R)[3][3], const double (&t)[3], double (&e)[6]) {
  const double sy = sqrt(R[0][0] * R[0][0] + R[1][0] * R[1][0]);
  if (sy > 1e-6) {
    e[0] = atan2(R[2][1], R[2][2]);
    e[1] = atan2(-R[2][0], sy);
    e[2] = atan2(R[1][0], R[0][0]);
  } else {
    e[0] = atan2(-R[1][2], R[1][1]);
    e[1] = atan2(-R[2][0], sy);
    e[2] = 0.0;
  }
  e[3] = t[0]; e[4] = t[1]; e[5] = t[2];
}
// C = A^T B
__device__ __forceinline__ void pg_mul_tn(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) C[a][b] = (A[0][a] * B[0][b] + A[1][a] * B[1][b]) + A[2][a] * B[2][b];
}
__device__ __forceinline__ void pg_load(const double* __restrict__ X, double (&R)[3][3], double (&t)[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) R[a][b] = X[4 * a + b];
    t[a] = X[4 * a + 3];
  }
}
// e_j x v
__device__ __forceinline__ void pg_cross_axis(int j, double v0, double v1, double v2, double (&o)[3]) {
  if (j == 0) { o[0] = 0.0; o[1] = -v2; o[2] = v1; }
  else if (j == 1) { o[0] = v2; o[1] = 0.0; o[2] = -v0; }
  else { o[0] = -v1; o[1] = v0; o[2] = 0.0; }
}

// One edge at the poses Xs, Xt: e, r, w into rec[0..7] and its share of F into `cost`; with `full` the Jacobian, W and g too.
__device__ void pg_edge(const double* __restrict__ Xs, const double* __restrict__ Xt, const double* __restrict__ Tk,
                        const double* __restrict__ Lm, bool uncertain, double mu, bool full, double* __restrict__ rec,
                        double& cost) {
  double Rs[3][3], ts[3], Rt[3][3], tt[3], Rk[3][3], tk[3];
  pg_load(Xs, Rs, ts);
  pg_load(Xt, Rt, tt);
  pg_load(Tk, Rk, tk);
  // X_t^-1 X_s = [Rt^T Rs, Rt^T (ts - tt)]: the difference first, so a graph far from the origin loses nothing
  double Rr[3][3], tr[3], Rd[3][3], td[3], e[6];
  pg_mul_tn(Rt, Rs, Rr);
  const double d0 = ts[0] - tt[0], d1 = ts[1] - tt[1], d2 = ts[2] - tt[2];
#pragma unroll
  for (int a = 0; a < 3; a++) tr[a] = (Rt[0][a] * d0 + Rt[1][a] * d1) + Rt[2][a] * d2;
  // D = T^-1 (X_t^-1 X_s), T^-1 = [Rk^T, -Rk^T tk]
  pg_mul_tn(Rk, Rr, Rd);
#pragma unroll
  for (int a = 0; a < 3; a++)
    td[a] = ((Rk[0][a] * tr[0] + Rk[1][a] * tr[1]) + Rk[2][a] * tr[2]) - ((Rk[0][a] * tk[0] + Rk[1][a] * tk[1]) + Rk[2][a] * tk[2]);
  pg_vec6(Rd, td, e);
  double Le[6], r = 0.0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) v += Lm[6 * a + b] * e[b];
    Le[a] = v;
  }
#pragma unroll
  for (int a = 0; a < 6; a++) r += e[a] * Le[a];
  double w = 1.0, c = r;
  if (uncertain) {      // the line process at its optimum (Geman-McClure)
    const double q = mu / (mu + r);
    w = q * q;
    c = mu * r / (mu + r);
  }
  cost += c;
#pragma unroll
  for (int a = 0; a < 6; a++) rec[a] = e[a];
  rec[6] = r;
  rec[7] = w;
  if (!full) return;
  // column j of J = lin6(T^-1 X_t^-1 G_j X_s); Ra = Rk^T Rt^T
  double Ra[3][3], J[6][6];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Ra[a][b] = (Rk[0][a] * Rt[b][0] + Rk[1][a] * Rt[b][1]) + Rk[2][a] * Rt[b][2];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double P[3][3], M[3][3], c3[3];      // P = S_j Rs, M = Ra P
#pragma unroll
    for (int b = 0; b < 3; b++) {
      pg_cross_axis(j, Rs[0][b], Rs[1][b], Rs[2][b], c3);
      P[0][b] = c3[0]; P[1][b] = c3[1]; P[2][b] = c3[2];
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) M[a][b] = (Ra[a][0] * P[0][b] + Ra[a][1] * P[1][b]) + Ra[a][2] * P[2][b];
    J[0][j] = (M[2][1] - M[1][2]) * 0.5;
    J[1][j] = (M[0][2] - M[2][0]) * 0.5;
    J[2][j] = (M[1][0] - M[0][1]) * 0.5;
    pg_cross_axis(j, ts[0], ts[1], ts[2], c3);
#pragma unroll
    for (int a = 0; a < 3; a++) J[3 + a][j] = (Ra[a][0] * c3[0] + Ra[a][1] * c3[1]) + Ra[a][2] * c3[2];
    // the translations
#pragma unroll
    for (int a = 0; a < 3; a++) {
      J[a][3 + j] = 0.0;
      J[3 + a][3 + j] = Ra[a][j];
    }
  }
  // W = w J^T Lambda J (upper triangle), g = w J^T Lambda e
  double LJ[6][6];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c2 = 0; c2 < 6; c2++) {
      double v = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) v += Lm[6 * a + b] * J[b][c2];
      LJ[a][c2] = v;
    }
  int o = 8;
#pragma unroll
  for (int c1 = 0; c1 < 6; c1++)
#pragma unroll
    for (int c2 = c1; c2 < 6; c2++) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) v += J[a][c1] * LJ[a][c2];
      rec[o++] = w * v;
    }
#pragma unroll
  for (int c1 = 0; c1 < 6; c1++) {
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) v += J[a][c1] * Le[a];
    rec[29 + c1] = w * v;
  }
}

// every edge at the poses X -> F (in every thread)
__device__ double pg_edges(const PgCtx& C, const double* __restrict__ X, bool full) {
  double cost = 0.0;
  for (int k = threadIdx.x; k < C.E; k += 256)
    pg_edge(X + 16 * (size_t)C.es[k], X + 16 * (size_t)C.et[k], C.eT + 16 * (size_t)k, C.eL + 36 * (size_t)k, C.unc[k] != 0, C.mu,
            full, C.erec + (size_t)PG_EDGE * k, cost);
  return pg_sum(cost);
}

// H_ii and b of every node from the edge records, incident edges in ascending index -> max diag(H) (in every thread)
__device__ double pg_nodes(const PgCtx& C) {
  double md = 0.0;
  for (int i = threadIdx.x; i < C.N; i += 256) {
    double acc[PG_NODE];
#pragma unroll
    for (int a = 0; a < PG_NODE; a++) acc[a] = 0.0;
    if (!C.fixed[i]) {
      for (int q = C.ptr[i]; q < C.ptr[i + 1]; q++) {
        const int code = C.adj[q];
        const double* rec = C.erec + (size_t)PG_EDGE * (code >> 1);
        const double sg = (code & 1) ? -1.0 : 1.0;      // delta_t enters with -J
#pragma unroll
        for (int a = 0; a < 21; a++) acc[a] += rec[8 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += sg * rec[29 + a];
      }
      md = fmax(md, fmax(fmax(acc[0], acc[6]), fmax(fmax(acc[11], acc[15]), fmax(acc[18], acc[20]))));
    }
#pragma unroll
    for (int a = 0; a < PG_NODE; a++) C.nrec[(size_t)PG_NODE * i + a] = acc[a];
  }
  return pg_max(md);
}

// the factor of H_ii + lam I of one node into f[21] (L below the diagonal row by row, then D); false: a rejected pivot
__device__ bool pg_factor_node(const double* __restrict__ H, double lam, double* __restrict__ f) {
  double A[6][6], L[6][6], D[6];
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) {
      const double v = H[o++] + (a == b ? lam : 0.0);
      A[a][b] = v;
      A[b][a] = v;
    }
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) L[a][b] = 0.0;
  if (!gsr_ldlt6_factor(A, L, D)) return false;
  if (f) {
    o = 0;
#pragma unroll
    for (int a = 1; a < 6; a++)
#pragma unroll
      for (int b = 0; b < a; b++) f[o++] = L[a][b];
#pragma unroll
    for (int a = 0; a < 6; a++) f[15 + a] = D[a];
  }
  return true;
}
// z = (H_ii + lam I)^-1 r from the stored factor
__device__ void pg_precondition(const double* __restrict__ f, const double (&r)[6], double (&z)[6]) {
  double L[6][6], D[6];
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) L[a][b] = 0.0;
#pragma unroll
  for (int a = 1; a < 6; a++)
#pragma unroll
    for (int b = 0; b < a; b++) L[a][b] = f[o++];
#pragma unroll
  for (int a = 0; a < 6; a++) D[a] = f[15 + a];
  gsr_ldlt6_solve(L, D, r, z);
}
__device__ __forceinline__ void pg_ld6(const double* __restrict__ p, double (&v)[6]) {
#pragma unroll
  for (int a = 0; a < 6; a++) v[a] = p[a];
}
__device__ __forceinline__ void pg_st6(double* __restrict__ p, const double (&v)[6]) {
#pragma unroll
  for (int a = 0; a < 6; a++) p[a] = v[a];
}
__device__ __forceinline__ double pg_dot6(const double (&a)[6], const double (&b)[6]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) s += a[k] * b[k];
  return s;
}
__device__ void pg_zero_x(const PgCtx& C) {
  for (int i = threadIdx.x; i < C.N; i += 256)
#pragma unroll
    for (int a = 0; a < 6; a++) C.x[6 * (size_t)i + a] = 0.0;
  __syncthreads();
}

// Whether a free node's H_ii alone fails the pivot rule: a node that its edges do not fix (lam I would hide it from the factorisation
// of H_ii + lam I).  Once per linearisation; the same answer in every thread.
__device__ bool pg_unfixed(const PgCtx& C) {
  int bad = 0;
  for (int i = threadIdx.x; i < C.N; i += 256)
    if (!C.fixed[i] && !pg_factor_node(C.nrec + (size_t)PG_NODE * i, 0.0, nullptr)) bad = 1;
  return __syncthreads_or(bad) != 0;
}

// (H + lam I) x = -b over the free nodes by preconditioned conjugate gradients from x = 0; the rows of fixed nodes stay 0.
// -> 0: |r| <= rtol |b| reached, 1: cg_max_iteration reached, 2: a rejected pivot or a direction with p.Ap not > 0 (x = 0)
__device__ int pg_pcg(const PgCtx& C, double lam, double rtol, int maxit, int& iters, double& rel) {
  iters = 0;
  rel = 0.0;
  // (a node that its edges do not fix was found by pg_unfixed, once per linearisation: here H_ii + lam I is factored)
  int bad = 0;
  for (int i = threadIdx.x; i < C.N; i += 256) {
    if (C.fixed[i]) continue;
    const double* H = C.nrec + (size_t)PG_NODE * i;
    if (!pg_factor_node(H, lam, C.fac + 21 * (size_t)i)) bad = 1;
  }
  if (__syncthreads_or(bad)) {
    pg_zero_x(C);
    return 2;
  }
  double bb = 0.0, rz = 0.0;
  for (int i = threadIdx.x; i < C.N; i += 256) {
    double r[6], z[6], zero[6];
#pragma unroll
    for (int a = 0; a < 6; a++) { zero[a] = 0.0; r[a] = 0.0; z[a] = 0.0; }
    if (!C.fixed[i]) {
#pragma unroll
      for (int a = 0; a < 6; a++) r[a] = -C.nrec[(size_t)PG_NODE * i + 21 + a];
      pg_precondition(C.fac + 21 * (size_t)i, r, z);
      bb += pg_dot6(r, r);
      rz += pg_dot6(r, z);
    }
    pg_st6(C.x + 6 * (size_t)i, zero);
    pg_st6(C.r + 6 * (size_t)i, r);
    pg_st6(C.p + 6 * (size_t)i, z);
  }
  bb = pg_sum(bb);
  rz = pg_sum(rz);
  if (!(bb > 0.0)) return bb == 0.0 ? 0 : 2;      // b = 0: x = 0 is the answer; a NaN: no answer
  const double bn = sqrt(bb);
  int status = 1;
  for (int it = 1; it <= maxit; it++) {
    // Ap: the node's own block, then -W_k p_j over its edges to free nodes, ascending k
    double pAp = 0.0;
    for (int i = threadIdx.x; i < C.N; i += 256) {
      if (C.fixed[i]) continue;
      double p[6], y[6];
      pg_ld6(C.p + 6 * (size_t)i, p);
#pragma unroll
      for (int a = 0; a < 6; a++) y[a] = lam * p[a];
      pg_sym_mul(C.nrec + (size_t)PG_NODE * i, p, y, 1.0);
      for (int q = C.ptr[i]; q < C.ptr[i + 1]; q++) {
        const int code = C.adj[q], k = code >> 1;
        const int j = (code & 1) ? C.es[k] : C.et[k];
        if (C.fixed[j]) continue;
        double pj[6];
        pg_ld6(C.p + 6 * (size_t)j, pj);
        pg_sym_mul(C.erec + (size_t)PG_EDGE * k + 8, pj, y, -1.0);
      }
      pg_st6(C.Ap + 6 * (size_t)i, y);
      pAp += pg_dot6(p, y);
    }
    pAp = pg_sum(pAp);
    if (!(pAp > 0.0)) {
      pg_zero_x(C);
      return 2;
    }
    const double alpha = rz / pAp;
    double rr = 0.0;
    for (int i = threadIdx.x; i < C.N; i += 256) {
      if (C.fixed[i]) continue;
      double x[6], r[6], p[6], y[6];
      pg_ld6(C.x + 6 * (size_t)i, x);
      pg_ld6(C.r + 6 * (size_t)i, r);
      pg_ld6(C.p + 6 * (size_t)i, p);
      pg_ld6(C.Ap + 6 * (size_t)i, y);
#pragma unroll
      for (int a = 0; a < 6; a++) {
        x[a] += alpha * p[a];
        r[a] -= alpha * y[a];
      }
      pg_st6(C.x + 6 * (size_t)i, x);
      pg_st6(C.r + 6 * (size_t)i, r);
      rr += pg_dot6(r, r);
    }
    rr = pg_sum(rr);
    iters = it;
    rel = sqrt(rr) / bn;
    if (rel <= rtol) {
      status = 0;
      break;
    }
    double rzn = 0.0;
    for (int i = threadIdx.x; i < C.N; i += 256) {
      if (C.fixed[i]) continue;
      double r[6], z[6];
      pg_ld6(C.r + 6 * (size_t)i, r);
      pg_precondition(C.fac + 21 * (size_t)i, r, z);
      pg_st6(C.z + 6 * (size_t)i, z);
      rzn += pg_dot6(r, z);
    }
    rzn = pg_sum(rzn);
    const double beta = rzn / rz;
    rz = rzn;
    for (int i = threadIdx.x; i < C.N; i += 256) {
      if (C.fixed[i]) continue;
      double z[6], p[6];
      pg_ld6(C.z + 6 * (size_t)i, z);
      pg_ld6(C.p + 6 * (size_t)i, p);
#pragma unroll
      for (int a = 0; a < 6; a++) p[a] = z[a] + beta * p[a];
      pg_st6(C.p + 6 * (size_t)i, p);
    }
    __syncthreads();      // every p before the next product reads its neighbours'
  }
  return status;
}

// ---- the three kernels ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pg_linearize(PgCtx C, const double* __restrict__ X, double* __restrict__ scalars) {
  const double F = pg_edges(C, X, true);
  const double md = pg_nodes(C);
  if (threadIdx.x == 0) {
    scalars[0] = F;
    scalars[1] = md;
  }
}

__global__ __launch_bounds__(256) void k_pg_solve(PgCtx C, double lam, double rtol, int maxit, double* __restrict__ stats) {
  int iters;
  double rel;
  int status = 2;
  if (pg_unfixed(C)) {
    iters = 0;
    rel = 0.0;
    pg_zero_x(C);
  } else {
    status = pg_pcg(C, lam, rtol, maxit, iters, rel);
  }
  if (threadIdx.x == 0) {
    stats[0] = (double)iters;
    stats[1] = rel;
    stats[2] = (double)status;
    stats[3] = 0.0;
  }
}

struct PgOpt {
  int max_iteration, cg_max_iteration;
  double min_rel_increment, min_rel_residual, cg_rtol;
};

__global__ __launch_bounds__(256) void k_pg_optimize(PgCtx C, PgOpt O, double* __restrict__ X, double* __restrict__ w_out,
                                                     double* __restrict__ r_out, double* __restrict__ stats) {
  double F = pg_edges(C, X, true);
  const double F0 = F;
  double lam = 1e-5 * pg_nodes(C), nu = 2.0, cg_worst = 0.0;
  bool unfixed = pg_unfixed(C);
  int status = GSR_PG_MAX_ITERATION, iterations = 0, accepted = 0;
  long long cg_total = 0;
  if (F == 0.0) status = GSR_PG_ZERO_RESIDUAL;
  for (int it = 0; it < O.max_iteration && F != 0.0; it++) {
    int cgi;
    double rel;
    if (unfixed) {
      status = GSR_PG_SOLVER_FAILED;
      break;
    }
    const int st = pg_pcg(C, lam, O.cg_rtol, O.cg_max_iteration, cgi, rel);
    cg_total += cgi;
    cg_worst = fmax(cg_worst, rel);
    if (st == 2) {
      status = GSR_PG_SOLVER_FAILED;
      break;
    }
    iterations++;
    // |delta|_inf against |x|_inf, delta^T (lam delta - b), and the candidate poses M(delta_i) X_i
    double dinf = 0.0, xinf = 0.0, den = 0.0;
    for (int i = threadIdx.x; i < C.N; i += 256) {
      double d[6], R[3][3], t[3], v[6], Xi[16];
      pg_ld6(C.x + 6 * (size_t)i, d);
#pragma unroll
      for (int a = 0; a < 16; a++) Xi[a] = X[16 * (size_t)i + a];
      pg_load(Xi, R, t);
      pg_vec6(R, t, v);
#pragma unroll
      for (int a = 0; a < 6; a++) {
        dinf = fmax(dinf, fabs(d[a]));
        xinf = fmax(xinf, fabs(v[a]));
        den += d[a] * (lam * d[a] - C.nrec[(size_t)PG_NODE * i + 21 + a]);
      }
      if (!C.fixed[i]) {      // (a fixed node's delta is 0: its pose is copied, bit for bit)
        double dR[3][3], td[3];
        gsr_rotation6(d, dR);
        td[0] = d[3]; td[1] = d[4]; td[2] = d[5];
        gsr_rigid_left6(dR, td, Xi);
      }
#pragma unroll
      for (int a = 0; a < 16; a++) C.Xn[16 * (size_t)i + a] = Xi[a];
    }
    dinf = pg_max(dinf);
    xinf = pg_max(xinf);
    den = pg_sum(den);
    if (dinf <= O.min_rel_increment * (xinf + O.min_rel_increment)) {
      status = GSR_PG_CONVERGED_STEP;
      break;
    }
    const double Fn = pg_edges(C, C.Xn, false);
    const double rho = (F - Fn) / den;
    if (Fn < F) {
      for (int i = threadIdx.x; i < C.N; i += 256) {
        if (C.fixed[i]) continue;
#pragma unroll
        for (int a = 0; a < 16; a++) X[16 * (size_t)i + a] = C.Xn[16 * (size_t)i + a];
      }
      __syncthreads();
      accepted++;
      const bool small = F - Fn <= O.min_rel_residual * F;
      F = Fn;
      const double q = 2.0 * rho - 1.0;
      lam *= fmax(1.0 / 3.0, 1.0 - q * q * q);
      nu = 2.0;
      if (small) {
        status = GSR_PG_CONVERGED_RESIDUAL;
        break;
      }
      if (F == 0.0) {
        status = GSR_PG_ZERO_RESIDUAL;
        break;
      }
      pg_edges(C, X, true);
      pg_nodes(C);
      unfixed = pg_unfixed(C);
    } else {
      lam *= nu;
      nu *= 2.0;
    }
    if (!(fabs(lam) <= 1e32)) {      // (false for NaN and the infinities too)
      status = GSR_PG_LAMBDA;
      break;
    }
  }
  // r and w of every edge at the poses that are returned
  pg_edges(C, X, false);
  for (int k = threadIdx.x; k < C.E; k += 256) {
    r_out[k] = C.erec[(size_t)PG_EDGE * k + 6];
    w_out[k] = C.erec[(size_t)PG_EDGE * k + 7];
  }
  if (threadIdx.x == 0) {
    stats[0] = (double)status;
    stats[1] = (double)iterations;
    stats[2] = (double)accepted;
    stats[3] = F0;
    stats[4] = F;
    stats[5] = lam;
    stats[6] = (double)cg_total;
    stats[7] = cg_worst;
    for (int a = 8; a < 16; a++) stats[a] = 0.0;
  }
}

// ---- information matrix -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_info_partial(uint32_t Ps, uint32_t Pt, const float* __restrict__ target,
                                                      const int32_t* __restrict__ idx, double* __restrict__ part) {
  double s[PG_INFO_SUMS];
#pragma unroll
  for (int a = 0; a < PG_INFO_SUMS; a++) s[a] = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < Ps; i += gridDim.x * 256u) {
    const int32_t k = idx[i];
    if (k < 0 || (uint32_t)k >= Pt) continue;
    const float fx = target[3 * (size_t)k], fy = target[3 * (size_t)k + 1], fz = target[3 * (size_t)k + 2];
    if (!(knn_finite(fx) && knn_finite(fy) && knn_finite(fz))) continue;
    const double x = fx, y = fy, z = fz;
    // G_1 = [0, z, -y, 1, 0, 0], G_2 = [-z, 0, x, 0, 1, 0], G_3 = [y, -x, 0, 0, 0, 1]: the upper triangle of their G^T G
    const double G[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    s[0] += 1.0;
    int o = 1;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++) {
        s[o] += (G[0][a] * G[0][b] + G[1][a] * G[1][b]) + G[2][a] * G[2][b];
        o++;
      }
  }
  gsr_block_sum_store(s, part);
}
__global__ __launch_bounds__(256) void k_info_final(uint32_t nblk, const double* __restrict__ part, double* __restrict__ info,
                                                    double* __restrict__ stats) {
  double s[PG_INFO_SUMS];
  gsr_block_sum_rows(s, part, nblk);
  if (threadIdx.x != 0) return;
  int o = 1;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) {
      info[6 * a + b] = s[o];
      info[6 * b + a] = s[o];
      o++;
    }
  stats[0] = s[0];
  stats[1] = stats[2] = stats[3] = 0.0;
}

PgCtx pg_ctx(int64_t N, int64_t E, const void* topo, const double* eT, const double* eL, const uint8_t* unc, double mu,
             double* erec, double* nrec, void* workspace) {
  const PgTopo t = pg_topo(topo, (size_t)N, (size_t)E);
  const PgWs w = pg_ws(workspace, (size_t)N, (size_t)E);      // (no workspace: every span NULL)
  PgCtx C;
  C.N = (int)N; C.E = (int)E;
  C.es = t.s; C.et = t.t; C.ptr = t.ptr; C.adj = t.adj; C.fixed = t.fixed;
  C.eT = eT; C.eL = eL; C.unc = unc; C.mu = mu;
  C.erec = erec ? erec : w.erec;
  C.nrec = nrec ? nrec : w.nrec;
  C.fac = w.fac; C.x = w.x; C.r = w.r; C.z = w.z; C.p = w.p; C.Ap = w.Ap; C.Xn = w.Xn;
  return C;
}

}  // namespace

extern "C" size_t gsr_information_workspace_bytes(int64_t Ps) {
  (void)Ps;      // (the partial sums of at most GSR_GN_BLOCKS workgroups: the size does not grow with the cloud)
  return gn_ws(nullptr, PG_INFO_SUMS, false).total;
}

extern "C" int gsr_registration_information(int64_t Pt, const float* target, int64_t Ps, const int32_t* idx, double* info_out,
                                            double* stats_dev, void* workspace, size_t workspace_bytes, void* stream) {
  if (gsr_bad_size(Pt) || gsr_bad_size(Ps) || !target || !idx || !info_out || !stats_dev || !workspace) {
    gsr_set_error("registration_information: bad arguments (Pt = %lld, Ps = %lld, or a NULL pointer)", (long long)Pt, (long long)Ps);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const GsrGnWs w = gn_ws(workspace, PG_INFO_SUMS, false);      // (the rows of partial sums of solve6_common.h, no shift)
  if (!gsr_workspace_fits("registration_information", workspace, workspace_bytes, w.total)) return GSR_ERR_STATE_TOO_SMALL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nblk = gn_partial_blocks((uint32_t)Ps);
  GSR_LAUNCH("information_partial", k_info_partial, dim3(nblk), dim3(256), 0, st, (uint32_t)Ps, (uint32_t)Pt, target, idx,
             w.part);
  GSR_LAUNCH("information_final", k_info_final, dim3(1), dim3(256), 0, st, nblk, (const double*)w.part, info_out, stats_dev);
  return gsr_launch_status("registration_information launch");
}

extern "C" size_t gsr_posegraph_topology_bytes(int64_t N, int64_t E) {
  if (pg_bad_sizes(N, E)) return 0;
  return pg_topo(nullptr, (size_t)N, (size_t)E).total;
}

extern "C" int gsr_posegraph_topology(int64_t N, int64_t E, const int32_t* edges_host, const uint8_t* fixed_host,
                                      void* host_scratch, void* topology, size_t topology_bytes, void* stream) {
  if (pg_bad_sizes(N, E) || (E > 0 && !edges_host) || !fixed_host || !host_scratch || !topology) {
    gsr_set_error("posegraph_topology: bad arguments (N = %lld, E = %lld, or a NULL pointer)", (long long)N, (long long)E);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  for (int64_t k = 0; k < E; k++) {
    const int32_t s = edges_host[2 * k], t = edges_host[2 * k + 1];
    if (s < 0 || s >= N || t < 0 || t >= N || s == t) {
      gsr_set_error("posegraph_topology: edge %lld joins %d and %d: expected two different nodes in [0, %lld)", (long long)k, (int)s,
                    (int)t, (long long)N);
      return GSR_ERR_INVALID_ARGUMENT;
    }
  }
  const PgTopo L = pg_topo(host_scratch, (size_t)N, (size_t)E);      // (filled on the host, copied whole)
  if (!gsr_workspace_fits("posegraph_topology", topology, topology_bytes, L.total, "topology")) return GSR_ERR_STATE_TOO_SMALL;
  // the CSR, built once in the caller's host scratch: node_ptr[N + 1], node_edge[2E] = 2 k + (1 where the node is edge k's
  // target), k ascending.  node_ptr[i] serves as node i's fill cursor and is shifted back afterwards: no second array.
  int32_t *hs = L.s, *ht = L.t, *hp = L.ptr, *ha = L.adj, *hf = L.fixed;
  for (int64_t i = 0; i <= N; i++) hp[i] = 0;
  for (int64_t k = 0; k < E; k++) {
    hs[k] = edges_host[2 * k];
    ht[k] = edges_host[2 * k + 1];
    hp[hs[k] + 1]++;
    hp[ht[k] + 1]++;
  }
  for (int64_t i = 0; i < N; i++) {
    hp[i + 1] += hp[i];
    hf[i] = fixed_host[i] ? 1 : 0;
  }
  for (int64_t k = 0; k < E; k++) {
    ha[hp[hs[k]]++] = (int32_t)(2 * k);
    ha[hp[ht[k]]++] = (int32_t)(2 * k + 1);
  }
  for (int64_t i = N; i > 0; i--) hp[i] = hp[i - 1];      // (every cursor ended at its node's end = the next node's start)
  hp[0] = 0;
  return gsr_check(hipMemcpyAsync(topology, host_scratch, L.total, hipMemcpyHostToDevice, (hipStream_t)stream), "posegraph_topology copy");
}

extern "C" size_t gsr_posegraph_workspace_bytes(int64_t N, int64_t E) {
  if (pg_bad_sizes(N, E)) return 0;
  return pg_ws(nullptr, (size_t)N, (size_t)E).total;
}

extern "C" int gsr_posegraph_linearize(int64_t N, int64_t E, const void* topology, const double* poses, const double* edge_T,
                                       const double* edge_info, const uint8_t* edge_uncertain, double mu, double* edge_out,
                                       double* node_out, double* scalars_out, void* stream) {
  if (pg_bad_sizes(N, E) || !topology || !poses || !node_out || !scalars_out ||
      (E > 0 && (!edge_T || !edge_info || !edge_uncertain || !edge_out)) || !(mu > 0.0)) {
    gsr_set_error("posegraph_linearize: bad arguments (N = %lld, E = %lld, mu = %g: expected > 0, or a NULL pointer)", (long long)N,
                  (long long)E, mu);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  const PgCtx C = pg_ctx(N, E, topology, edge_T, edge_info, edge_uncertain, mu, edge_out, node_out, nullptr);
  GSR_LAUNCH("posegraph_linearize", k_pg_linearize, dim3(1), dim3(256), 0, (hipStream_t)stream, C, poses, scalars_out);
  return gsr_launch_status("posegraph_linearize launch");
}

extern "C" int gsr_posegraph_solve(int64_t N, int64_t E, const void* topology, const double* edge_rec, const double* node_rec,
                                   double lambda, double cg_rtol, int32_t cg_max_iteration, double* delta_out, double* stats_dev,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (pg_bad_sizes(N, E) || !topology || !node_rec || (E > 0 && !edge_rec) || !delta_out || !stats_dev || !workspace ||
      !(lambda >= 0.0) || !(lambda <= 1e300) || !(cg_rtol >= 0.0) || cg_max_iteration < 1) {
    gsr_set_error("posegraph_solve: bad arguments (N = %lld, E = %lld, lambda = %g: expected finite, >= 0, cg_rtol = %g: expected "
                  ">= 0, cg_max_iteration = %d: expected >= 1, or a NULL pointer)", (long long)N, (long long)E, lambda, cg_rtol,
                  (int)cg_max_iteration);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!gsr_workspace_fits("posegraph_solve", workspace, workspace_bytes, gsr_posegraph_workspace_bytes(N, E)))
    return GSR_ERR_STATE_TOO_SMALL;
  PgCtx C = pg_ctx(N, E, topology, nullptr, nullptr, nullptr, 1.0, const_cast<double*>(edge_rec), const_cast<double*>(node_rec),
                   workspace);
  C.x = delta_out;
  GSR_LAUNCH("posegraph_solve", k_pg_solve, dim3(1), dim3(256), 0, (hipStream_t)stream, C, lambda, cg_rtol, (int)cg_max_iteration,
             stats_dev);
  return gsr_launch_status("posegraph_solve launch");
}

extern "C" int gsr_posegraph_optimize(int64_t N, int64_t E, const void* topology, double* poses, const double* edge_T,
                                      const double* edge_info, const uint8_t* edge_uncertain, double mu, int32_t max_iteration,
                                      double min_relative_increment, double min_relative_residual_increment, double cg_rtol,
                                      int32_t cg_max_iteration, double* edge_w_out, double* edge_r_out, double* stats_dev,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (pg_bad_sizes(N, E) || !topology || !poses || !stats_dev || !workspace ||
      (E > 0 && (!edge_T || !edge_info || !edge_uncertain || !edge_w_out || !edge_r_out))) {
    gsr_set_error("posegraph_optimize: bad arguments (N = %lld, E = %lld, or a NULL pointer)", (long long)N, (long long)E);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!(mu > 0.0) || max_iteration < 0 || !(min_relative_increment >= 0.0) || !(min_relative_residual_increment >= 0.0) ||
      !(cg_rtol >= 0.0) || cg_max_iteration < 1) {
    gsr_set_error("posegraph_optimize: bad arguments (mu = %g: expected > 0; max_iteration = %d: expected >= 0; increments %g, %g "
                  "and cg_rtol = %g: expected >= 0; cg_max_iteration = %d: expected >= 1)", mu, (int)max_iteration,
                  min_relative_increment, min_relative_residual_increment, cg_rtol, (int)cg_max_iteration);
    return GSR_ERR_INVALID_ARGUMENT;
  }
  if (!gsr_workspace_fits("posegraph_optimize", workspace, workspace_bytes, gsr_posegraph_workspace_bytes(N, E)))
    return GSR_ERR_STATE_TOO_SMALL;
  const PgCtx C = pg_ctx(N, E, topology, edge_T, edge_info, edge_uncertain, mu, nullptr, nullptr, workspace);
  PgOpt O;
  O.max_iteration = max_iteration; O.cg_max_iteration = cg_max_iteration;
  O.min_rel_increment = min_relative_increment; O.min_rel_residual = min_relative_residual_increment; O.cg_rtol = cg_rtol;
  GSR_LAUNCH("posegraph_optimize", k_pg_optimize, dim3(1), dim3(256), 0, (hipStream_t)stream, C, O, poses, edge_w_out, edge_r_out,
             stats_dev);
  return gsr_launch_status("posegraph_optimize launch");
}
