// SE(3) pose arithmetic of the tracking loop on the device (include/gsr.h, gsr_pose_forward / gsr_pose_backward).
//
// The camera of a tracking iteration is W2C' = exp(tau) W2C (scene_utils/pose.py): a base matrix, a six-component twist and the
// projection matrix, all float64 in device memory.  One launch turns them into the three float32 tensors the rasterizer reads,
// one launch turns the rasterizer's three camera gradients into dL/dtau - and, when asked, applies the Adam step to tau in the
// same launch.  About a hundred float64 operations each: what matters is that there is ONE launch and no host in between, not
// throughput, so each kernel is a single wave in which every lane that takes part runs the whole (straight-line) chain on its own
// and then writes the entries it owns: no LDS hand-off but one, no atomics, bitwise reproducible.
#include "gsr_common.h"

namespace {

// A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 of t = |theta|, and a1, b1, c1 = (1 / t) d{A, B, C}/dt (so that
// d{A, B, C}/dtheta_k = theta_k {a1, b1, c1}).  The small-angle rule is scene_utils.pose.se3_exp's: below |theta|^2 = 1e-6 the
// Taylor polynomials in t^2 (their derivatives are those of the polynomials, what autograd gives on the host), above it the closed
// forms with 1 - cos t = 2 sin^2(t / 2).  The derivatives use 1 - A = t^2 C: a1 = C - B, b1 = (A - 2 B) / t^2, c1 = (B - 3 C) / t^2.
struct Se3Coef {
  double A, B, C, a1, b1, c1;
};

__device__ __forceinline__ Se3Coef se3_coef(const double t2) {
  Se3Coef k;
  if (t2 < 1e-6) {
    k.A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
    k.B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    k.C = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
    k.a1 = -1.0 / 3.0 + t2 / 30.0;
    k.b1 = -1.0 / 12.0 + t2 / 180.0;
    k.c1 = -1.0 / 60.0 + t2 / 1260.0;
  } else {
    const double t = sqrt(t2), s = sin(t), h = sin(0.5 * t);
    k.A = s / t;
    k.B = 2.0 * h * h / t2;
    k.C = (t - s) / (t2 * t);
    k.a1 = k.C - k.B;
    k.b1 = (k.A - 2.0 * k.B) / t2;
    k.c1 = (k.B - 3.0 * k.C) / t2;
  }
  return k;
}

// K = hat(w), K2 = K K (row-major 3x3)
__device__ __forceinline__ void hat_and_square(const double* w, double* K, double* K2) {
  K[0] = 0.0;   K[1] = -w[2]; K[2] = w[1];
  K[3] = w[2];  K[4] = 0.0;   K[5] = -w[0];
  K[6] = -w[1]; K[7] = w[0];  K[8] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
}

// The pieces of exp(tau) = [[R, V rho], [0, 1]]: R = I + A K + B K^2, V = I + B K + C K^2.
struct Se3 {
  Se3Coef k;
  double K[9], K2[9], R[9], V[9], u[3];   // u = V rho
};

__device__ __forceinline__ void se3_exp(const double* tau, Se3& e) {
  const double* rho = tau;
  const double* th = tau + 3;
  e.k = se3_coef(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
  hat_and_square(th, e.K, e.K2);
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const double eye = (i % 4 == 0) ? 1.0 : 0.0;
    e.R[i] = eye + e.k.A * e.K[i] + e.k.B * e.K2[i];
    e.V[i] = eye + e.k.B * e.K[i] + e.k.C * e.K2[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) e.u[i] = e.V[3 * i] * rho[0] + e.V[3 * i + 1] * rho[1] + e.V[3 * i + 2] * rho[2];
}

// T = exp(tau) base: rows 0..2 (the bottom row is base's own, (0, 0, 0, 1) for a rigid pose)
__device__ __forceinline__ void pose_T(const Se3& e, const double* base, double* T /*16*/) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
      T[4 * i + j] = e.R[3 * i] * base[j] + e.R[3 * i + 1] * base[4 + j] + e.R[3 * i + 2] * base[8 + j] + e.u[i] * base[12 + j];
#pragma unroll
  for (int j = 0; j < 4; j++) T[12 + j] = base[12 + j];
}

__global__ __launch_bounds__(64) void k_pose_forward(const double* __restrict__ base_w2c, const double* __restrict__ tau_in,
                                                     const double* __restrict__ proj_T, float* __restrict__ viewmatrix,
                                                     float* __restrict__ projmatrix, float* __restrict__ campos) {
  __shared__ double Ts[16];
  if (threadIdx.x == 0) {
    double tau[6], base[16], T[16];
#pragma unroll
    for (int i = 0; i < 6; i++) tau[i] = tau_in[i];
#pragma unroll
    for (int i = 0; i < 16; i++) base[i] = base_w2c[i];
    Se3 e;
    se3_exp(tau, e);
    pose_T(e, base, T);
#pragma unroll
    for (int i = 0; i < 16; i++) Ts[i] = T[i];
  }
  __syncthreads();
  const int l = (int)threadIdx.x;
  if (l < 16) {                      // world_view_transform = T^T
    const int r = l >> 2, c = l & 3;
    viewmatrix[l] = (float)Ts[4 * c + r];
  } else if (l < 32) {               // full_proj_transform = T^T proj_T
    const int r = (l - 16) >> 2, c = l & 3;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) s += Ts[4 * k + r] * proj_T[4 * k + c];
    projmatrix[l - 16] = (float)s;
  } else if (l < 35) {               // camera_center = -R^T t
    const int i = l - 32;
    campos[i] = (float)(-(Ts[i] * Ts[3] + Ts[4 + i] * Ts[7] + Ts[8 + i] * Ts[11]));
  }
}

// Lane k < 6 forms dL/dtau_k; with `adam` it then applies torch.optim.Adam's update (bias correction, no weight decay, no amsgrad)
// to tau_k in place, and lane 0 advances the stored step and learning rate.  Every lane reads tau, the step and the learning rate
// before the barrier and writes behind it.
__global__ __launch_bounds__(64) void k_pose_backward(const double* __restrict__ base_w2c, double* tau_io,
                                                      const double* __restrict__ proj_T, const float* __restrict__ gV,
                                                      const float* __restrict__ gPV, const float* __restrict__ gC,
                                                      double* __restrict__ dL_dtau, gsr_pose_adam* adam) {
  const int k = (int)threadIdx.x;
  double g = 0.0, tau_k = 0.0;
  int64_t step = 0;
  double lr = 0.0;
  if (k < 6) {
    double tau[6], base[16], T[16];
#pragma unroll
    for (int i = 0; i < 6; i++) tau[i] = tau_io[i];
#pragma unroll
    for (int i = 0; i < 16; i++) base[i] = base_w2c[i];
    tau_k = tau_io[k];
    if (adam) { step = adam->step; lr = adam->lr; }
    Se3 e;
    se3_exp(tau, e);
    pose_T(e, base, T);
    // G_T = (gV + gPV proj_T^T)^T, minus the camera centre's part (C = -R^T t): rows 0..2 (the bottom row of T is constant)
    double GT[12];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        double s = gV ? (double)gV[4 * j + i] : 0.0;
        if (gPV) {
#pragma unroll
          for (int c = 0; c < 4; c++) s += (double)gPV[4 * j + c] * proj_T[4 * i + c];
        }
        GT[4 * i + j] = s;
      }
    if (gC) {
      const double c[3] = {(double)gC[0], (double)gC[1], (double)gC[2]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) GT[4 * i + j] -= T[4 * i + 3] * c[j];
        GT[4 * i + 3] -= T[4 * i] * c[0] + T[4 * i + 1] * c[1] + T[4 * i + 2] * c[2];
      }
    }
    // G_E = G_T base^T (rows 0..2)
    double GE[12];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        GE[4 * i + j] = GT[4 * i] * base[4 * j] + GT[4 * i + 1] * base[4 * j + 1] + GT[4 * i + 2] * base[4 * j + 2] +
                        GT[4 * i + 3] * base[4 * j + 3];
    // dL/dtau_k = sum_ij G_E[i][j] dE[i][j]/dtau_k, E = [[R, V rho], [0, 1]], at this tau (the twist is not reset between
    // iterations).  rho_k: dE[:, 3] = V[:, k].  theta_k, with G = hat(e_k) and S = G K + K G:
    //   dR = theta_k (a1 K + b1 K^2) + A G + B S,   dV = theta_k (b1 K + c1 K^2) + B G + C S
    if (k < 3) {
      // (a select per term, not V[3 i + k]: a run-time index would put the array into scratch memory)
#pragma unroll
      for (int i = 0; i < 3; i++) g += GE[4 * i + 3] * (k == 0 ? e.V[3 * i] : (k == 1 ? e.V[3 * i + 1] : e.V[3 * i + 2]));
    } else {
      const double ek[3] = {k == 3 ? 1.0 : 0.0, k == 4 ? 1.0 : 0.0, k == 5 ? 1.0 : 0.0};
      const double thk = k == 3 ? tau[3] : (k == 4 ? tau[4] : tau[5]);
      double G[9], G2[9], S[9];
      hat_and_square(ek, G, G2);
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
          S[3 * i + j] = G[3 * i] * e.K[j] + G[3 * i + 1] * e.K[3 + j] + G[3 * i + 2] * e.K[6 + j] +
                         e.K[3 * i] * G[j] + e.K[3 * i + 1] * G[3 + j] + e.K[3 * i + 2] * G[6 + j];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        double du = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double dR = thk * (e.k.a1 * e.K[3 * i + j] + e.k.b1 * e.K2[3 * i + j]) + e.k.A * G[3 * i + j] + e.k.B * S[3 * i + j];
          const double dV = thk * (e.k.b1 * e.K[3 * i + j] + e.k.c1 * e.K2[3 * i + j]) + e.k.B * G[3 * i + j] + e.k.C * S[3 * i + j];
          g += GE[4 * i + j] * dR;
          du += dV * tau[j];
        }
        g += GE[4 * i + 3] * du;
      }
    }
  }
  __syncthreads();
  if (k >= 6) return;
  if (dL_dtau) dL_dtau[k] = g;
  if (adam) {
    const double b1 = adam->beta1, b2 = adam->beta2;
    const double t = (double)(step + 1);
    const double m = adam->exp_avg[k] + (g - adam->exp_avg[k]) * (1.0 - b1);
    const double v = adam->exp_avg_sq[k] * b2 + (1.0 - b2) * g * g;
    const double step_size = lr / (1.0 - pow(b1, t));
    const double denom = sqrt(v) / sqrt(1.0 - pow(b2, t)) + adam->eps;
    adam->exp_avg[k] = m;
    adam->exp_avg_sq[k] = v;
    tau_io[k] = tau_k - step_size * (m / denom);
    if (k == 0) {
      adam->step = step + 1;
      adam->lr = lr * adam->lr_decay;
    }
  }
}

}  // namespace

extern "C" int gsr_pose_forward(const double* base_w2c, const double* tau, const double* proj_T, float* viewmatrix,
                                float* projmatrix, float* campos, void* stream) {
  if (!base_w2c || !tau || !proj_T || !viewmatrix || !projmatrix || !campos) {
    gsr_set_error("pose forward: null buffer");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  GSR_LAUNCH("pose_fwd", k_pose_forward, dim3(1), dim3(64), 0, (hipStream_t)stream, base_w2c, tau, proj_T, viewmatrix,
             projmatrix, campos);
  return gsr_launch_status("pose forward");
}

extern "C" int gsr_pose_backward(const double* base_w2c, double* tau, const double* proj_T, const float* dL_dviewmatrix,
                                 const float* dL_dprojmatrix, const float* dL_dcampos, double* dL_dtau, gsr_pose_adam* adam,
                                 void* stream) {
  if (!base_w2c || !tau || !proj_T || (!dL_dtau && !adam)) {
    gsr_set_error("pose backward: null buffer (dL_dtau may be NULL only with an Adam state)");
    return GSR_ERR_INVALID_ARGUMENT;
  }
  GSR_LAUNCH("pose_bwd", k_pose_backward, dim3(1), dim3(64), 0, (hipStream_t)stream, base_w2c, tau, proj_T, dL_dviewmatrix,
             dL_dprojmatrix, dL_dcampos, dL_dtau, adam);
  return gsr_launch_status("pose backward");
}
