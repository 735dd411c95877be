// The per-point variational maths every path shares (shard tables, prediction, latent inference, the reference-shaped arrays): one definition each of
// the variance transform, the factors of (alpha_q, S_nq) and the exponent LEA of the factorised psi2.  The header shares the arithmetic, not the table
// layouts: callers keep their own stores and their own running logs, ln c1 -= var_log1 and 1/2 ln c2 -= var_half_log2.
#pragma once
#include <hip/hip_runtime.h>

namespace gp {

// S = softplus(raw) and dS / d raw (transformVar / transformVar_grad, supporting_functions.py:160-168)
__device__ __forceinline__ double softplus(double x) { return log(1.0 + exp(x)); }
__device__ __forceinline__ double softplus_slope(double x) { return 1.0 / (1.0 + exp(-x)); }

// x + a d with the product rounded first, as the reference's NumPy rounds it (local_MapReduce.py:205-211, scg_adapted_local_MapReduce.py:175-214):
// never contracted into a fused multiply-add.  The trial point, grad_latest's variance transform at it, gp_cg_update's update_d and update_X all
// go through here, so the resident vectors follow the reference's files to the bit and do not depend on what the compiler chooses to contract.
__device__ __forceinline__ double mul_then_add(double a, double d, double x) {
#pragma clang fp contract(off)
  const double p = a * d;
  return p + x;
}

// d1 = alpha S + 1, d2 = 2 alpha S + 1, u = alpha / d1 (Psi1), w = alpha / d2 and v2 = (alpha - w) / 2 = -2 V (psi2)
struct VarQ { double d1, d2, u, w, v2; };
__device__ __forceinline__ VarQ var_q(double a, double s) {
  const double d1 = a * s + 1.0, d2 = 2.0 * a * s + 1.0, w = a / d2;
  return VarQ{d1, d2, a / d1, w, 0.5 * (a - w)};
}
// one latent dimension's share of ln c1 = ln sf2 - 1/2 sum_q ln d1 and of 1/2 ln c2 = ln sf2 - 1/4 sum_q ln d2
__device__ __forceinline__ double var_log1(const VarQ& f) { return 0.5 * log(f.d1); }
__device__ __forceinline__ double var_half_log2(const VarQ& f) { return 0.25 * log(f.d2); }

// LE[n][m] = 1/2 ln c2_n - 1/2 s and LEA[n][m] = LE - 1/2 t with s = sum_q w_nq (mu_nq - z_mq)^2, t = sum_q v2_nq z_mq^2 (q ascending)
__device__ __forceinline__ void lea_sums(const double* mu, const double* w, const double* v2, const double* z, int Q, double* s_out, double* t_out) {
  double s = 0.0, t = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double d = mu[q] - z[q];
    s = fma(w[q] * d, d, s);
    t = fma(v2[q] * z[q], z[q], t);
  }
  *s_out = s; *t_out = t;
}
__device__ __forceinline__ double le_value(double l0, double s) { return l0 - 0.5 * s; }
__device__ __forceinline__ double lea_value(double le, double t) { return le - 0.5 * t; }

}  // namespace gp
