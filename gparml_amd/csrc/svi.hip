// Explicit q(u) in the whitened space and the uncollapsed bound (gp_svi_*; include/gparml_hip.h has the formulas, DESIGN.md section 21 the derivation).
//
// u = L_k v, q(v_d) = N(Mv[:, d], Sv), state in natural parameters Lam = Sv^-1 [Mp][Mp] and H = Lam Mv [Mp][Dp].  Everything is padded as the global
// step pads it: K_mm carries an identity block, Psi2 and C zeros, so a = L_k^-1 and Lam carry an identity block too, Psi2w, Cw, H, Mv and every
// partial zeros there, and log-determinants and traces (taken over the leading M) are those of the unpadded problem.
//   front (kept until the statistics or the globals change, Lifecycle::inputs_serial): K_mm (build_kmm_kernel) -> L_k, a (blocked Cholesky and
//     triangular inverse, no K_mm^-1) -> T = a Psi2, Psi2w = T a^T, Cw = a C                                      [3 products]
//   gp_svi_natural_step: one elementwise pass (svi_axpy_kernel)
//   gp_svi_step: Lam -> L_l, L_l^-1, Sv = L_l^-T L_l^-1 (the same driver) -> Mv = Sv H -> W = D Sv + Mv Mv^T -> G2 (elementwise) -> R = 2 G2 Psi2w,
//     R += beta Mv Cw^T -> S = -1/2 (Phi(R) + Phi(R)^T) (elementwise) -> T = G2 a, Bbar = a^T T; Abar = beta a^T Mv; T = S a, dF/dKmm = a^T T -> Bm
//     (elementwise) -> seven traces (the global step's dots kernel) -> scalars -> K_mm parts of grad_Z / grad_alpha (the global step's kernels)
//     [1 + 1 + 2 + 5 products; with the front 12: the collapsed step runs 6 and two double-double ones]
//   gp_svi_publish: X = Lam - I -> T = L_k X, Psi2_eff = T L_k^T / beta; C_eff = L_k H / beta                      [3 products]
// Every M-sized product goes through launch_gemm in plain float64, described once below with its layouts.  The new kernels are elementwise passes and
// one single-workgroup scalar kernel: no LDS beyond the 64-double reduction of the scalars, no scratch, no atomics -- every sum has a fixed order
// (dots_kernel's block partials added in ascending order), so the results are bit-identical from run to run.
// The plan's buffers are DA_RAW: every element is written before it is read (the two inverse factors' upper 128-blocks, never written by the
// factorisation, are zeroed once by gp_svi_begin).
#include "gp_common.h"
#include <cmath>
#include <cstring>

namespace gp {

struct SviPlan {
  DevBuf<double> Lam, H;                  // the state
  DevBuf<double> Lk, a, P2w, Cw;          // the front: L_k, a = L_k^-1, Psi2w, Cw
  DevBuf<double> fsc;                     // [GS_HOST] the front's scalars, laid out as GsState::gs: ln|K_mm| at GS_LOGDET_K, K_mm's failure flag at GS_FLAGS
  DevBuf<double> Ll, Lli, W, Mv, G2, R, S;   // gp_svi_step: L_l, L_l^-1, Sv then D Sv + Mv Mv^T, Mv, G2 (publish: Lam - I), R, S
  DevBuf<double> T;                       // [Mp][max(Mp, Dp)] work panel of the factorisations and the left half of every two-sided product
  DevBuf<double> dg;                      // [3][Mp] diag W | diag Psi2w | ones: the two plain traces as dot jobs
  DevBuf<double> lsc;                     // [8] ln|Lam| and Lam's failure flag
  long front_serial = -1;                 // Lifecycle::inputs_serial the front was computed at; -1: none
  int jitK = 0;                           // 1: K_mm + 1e-7 I (the mask of the last gp_svi_step)
};
void SviPlanDelete::operator()(SviPlan* p) const { delete p; }

// the slots of GsState::gs the four traces of the bound borrow (the collapsed step's traces live there in its own steps)
enum { SVI_TR_MC = GS_TR_KIPSI2, SVI_TR_P2W_W = GS_TR_PPSI2, SVI_TR_W = GS_TR_CE, SVI_TR_P2W = GS_TR_EPSI2E };

// ---- the products, each described once (LA / LB: launch_gemm's layouts of A and B) -------------------------------------------------------------
struct SviOps {
  const double *Psi2, *C;                 // the statistics buffer
  double *stPsi2, *stC;                   // the same, as publish's outputs
  double *Bbar, *Abar, *dFdK;             // GsState's
  SviPlan* p;
  int Mp, Dp;
};
struct T_is_a_Psi2 {       // a [m][k] -> K_CONTIG, Psi2 stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->a, o.Mp}, {o.Psi2, o.Mp}, {o.p->T, o.Mp}, o.Mp); }
};
struct P2w_is_T_at {       // T [m][k] -> K_CONTIG; B(k, c) = a[c][k] -> K_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = K_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->T, o.Mp}, {o.p->a, o.Mp}, {o.p->P2w, o.Mp}, o.Mp); }
};
struct Cw_is_a_C {         // a [m][k] -> K_CONTIG, C stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->a, o.Mp}, {o.C, o.Dp}, {o.p->Cw, o.Dp}, o.Mp); }
};
struct Mv_is_Sv_H {        // Sv (in W) [m][k] -> K_CONTIG, H stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->W, o.Mp}, {o.p->H, o.Dp}, {o.p->Mv, o.Dp}, o.Mp); }
};
struct W_is_DSv_plus_Mv_Mvt {   // W holds Sv: W = Mv Mv^T + D W.  Mv [m][k] -> K_CONTIG; B(k, c) = Mv[c][k] -> K_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = K_CONTIG;
  static GemmP of(const SviOps& o, double Dd) { return gemm_of({o.p->Mv, o.Dp}, {o.p->Mv, o.Dp}, {o.p->W, o.Mp}, o.Dp, 1.0, Dd); }
};
struct R_is_2_G2_P2w {     // G2 [m][k] -> K_CONTIG, Psi2w stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->G2, o.Mp}, {o.p->P2w, o.Mp}, {o.p->R, o.Mp}, o.Mp, 2.0); }
};
struct R_plus_Gc_Cwt {     // Gc = beta Mv: R += beta Mv Cw^T.  Mv [m][k] -> K_CONTIG; B(k, c) = Cw[c][k] -> K_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = K_CONTIG;
  static GemmP of(const SviOps& o, double beta) { return gemm_of({o.p->Mv, o.Dp}, {o.p->Cw, o.Dp}, {o.p->R, o.Mp}, o.Dp, beta, 1.0); }
};
struct T_is_X_a {          // the right half of a^T X a: X [m][k] -> K_CONTIG, a stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o, const double* X) { return gemm_of({X, o.Mp}, {o.p->a, o.Mp}, {o.p->T, o.Mp}, o.Mp); }
};
struct Out_is_at_T {       // the left half: A(i, k) = a[k][i] -> FREE_CONTIG, T stored [k][c] -> FREE_CONTIG (dF/dKmm's sign is in S)
  static constexpr Layout LA = FREE_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o, double* out) { return gemm_of({o.p->a, o.Mp}, {o.p->T, o.Mp}, {out, o.Mp}, o.Mp); }
};
struct Abar_is_at_Gc {     // beta a^T Mv: A(i, k) = a[k][i] -> FREE_CONTIG, Mv stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = FREE_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o, double beta) { return gemm_of({o.p->a, o.Mp}, {o.p->Mv, o.Dp}, {o.Abar, o.Dp}, o.Mp, beta); }
};
struct T_is_Lk_X {         // publish: L_k [m][k] -> K_CONTIG, X = Lam - I (in G2) stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o) { return gemm_of({o.p->Lk, o.Mp}, {o.p->G2, o.Mp}, {o.p->T, o.Mp}, o.Mp); }
};
struct Psi2eff_is_T_Lkt {  // T [m][k] -> K_CONTIG; B(k, c) = L_k[c][k] -> K_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = K_CONTIG;
  static GemmP of(const SviOps& o, double beta) { return gemm_of({o.p->T, o.Mp}, {o.p->Lk, o.Mp}, {o.stPsi2, o.Mp}, o.Mp, 1.0 / beta); }
};
struct Ceff_is_Lk_H {      // L_k [m][k] -> K_CONTIG, H stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static GemmP of(const SviOps& o, double beta) { return gemm_of({o.p->Lk, o.Mp}, {o.p->H, o.Dp}, {o.stC, o.Dp}, o.Mp, 1.0 / beta); }
};
static SviOps svi_ops(gp_ctx* c) {
  const long mm = (long)c->Mp * c->Mp;
  return {c->stats, c->stats + mm, c->stats, c->stats + mm, c->gstep.Bbar, c->gstep.Abar, c->gstep.dFdK, c->svi.get(), c->Mp, c->Dp};
}
template <class P, class... A>
static int svi_gemm(gp_ctx* c, int m, int n, const SviOps& o, A... args) {
  return launch_gemm(c, c->stream, P::LA, P::LB, m, n, 1, P::of(o, args...));
}

// ---- the elementwise kernels ---------------------------------------------------------------------------------------------------------------------
// the prior: Lam = I, H = 0 (padding included)
__global__ void __launch_bounds__(256) svi_prior_kernel(int Mp, int Dp, double* __restrict__ Lam, double* __restrict__ H) {
  const long mm = (long)Mp * Mp, md = (long)Mp * Dp;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < mm + md; idx += (long)gridDim.x * 256L) {
    if (idx < mm) { const long i = idx / Mp, j = idx - i * Mp; Lam[idx] = (i == j) ? 1.0 : 0.0; }
    else H[idx - mm] = 0.0;
  }
}
// the natural step.  Psi2w = (a Psi2) a^T is symmetric up to rounding only: element (i, j) and (j, i) take the same mean of the two, so a symmetric Lam
// stays symmetric bit for bit.  The padded diagonal stays (1 - rho) + rho: 1 up to rounding, and nothing multiplies it with data.
// kfail: K_mm's failure flag of the front.  A K_mm that did not factorise left NaN in Psi2w and Cw: the state is then left as it is (every thread reads the
// same flag), and the gp_svi_step that follows reports K_mm; the caller repeats the natural step once the jittered front stands.
__global__ void __launch_bounds__(256) svi_axpy_kernel(int Mp, int Dp, double rho, double beta, const double* __restrict__ P2w, const double* __restrict__ Cw,
                                                       const double* __restrict__ kfail, double* __restrict__ Lam, double* __restrict__ H) {
  const long mm = (long)Mp * Mp, md = (long)Mp * Dp;
  if (*kfail != 0.0) return;
  const double keep = 1.0 - rho;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < mm + md; idx += (long)gridDim.x * 256L) {
    if (idx < mm) {
      const long i = idx / Mp, j = idx - i * Mp;
      const double p = 0.5 * (P2w[idx] + P2w[j * Mp + i]);
      Lam[idx] = keep * Lam[idx] + rho * ((i == j ? 1.0 : 0.0) + beta * p);
    } else {
      const long e = idx - mm;
      H[e] = keep * H[e] + rho * (beta * Cw[e]);
    }
  }
}
// The assembly, one kernel for its four elementwise passes (the products between them need whole matrices):
//   SVI_COPY: Ll = Lam (the factorisation works in place) and its two scalars zeroed       SVI_X: G2 = Lam - I (publish)
//   SVI_G2:   G2 = 1/2 beta D I - 1/2 beta W, and dg = diag W | diag Psi2w | ones
//   SVI_S:    S = -1/2 (Phi(R) + Phi(R)^T): the lower triangle of R mirrored, times -1/2
//   SVI_BM:   Bm = [2 Bbar ; Abar^T], as assemble_elem lays it out
enum { SVI_COPY = 0, SVI_G2 = 1, SVI_S = 2, SVI_BM = 3, SVI_X = 4 };
struct SviElem {
  const double *Lam, *W, *P2w, *R, *Bbar, *Abar;
  double *Ll, *lsc, *G2, *dg, *S, *Bm;
  double beta, Dd;
  int Mp, Dp;
};
__global__ void __launch_bounds__(256) svi_assemble_kernel(SviElem p, int pass) {
  const int Mp = p.Mp, Dp = p.Dp;
  const long mm = (long)Mp * Mp, total = pass == SVI_BM ? mm + (long)Mp * Dp : mm;
  if (pass == SVI_COPY && blockIdx.x == 0 && threadIdx.x < 8) p.lsc[threadIdx.x] = 0.0;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
    const long i = idx / Mp, j = idx - i * Mp;
    if (pass == SVI_COPY) {
      p.Ll[idx] = p.Lam[idx];
    } else if (pass == SVI_X) {
      p.G2[idx] = p.Lam[idx] - (i == j ? 1.0 : 0.0);
    } else if (pass == SVI_G2) {
      const double w = p.W[idx];
      p.G2[idx] = (i == j ? 0.5 * p.beta * p.Dd : 0.0) - 0.5 * p.beta * w;
      if (i == j) { p.dg[i] = w; p.dg[Mp + i] = p.P2w[idx]; p.dg[2 * Mp + i] = 1.0; }
    } else if (pass == SVI_S) {
      p.S[idx] = -0.5 * (i >= j ? p.R[idx] : p.R[j * Mp + i]);
    } else if (idx < mm) {
      p.Bm[idx] = 2.0 * p.Bbar[idx];
    } else {
      const long e = idx - mm;
      const long m = e / Dp, d = e - m * Dp;
      p.Bm[mm + d * Mp + m] = p.Abar[e];
    }
  }
}
// F = L, grad_beta, grad_sf2, the two log-determinants and the failure flags, from the traces' block partials added in ascending order (as
// scalars_block adds them).  Writes all GS_HOST entries of gs: nothing else of the step touches the scalars.
__global__ void __launch_bounds__(64) svi_scalars_kernel(const double* __restrict__ sc, const double* __restrict__ fsc, const double* __restrict__ lsc,
                                                        DotJobs jobs, const double* __restrict__ part, double beta, double sf2, double Dd, double Nglob,
                                                        double Md, double* __restrict__ gs) {
  __shared__ double tr[GS_COUNT];
  if (threadIdx.x < GS_COUNT) tr[threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x < jobs.n) {
    double s = 0.0;
    for (int b = 0; b < DOT_BLOCKS; ++b) s += part[threadIdx.x * DOT_BLOCKS + b];
    tr[jobs.j[threadIdx.x].slot] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sumYY = sc[SC_SUM_YYT], Psi0 = sc[SC_PSI0], KL = sc[SC_KL];
  const double ldK = fsc[GS_LOGDET_K], ldL = lsc[0];
  const double tMC = tr[SVI_TR_MC], tPW = tr[SVI_TR_P2W_W], tW = tr[SVI_TR_W], tP = tr[SVI_TR_P2W];
  const double two_pi = 6.283185307179586476925286766559;
  const double KLu = 0.5 * tW - 0.5 * Dd * Md + 0.5 * Dd * ldL;       // 1/2 D (tr Sv - M + ln|Lam|) + 1/2 tr(Mv^T Mv), with tr W = D tr Sv + tr(Mv^T Mv)
  for (int i = 0; i < GS_HOST; ++i) gs[i] = i < GS_COUNT ? tr[i] : 0.0;
  gs[GS_LOGDET_K] = ldK;
  gs[GS_LOGDET_A] = ldK + ldL;
  gs[GS_F] = -0.5 * Nglob * Dd * log(two_pi) + 0.5 * Nglob * Dd * log(beta) - 0.5 * beta * sumYY + beta * tMC - 0.5 * beta * tPW -
             0.5 * beta * Dd * (Psi0 - tP) - KL - KLu;
  gs[GS_GRAD_BETA] = 0.5 * Nglob * Dd / beta - 0.5 * sumYY + tMC - 0.5 * tPW - 0.5 * Dd * (Psi0 - tP);
  gs[GS_GRAD_SF2] = (tr[GS_SUM_V] + tr[GS_SUM_AC] + 2.0 * tr[GS_SUM_BPSI2] + (-0.5 * beta * Dd) * Psi0) / sf2;
  gs[GS_FAIL] = 0.0;
  gs[GS_FLAGS] = fsc[GS_FLAGS];
  gs[GS_FLAGS + 1] = lsc[1];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
static int svi_ready(gp_ctx* c, const char* who, SviPlan** p) {
  if (!c->svi) return fail(c, GP_ERR_STATE, "%s before gp_svi_begin (or after gp_svi_end)", who);
  *p = c->svi.get();
  return GP_OK;
}
static SviElem svi_elem(gp_ctx* c, SviPlan* p) {
  return {p->Lam, p->W, p->P2w, p->R, c->gstep.Bbar, c->gstep.Abar, p->Ll, p->lsc, p->G2, p->dg, p->S, c->gstep.Bm, c->beta, (double)c->D, c->Mp, c->Dp};
}
static int svi_pass(gp_ctx* c, SviPlan* p, int pass) {
  const long n = (long)c->Mp * c->Mp + (pass == SVI_BM ? (long)c->Mp * c->Dp : 0);
  GP_LAUNCH(c, c->stream, svi_assemble_kernel, dim3(blocks_for(n)), dim3(256), 0, svi_elem(c, p), pass);
  return GP_OK;
}
// a, Psi2w, Cw of the statistics and globals as they are now
static int svi_front(gp_ctx* c, SviPlan* p) {
  if (p->front_serial == c->life.inputs_serial()) return GP_OK;
  p->front_serial = -1;
  const int Mp = c->Mp, Dp = c->Dp;
  const SviOps o = svi_ops(c);
  // K_mm (+ 1e-7 I) into Lk and the kept copy; the kernel's A = K_mm + beta Psi2 is not wanted and lands in the work panel
  GP_TRY_RC(launch_build_kmm(c, c->stream, p->Lk, p->T, p->jitK ? 1e-7 : 0.0, 0.0, p->fsc, nullptr));
  GP_TRY_RC(potrf_inverse_batched(c, c->stream, Mp, 1, p->Lk, p->a, nullptr, p->T, p->fsc + GS_LOGDET_K, p->fsc + GS_FLAGS, nullptr, 0, false, true));
  // the blocked factorisation zeroes the upper part of the diagonal panels only: the 128-blocks above them still hold K_mm, and publish multiplies by
  // the whole of L_k
  for (int i = 0; i + 1 < Mp / 128; ++i) {
    const size_t cols = (size_t)Mp - (size_t)(i + 1) * 128;
    GP_HIP(c, hipMemset2DAsync(p->Lk + (size_t)i * 128 * Mp + (size_t)(i + 1) * 128, (size_t)Mp * 8, 0, cols * 8, 128, c->stream));
  }
  GP_TRY_RC((svi_gemm<T_is_a_Psi2>(c, Mp, Mp, o)));
  GP_TRY_RC((svi_gemm<P2w_is_T_at>(c, Mp, Mp, o)));
  GP_TRY_RC((svi_gemm<Cw_is_a_C>(c, Mp, Dp, o)));
  p->front_serial = c->life.inputs_serial();
  return GP_OK;
}
// Lam -> L_l (in Ll), L_l^-1, Sv (in W), Mv; ln|Lam| and the failure flag in lsc
static int svi_moments(gp_ctx* c, SviPlan* p) {
  const SviOps o = svi_ops(c);
  GP_TRY_RC(svi_pass(c, p, SVI_COPY));
  GP_TRY_RC(potrf_inverse_batched(c, c->stream, c->Mp, 1, p->Ll, p->Lli, p->W, p->T, p->lsc, p->lsc + 1, nullptr, 0));
  return svi_gemm<Mv_is_Sv_H>(c, c->Mp, c->Dp, o);
}
static int run_svi_step(gp_ctx* c, SviPlan* p) {
  const int Mp = c->Mp, Dp = c->Dp, M = c->M, D = c->D;
  const SviOps o = svi_ops(c);
  c->gstep.gs_status = GP_OK;
  GP_TRY_RC(svi_front(c, p));
  GP_TRY_RC(svi_moments(c, p));
  GP_TRY_RC((svi_gemm<W_is_DSv_plus_Mv_Mvt>(c, Mp, Mp, o, (double)D)));
  GP_TRY_RC(svi_pass(c, p, SVI_G2));
  GP_TRY_RC((svi_gemm<R_is_2_G2_P2w>(c, Mp, Mp, o)));
  GP_TRY_RC((svi_gemm<R_plus_Gc_Cwt>(c, Mp, Mp, o, c->beta)));
  GP_TRY_RC(svi_pass(c, p, SVI_S));
  GP_TRY_RC((svi_gemm<T_is_X_a>(c, Mp, Mp, o, (const double*)p->G2)));
  GP_TRY_RC((svi_gemm<Out_is_at_T>(c, Mp, Mp, o, o.Bbar)));
  GP_TRY_RC((svi_gemm<Abar_is_at_Gc>(c, Mp, Dp, o, c->beta)));
  GP_TRY_RC((svi_gemm<T_is_X_a>(c, Mp, Mp, o, (const double*)p->S)));
  GP_TRY_RC((svi_gemm<Out_is_at_T>(c, Mp, Mp, o, o.dFdK)));
  GP_TRY_RC(svi_pass(c, p, SVI_BM));
  const double* dg = p->dg;
  const DotJobs jobs = {{{p->Mv, p->Cw, Dp, M, D, SVI_TR_MC},
                         {p->P2w, p->W, Mp, M, M, SVI_TR_P2W_W},
                         {dg, dg + 2 * Mp, Mp, 1, M, SVI_TR_W},
                         {dg + Mp, dg + 2 * Mp, Mp, 1, M, SVI_TR_P2W},
                         {o.dFdK, c->gstep.KmmKeep, Mp, M, M, GS_SUM_V},
                         {o.Abar, o.C, Dp, M, D, GS_SUM_AC},
                         {o.Bbar, o.Psi2, Mp, M, M, GS_SUM_BPSI2}},
                        7};
  double* part = c->gstep.gs + GS_DOTS;
  GP_TRY_RC(launch_dots(c, c->stream, jobs, part));
  GP_LAUNCH(c, c->stream, svi_scalars_kernel, dim3(1), dim3(64), 0, o.C + (long)Mp * Dp, p->fsc, p->lsc, jobs, part, c->beta, c->sf2, (double)D,
            (double)c->N_global, (double)M, c->gstep.gs);
  return launch_kmm_grads(c, c->stream);
}

}  // namespace gp

using namespace gp;

extern "C" int gp_svi_begin(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  if (c->svi) return fail(c, GP_ERR_STATE, "gp_svi_begin: an SVI state exists already (gp_svi_end first)");
  GP_HIP(c, hipSetDevice(c->device));
  const size_t Mp = c->Mp, Dp = c->Dp, mm = Mp * Mp, md = Mp * Dp;
  // built aside and published whole: a failed allocation leaves the context without a plan
  std::unique_ptr<SviPlan, SviPlanDelete> p(new SviPlan());
  int rc = GP_OK;
  auto A = [&](DevBuf<double>& b, size_t n) { if (rc == GP_OK) rc = b.alloc(c, n, DA_RAW); };
  A(p->Lam, mm); A(p->H, md); A(p->Lk, mm); A(p->a, mm); A(p->P2w, mm); A(p->Cw, md); A(p->fsc, GS_HOST);
  A(p->Ll, mm); A(p->Lli, mm); A(p->W, mm); A(p->Mv, md); A(p->G2, mm); A(p->R, mm); A(p->S, mm);
  A(p->T, Mp * std::max(Mp, Dp)); A(p->dg, 3 * Mp); A(p->lsc, 8);
  GP_TRY_RC(rc);
  // the inverse factors' 128-blocks above the block diagonal are never written by the factorisation (potrf_inverse_batched's precondition)
  GP_HIP(c, hipMemsetAsync(p->a, 0, p->a.bytes(), c->stream));
  GP_HIP(c, hipMemsetAsync(p->Lli, 0, p->Lli.bytes(), c->stream));
  GP_LAUNCH(c, c->stream, svi_prior_kernel, dim3(blocks_for((long)(mm + md))), dim3(256), 0, c->Mp, c->Dp, p->Lam.get(), p->H.get());
  c->svi = std::move(p);
  return GP_OK;
}

extern "C" int gp_svi_end(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_end", &p));
  GP_HIP(c, hipSetDevice(c->device));
  GP_HIP(c, hipStreamSynchronize(c->stream));      // nothing enqueued may still use the plan
  ++c->sync_epoch;
  c->svi.reset();
  return GP_OK;
}

extern "C" int gp_svi_set(gp_ctx* c, const double* Lam, const double* H) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_set", &p));
  if (!Lam || !H) return fail(c, GP_ERR_BAD_ARG, "gp_svi_set: NULL array");
  const long M = c->M, D = c->D, Mp = c->Mp, Dp = c->Dp;
  for (long i = 0; i < M * M; ++i) if (!std::isfinite(Lam[i])) return fail(c, GP_ERR_BAD_ARG, "gp_svi_set: Lam is not finite");
  for (long i = 0; i < M * D; ++i) if (!std::isfinite(H[i])) return fail(c, GP_ERR_BAD_ARG, "gp_svi_set: H is not finite");
  for (long i = 0; i < M; ++i)
    for (long j = 0; j < i; ++j)
      if (Lam[i * M + j] != Lam[j * M + i]) return fail(c, GP_ERR_BAD_ARG, "gp_svi_set: Lam is not symmetric at (%ld, %ld)", i, j);
  GP_HIP(c, hipSetDevice(c->device));
  // padded images: identity block in Lam, zeros in H
  std::vector<double> hl((size_t)Mp * Mp, 0.0), hh((size_t)Mp * Dp, 0.0);
  for (long i = 0; i < Mp; ++i) {
    if (i < M) { memcpy(&hl[i * Mp], Lam + i * M, M * 8); memcpy(&hh[i * Dp], H + i * D, D * 8); }
    else hl[i * Mp + i] = 1.0;
  }
  GP_HIP(c, hipMemcpyAsync(p->Lam, hl.data(), hl.size() * 8, hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipMemcpyAsync(p->H, hh.data(), hh.size() * 8, hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));      // the staging vectors go
  ++c->sync_epoch;
  return GP_OK;
}

extern "C" int gp_svi_get(gp_ctx* c, double* Lam, double* H, double* Mv, double* Sv) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_get", &p));
  GP_HIP(c, hipSetDevice(c->device));
  const size_t M = c->M, D = c->D, Mp = c->Mp, Dp = c->Dp;
  double ls[2] = {0.0, 0.0};
  if (Mv || Sv) {
    GP_TRY_RC(svi_moments(c, p));
    GP_HIP(c, hipMemcpyAsync(ls, p->lsc, sizeof(ls), hipMemcpyDeviceToHost, c->stream));
  }
  auto down = [&](double* dst, const double* src, size_t ld, size_t cols) {
    return dst ? hipMemcpy2DAsync(dst, cols * 8, src, ld * 8, cols * 8, M, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  GP_HIP(c, down(Lam, p->Lam, Mp, M));
  GP_HIP(c, down(H, p->H, Dp, D));
  GP_HIP(c, down(Mv, p->Mv, Dp, D));
  GP_HIP(c, down(Sv, p->W, Mp, M));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  ++c->sync_epoch;
  if (ls[1] != 0.0) return fail(c, GP_ERR_NOT_PD, "gp_svi_get: Lambda_v is not positive definite (Mv and Sv are not defined)");
  return GP_OK;
}

extern "C" int gp_svi_natural_step(gp_ctx* c, double rho) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_natural_step", &p));
  if (!(rho > 0.0) || !(rho <= 1.0)) return fail(c, GP_ERR_BAD_ARG, "gp_svi_natural_step: rho must be in (0, 1], got %g", rho);
  if (!c->life.has_stats() || !c->life.has_globals()) return fail(c, GP_ERR_STATE, "gp_svi_natural_step needs statistics (gp_phase1 / gp_set_local_statistics) and globals");
  GP_HIP(c, hipSetDevice(c->device));
  GP_TRY_RC(svi_front(c, p));
  const long n = (long)c->Mp * c->Mp + (long)c->Mp * c->Dp;
  GP_LAUNCH(c, c->stream, svi_axpy_kernel, dim3(blocks_for(n)), dim3(256), 0, c->Mp, c->Dp, rho, c->beta, (const double*)p->P2w, (const double*)p->Cw,
            (const double*)(p->fsc + GS_FLAGS), p->Lam.get(), p->H.get());
  return GP_OK;
}

extern "C" int gp_svi_step(gp_ctx* c, int jitter_mask) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_step", &p));
  if (!c->life.has_stats() || !c->life.has_globals()) return fail(c, GP_ERR_STATE, "gp_svi_step needs statistics (gp_phase1 / gp_set_local_statistics) and globals");
  if (jitter_mask != 0 && jitter_mask != 1) return fail(c, GP_ERR_BAD_ARG, "gp_svi_step: mask must be 0 or 1 (K_mm; no jitter is added to Lambda_v)");
  GP_HIP(c, hipSetDevice(c->device));
  if (p->jitK != jitter_mask) { p->jitK = jitter_mask; p->front_serial = -1; }
  c->gstep.jitter_mask = jitter_mask;
  c->gstep.svi_step = true;
  c->life.step_started();
  GP_EV(c, 3);
  const int rc = run_svi_step(c, p);
  GP_EV(c, 4);
  if (rc != GP_OK) return rc;
  c->life.svi_step_enqueued();
  return GP_OK;
}

extern "C" int gp_svi_publish(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  SviPlan* p = nullptr;
  GP_TRY_RC(svi_ready(c, "gp_svi_publish", &p));
  if (!c->life.has_stats() || !c->life.has_globals()) return fail(c, GP_ERR_STATE, "gp_svi_publish needs statistics (gp_phase1 / gp_set_local_statistics) and globals");
  GP_HIP(c, hipSetDevice(c->device));
  const SviOps o = svi_ops(c);
  GP_TRY_RC(svi_front(c, p));                       // L_k (the front reads the statistics this call then replaces)
  GP_TRY_RC(svi_pass(c, p, SVI_X));
  GP_TRY_RC((svi_gemm<T_is_Lk_X>(c, c->Mp, c->Mp, o)));
  GP_TRY_RC((svi_gemm<Psi2eff_is_T_Lkt>(c, c->Mp, c->Mp, o, c->beta)));
  GP_TRY_RC((svi_gemm<Ceff_is_Lk_H>(c, c->Mp, c->Dp, o, c->beta)));
  c->life.stats_injected();
  return GP_OK;
}
