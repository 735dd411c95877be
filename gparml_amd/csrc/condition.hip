// The posterior conditioned on m extra observed rows (gp_condition_set, gp_condition_predict, gp_condition_clear), after a global step of this
// context: a rank-m UPDATE of the model, the mirror image of gp_loo_score's downdate.
//
// Fixed Z, sf2, alpha, beta.  With k(x) = psi1(x), a = Lk^-1 k, b = La^-1 k, mean(x) = k^T W and var(x) = sf2 - |a|^2 + |b|^2 (gp_predict's
// quantities), a row with a deterministic input contributes beta k k^T to A = Kmm + beta Psi2 and k y^T to Psi1^T Y.  For the conditioning rows
// x_1 .. x_m with outputs Y_c (m, D), B_c (m, M) their rows b_j and M_c (m, D) their means under the model as it is:
//   S = I + beta B_c B_c^T = L L^T,  X = L^-1,  V = X B_c (m, M),  T = X (Y_c - M_c) (m, D)
// and for any query x with u(x) = V b(x) (m):
//   mean'(x)_d = mean(x)_d + beta u . T[:, d]        var'(x) = var(x) - beta |u|^2 (+ 1/beta)
// S >= I: it always factorises, |S^-1| <= 1, nothing is amplified.
// gp_condition_set, the m rows in chunks of gp_predict's pipeline:
//   pred_chunk_front, factors on the 128 x 128-tile kernel (on_big): G = [M_c | a | b];
//   cond_rhs_kernel     W = [B_c | Y_c - M_c], [mp][Mp + Dp], mp = m rounded up to 128; rows >= m, columns >= M and >= D are exact zeros;
//   launch_gemm         S = beta B_c B_c^T (B_c against itself, k over Mp ascending);
//   cond_identity_kernel  adds the identity; rows and columns m .. mp - 1 become the identity's;
//   mp = 128: potrf_trinv128_tiles (L and X = L^-1, LDS-resident); beyond: potrf_inverse_batched(factor_only): L and the inverses X_ii of its
//     diagonal blocks, then the block forward substitution R_i = X_ii (W_i - sum_{j < i} L_ij R_j), two products per block row;
//   R = [V | T] [mp][Mp + Dp] is all the plan keeps.  Rows >= m of R are exact zeros (X is the identity there, W zero).
// gp_condition_predict, per chunk of gp_predict's plan:
//   pred_chunk_front, factors on_big: G = [mean | a | b];
//   launch_gemm         U = b V^T, [rows][Mp] x [Mp][mp] (k over Mp ascending);
//   launch_gemm         mean += beta U T, accumulating onto the mean columns of G (k over mp ascending);
//   cond_rows_kernel    one wave per point: the mean out, |a|^2 and |b|^2 (fac_norms), |u|^2 (lane l adds j = l, l + 64, .. ascending, then the xor
//                       butterfly), var, var' = var - beta |u|^2 and reduction = var - var'.
// The reduction is returned as the difference of the two variances as they are rounded, so that var - reduction gives the bits of var' and
// var - var' the bits of reduction, where var is gp_predict's for a row on the same GEMM kernel; it is >= 0 because rounding is monotone.
// Determinism: every product runs on the 128 x 128-tile GEMM kernel without split-k (on_big) whatever the launch size, so a point's outputs depend
// on that point, the set and the model only: the same bits alone, in any batch and wherever a chunk boundary falls.  No floating-point atomics, no
// scratch.  Every buffer belongs to the context's CondPlan, built aside and published whole; every element is written before it is read (DA_RAW),
// except the inverse factor's zero contract.  The evaluation's buffers are only read.
#define POTRF128_NO_KERNEL
#include "potrf128.h"
#include "pred_chunk.h"
#include "lane_reduce.h"
#include "score_pass.h"
#include <algorithm>
#include <cmath>

namespace gp {

// rows r0 .. r1 - 1 of W [mp][ldw] = [b (Mp) | y - mean (Dp)]: row r < m from row r - g0 of the chunk's G and row r of Y, else zero
__global__ void __launch_bounds__(256) cond_rhs_kernel(const double* __restrict__ G, long ldg, long g0, const double* __restrict__ Y, long r0, long r1, long m, int M,
                                                       int Mp, int D, int Dp, double* __restrict__ W) {
#pragma clang fp contract(off)
  const long ldw = Mp + Dp, total = (r1 - r0) * ldw;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long r = r0 + e / ldw, col = e % ldw;
    double v = 0.0;
    if (r < m) {
      const double* g = G + (r - g0) * ldg;
      if (col < M) v = g[Dp + Mp + col];
      else if (col >= Mp && col - Mp < D) v = Y[r * D + (col - Mp)] - g[col - Mp];
    }
    W[r * ldw + col] = v;
  }
}

// S [mp][mp] = beta B_c B_c^T on entry: the identity is added; rows and columns m .. mp - 1 become the identity's
__global__ void __launch_bounds__(256) cond_identity_kernel(double* __restrict__ S, long m, long mp) {
  const long total = mp * mp;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long r = e / mp, col = e - r * mp;
    const double delta = r == col ? 1.0 : 0.0;
    S[e] = (r < m && col < m) ? S[e] + delta : delta;
  }
}

struct CondRowsArgs {
  const double* G;      // [rows][ldg] [mean' | a | b] of the chunk
  long ldg;
  const double* U;      // [rows][mp] u = V b
  long cnt;
  int m, mp, M, Mp, D, Dp;
  double sf2, beta, noise;
  double* mean;         // [cnt][D], NULL: not wanted
  double* var;          // [cnt] var'
  double* red;          // [cnt] var - var'
};

// one wave per point
__global__ void __launch_bounds__(256) cond_rows_kernel(CondRowsArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long n = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (n >= a.cnt) return;
  const double* g = a.G + n * a.ldg;
  if (a.mean)
    for (int d = lane; d < a.D; d += 64) a.mean[n * a.D + d] = g[d];
  const FacNorms f = fac_norms(g, a.M, a.Dp, a.Mp, lane);
  const double* u = a.U + n * a.mp;
  double s = 0.0;
  for (int j = lane; j < a.m; j += 64) s = fma(u[j], u[j], s);
  const double u2 = wave_sum(s);
  if (lane == 0) {
    const double var = a.sf2 - f.a2 + f.b2 + a.noise;       // pred_det_rows_kernel's expression
    const double vc = var - a.beta * u2;
    a.var[n] = vc;
    a.red[n] = var - vc;
  }
}

// the chunk buffers of gp_condition_predict: replaced whole when gp_predict's chunk length changes
struct CondChunk {
  long rows = 0;
  DevBuf<double> U;           // [rows][mp]
  DevBuf<double> mean;        // [rows][D]
  DevBuf<double> out;         // [2][rows] var' | reduction
};

struct CondPlan {
  long m = 0, mp = 0;
  long serial = 0;            // Lifecycle::model_serial() of the global step the set was formed from
  DevBuf<double> R;           // [mp][Mp + Dp] [V | T]
  std::unique_ptr<CondChunk> chunk;
};
void CondPlanDelete::operator()(CondPlan* p) const { delete p; }

// The earlier set is dropped first; the new one is built aside and published only when complete: a call that fails part way leaves the context
// without a set, never with half of one.
int run_condition_set(gp_ctx* c, long m, const double* Xc, const double* Yc) {
  const long Mp = c->Mp, Dp = c->Dp, D = c->D, mp = round_up(m, NB), ldw = Mp + Dp;
  hipStream_t st = c->stream;
  c->cond.reset();
  std::unique_ptr<CondPlan, CondPlanDelete> p(new CondPlan());
  p->m = m; p->mp = mp; p->serial = c->life.model_serial();
  DevBuf<double> dY, W, S, X, Tw, flag;               // this call's only: Y_c, [B_c | Y_c - M_c], S -> L, X (its diagonal blocks), the work panel, fail | logdet
  GP_TRY_RC(p->R.alloc(c, (size_t)(mp * ldw), DA_RAW));
  GP_TRY_RC(dY.alloc(c, (size_t)(m * D), DA_RAW)); GP_TRY_RC(W.alloc(c, (size_t)(mp * ldw), DA_RAW)); GP_TRY_RC(S.alloc(c, (size_t)(mp * mp), DA_RAW));
  GP_TRY_RC(X.alloc(c, (size_t)(mp * mp), DA_ZERO));   // zero contract: the 128-blocks above the block diagonal are never written (potrf_inverse_batched's precondition)
  GP_TRY_RC(Tw.alloc(c, (size_t)(mp * mp / 2), DA_RAW));
  GP_TRY_RC(flag.alloc(c, 2, DA_ZERO));                // zero contract: the factorisation raises the flag and adds to the log-determinant
  GP_HIP(c, hipMemcpyAsync(dY, Yc, dY.bytes(), hipMemcpyHostToDevice, st));
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  for (long n0 = 0; n0 < m; n0 += k.rows) {
    const long cnt = std::min(k.rows, m - n0), r1 = n0 + cnt == m ? mp : n0 + cnt;
    GP_TRY_RC(pred_chunk_front(c, pred_at(Xc), n0, cnt, pred_into(k.mu).factors(k.G + Dp, k.ldg).on_big()));
    GP_LAUNCH(c, st, cond_rhs_kernel, dim3((unsigned)blocks_for((r1 - n0) * ldw)), dim3(256), 0, (const double*)k.G, k.ldg, n0, (const double*)dY, n0, r1, m, c->M,
              (int)Mp, (int)D, (int)Dp, W.get());
  }
  // S = beta B_c B_c^T: B_c [i][k] K_CONTIG on both sides
  GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)mp, (int)mp, 1, gemm_of({W, ldw}, {W, ldw}, {S, mp}, (int)Mp, c->beta).on_big(1)));
  GP_LAUNCH(c, st, cond_identity_kernel, dim3((unsigned)blocks_for(mp * mp)), dim3(256), 0, S.get(), m, mp);
  if (mp == NB) GP_TRY_RC(potrf_trinv128_tiles(c, st, 1, S, X, flag, flag + 1));
  else GP_TRY_RC(potrf_inverse_batched(c, st, (int)mp, 1, S, X, nullptr, Tw, flag + 1, flag, nullptr, 0, true));
  // R = L^-1 W by block rows: W_i -= L_ij R_j over the finished rows j < i (L [i][k] K_CONTIG, R [k][column] FREE_CONTIG), then R_i = X_ii W_i
  for (long i = 0; i < mp / NB; ++i) {
    double* Wi = W + i * NB * ldw;
    if (i > 0)
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, NB, (int)ldw, 1, gemm_of({S + i * NB * mp, mp}, {p->R, ldw}, {Wi, ldw}, (int)(i * NB), -1.0, 1.0).on_big(1)));
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, NB, (int)ldw, 1, gemm_of({X + i * NB * (mp + 1), mp}, {Wi, ldw}, {p->R + i * NB * ldw, ldw}, NB).on_big(1)));
  }
  double h[2];
  GP_HIP(c, hipMemcpyAsync(h, flag, sizeof(h), hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  if (h[0] != 0.0)
    return fail(c, GP_ERR_NOT_PD, "gp_condition_set: S = I + beta B B^T of the conditioning rows does not factorise.  In exact arithmetic this cannot "
                "happen (S >= I): the model's factors or the rows are not what they should be");
  c->cond = std::move(p);
  return GP_OK;
}

bool cond_plan_current(gp_ctx* c) {
  if (c->cond && !(c->life.model_current() && c->cond->serial == c->life.model_serial())) c->cond.reset();
  return c->cond != nullptr;
}

int run_condition_predict(gp_ctx* c, long n, const double* X, int flags, double* mean, double* var, double* reduction) {
  CondPlan& p = *c->cond;
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Dp = c->Dp, D = c->D, mp = p.mp, ldw = Mp + Dp;
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  const long R = k.rows;
  if (!p.chunk || p.chunk->rows != R) {
    p.chunk.reset();
    auto q = std::make_unique<CondChunk>();
    GP_TRY_RC(q->U.alloc(c, (size_t)(R * mp), DA_RAW)); GP_TRY_RC(q->mean.alloc(c, (size_t)(R * D), DA_RAW)); GP_TRY_RC(q->out.alloc(c, (size_t)(2 * R), DA_RAW));
    q->rows = R;
    p.chunk = std::move(q);
  }
  const CondChunk& q = *p.chunk;
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0), rows = round_up(cnt, TILE);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), n0, cnt, pred_into(k.mu).factors(k.G + Dp, k.ldg).on_big()));
    // U = b V^T: b [i][k] K_CONTIG, V [j][k] K_CONTIG
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)rows, (int)mp, 1, gemm_of({k.G + Dp + Mp, k.ldg}, {p.R, ldw}, {q.U, mp}, (int)Mp).on_big(1)));
    // mean += beta U T: U [i][k] K_CONTIG, T [k][d] FREE_CONTIG
    if (mean)
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)rows, (int)Dp, 1, gemm_of({q.U, mp}, {p.R + Mp, ldw}, {k.G, k.ldg}, (int)mp, c->beta, 1.0).on_big(1)));
    CondRowsArgs a;
    a.G = k.G; a.ldg = k.ldg; a.U = q.U; a.cnt = cnt; a.m = (int)p.m; a.mp = (int)mp; a.M = c->M; a.Mp = (int)Mp; a.D = (int)D; a.Dp = (int)Dp;
    a.sf2 = c->sf2; a.beta = c->beta; a.noise = (flags & 1) ? 1.0 / c->beta : 0.0;
    a.mean = mean ? q.mean.get() : nullptr; a.var = q.out; a.red = q.out + R;
    GP_LAUNCH(c, st, cond_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, a);
    if (mean) GP_HIP(c, hipMemcpyAsync(mean + n0 * D, q.mean, (size_t)(cnt * D) * 8, hipMemcpyDeviceToHost, st));
    if (var) GP_HIP(c, hipMemcpyAsync(var + n0, q.out, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (reduction) GP_HIP(c, hipMemcpyAsync(reduction + n0, q.out + R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
