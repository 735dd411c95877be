// gp_predict's chunk pipeline (predict.hip) as the features at new inputs share it (joint, grad, paths, curve, score): pred_chunk_open once per call,
// pred_chunk_front per chunk, described by name as gemm_of(..) describes a product: pred_at(X).uncertain(..), pred_into(mu).factors(..).on_big()
#pragma once
#include "gp_common.h"

namespace gp {

// A view of the chunk buffers.  It points into the context's PredPlan and is valid until that plan is replaced: by a pred_chunk_open after the
// chunk length changed (gp_debug_set_option "predict_rows"), or by the context's deletion.  Every call takes its own.
struct PredChunk {
  long rows;                  // points per chunk (a multiple of 128)
  const double* inputs;       // [2][rows][Q] X_mu | X_S of the chunk as the caller gave them (curve.hip differences them before the centring rounds them)
  double* mu;                 // [rows][Q] the chunk's own place for the centred inputs
  const double* psi1;         // [rows][Mp] Psi1* of the chunk pred_chunk_front has just run
  double* G;                  // [rows][ldg] [mean | Lk^-1 k* | La^-1 k*]; the mean product always lands in its first Dp columns
  long ldg;                   // Dp + 2 Mp
  double* var;                // [rows][D] the chunk's own place for the variances
};
// builds the buffers on first use; uncertain: with those of the uncertain-input variance
int pred_chunk_open(gp_ctx* c, bool uncertain, PredChunk* k);

// GEMM_BIG: the 128 x 128-tile kernel whatever the chunk's size (GemmP::on_big), so that a row's bits do not depend on the rows around it
enum GemmTile { GEMM_BY_SIZE = 0, GEMM_BIG = 1 };

// The inputs of a call, all n rows: pred_chunk_front takes rows n0 .. n0 + cnt.  X_S NULL: deterministic; raw: X_S in softplus-inverse space;
// device: both are device arrays (the resident rows, score.hip) and go to pred_prep_kernel as they are, nothing is uploaded or staged
struct PredIn {
  const double* X_mu = nullptr; const double* X_S = nullptr; int raw = 0; bool device = false;
  PredIn uncertain(const double* S, int S_is_raw) const { PredIn p = *this; p.X_S = S; p.raw = S_is_raw; return p; }
  PredIn on_device(bool d) const { PredIn p = *this; p.device = d; return p; }
};
inline PredIn pred_at(const double* X_mu) { PredIn p; p.X_mu = X_mu; return p; }
// Where a chunk's results go: mu [rows][Q] the centred inputs; fac (leading dimension ldf) the rows [Lk^-1 k* | La^-1 k*], NULL: not formed
struct PredOut {
  double* mu = nullptr; double* fac = nullptr; long ldf = 0; GemmTile tile = GEMM_BY_SIZE;
  PredOut factors(double* f, long ld) const { PredOut p = *this; p.fac = f; p.ldf = ld; return p; }
  PredOut on_big() const { PredOut p = *this; p.tile = GEMM_BIG; return p; }
};
inline PredOut pred_into(double* mu) { PredOut p; p.mu = mu; return p; }

// upload, pred_prep_kernel, Psi1*, then pred_project of the Psi1* rows: the mean into the chunk's G, the factor rows into out.fac
int pred_chunk_front(gp_ctx* c, const PredIn& in, long n0, long cnt, const PredOut& out);
// The product pair [rows][Mp] x [beta E | Linv^T] that turns rows of Psi1* -- or their derivatives (grad.hip) or differences (curve.hip) -- into
// [mean | Lk^-1 k | La^-1 k]: A against gstep.E into e [rows][Dp], then against gstep.Linv into fac [rows][2 Mp]; a NULL destination is not formed
int pred_project(gp_ctx* c, const double* A, long rows, GemmOut e, GemmOut fac, GemmTile tile);
// the mean rows [cnt][D] of the chunk pred_chunk_front has just run, out of G into a device buffer of the caller
int pred_chunk_mean(gp_ctx* c, long cnt, double* mean);
// the uncertain-input variance: B = Ki - P once per call before the first chunk, then per chunk LEA and pred_psi2w_kernel into var [cnt][D]
int pred_unc_begin(gp_ctx* c);
int pred_chunk_var_unc(gp_ctx* c, long cnt, double noise, double* var);
// fill_mean_kernel: C [rows][cols] = mean[i][col mod D] for i < n and col < used, else 0; a product with beta = 1 then adds a draw's terms on top
int pred_fill_mean(gp_ctx* c, const double* mean, long n, long rows, long cols, long used, double* C);
// the same with a leading dimension on the source: C [rows][cols] = src[i][col mod D] (row stride lds) for i < n and col < used, else 0 -- the
// rows of gp_paths_grad are (point, q) rows of the mean's Jacobian.  A sibling kernel: fill_mean_kernel and its callers keep their bits
int pred_fill_rows(gp_ctx* c, const double* src, long lds, long n, long rows, long cols, long used, double* C);
// grad.hip's grad_dk_kernel as gp_predict_grad launches it: dK [(i, q)][Mp] = d k(x_i) / d x_q for i < pts, exact zeros in the rows beyond (and in
// the columns >= M), rows = round_up(pts Q, 128); P1 = Psi1* and X the centred inputs of the chunk pred_chunk_front has just run
int grad_launch_dk(gp_ctx* c, const double* P1, const double* X, long pts, long rows, double* dK);
const double* pred_debug_lea(const gp_ctx* c, long* n);               // gp_debug_peek: the uncertain-input plan's LEA, NULL / 0 without one

}  // namespace gp
