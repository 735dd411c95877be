// Held-out scoring on the device (gp_predict_score): the Gaussian log predictive density, the squared error and the normalised squared error of
// given outputs Y under gp_predict's mean and variance, reduced to one value per row and five sums per output column.
//
// For every observed entry (i, d), with m = gp_predict's mean, v = its variance (one per row for deterministic inputs, one per entry for uncertain
// ones, 1/beta added with flags bit 0) and e = y - m:
//   e2 = e e,   q = e2 / v,   logp = -1/2 (ln(2 pi v) + q)          each operation rounded once, no contraction (score_term, score_pass.h)
//   row_logp[i] = sum_d logp,  row_sse[i] = sum_d e2,  row_chi2[i] = sum_d q,   cols[d] = [count, sum_i e, sum_i e2, sum_i q, sum_i logp].
// Nothing of size n x D leaves the device: per chunk of gp_predict's pipeline
//   pred_chunk_front (predict.hip, as gp_predict runs it: the same kernels on the same buffers, so m and v are gp_predict's bits): G = [mean | Lk^-1 k |
//     La^-1 k]; uncertain inputs: pred_chunk_var_unc (LEA, pred_psi2w_kernel) -> var [cnt][D];
//   score_rows_kernel: one wave per row.  Deterministic inputs: the row's variance sf2 - |Lk^-1 k|^2 + |La^-1 k|^2 (+ 1/beta) from fac_norms as
//     pred_det_rows_kernel forms it, kept in rowv for the column pass; then score_row_sums.  Loads run along d (coalesced); no LDS, no scratch.
//   ScoreTotals::add_segments on PredSrc: the column sums of the chunk's segments into the call's totals.
// The passes, their summation order and the bad-variance flag are defined once, in score_pass.h, for this entry and gp_loo_score.
// Row invariance has gp_predict's limit: pred_chunk_front leaves the choice of the GEMM kernel to launch_gemm (32 x 32 tiles up to 256 tiles of 128 x 128
// in the launch, 128 x 128 tiles beyond; their k order differs), as gp_predict does, so that a row is scored on gp_predict's bits.  A row's mean and
// variance are the same bits in any two launches that put each product on the same kernel, and equal to rounding otherwise (include/gparml_hip.h).
// A scored entry whose variance is not > 0 has NaN terms: its row's three outputs and its column's five sums become NaN through the sums themselves;
// the column pass notes the first such row (plain stores, integer minimum) and the host reads one integer with the totals: no second pass.
// Resident rows (X_mu == NULL): device pointers into the context's X_mu / X_S go straight to pred_prep_kernel and Y is read where it lies, in the
// columns of Kaug behind Psi1 (leading dimension LDK): nothing is uploaded but an optional mask, nothing is staged.
// Buffers: ScorePlan, built aside and published whole; every element is written before it is read (DA_RAW: NaN-filled in the poison test mode).
#include "pred_chunk.h"
#include "score_pass.h"
#include <algorithm>
#include <cmath>

namespace gp {

// The entries of a chunk of gp_predict's pipeline: y from Y, m from G, v per entry (uncertain inputs) or per row (deterministic ones); no window
struct PredSrc {
  static constexpr int NFLAGS = 1;
  const double* G;          // [rows][ldg] the chunk's products: mean in columns 0 .. D, deterministic inputs [Lk^-1 k | La^-1 k] behind Dp
  long ldg;
  const double* uvar;       // [rows][D] uncertain inputs: the variance of every entry; NULL: deterministic
  double* rowv;             // [rows] deterministic inputs: the row's variance (written by the row pass, read by the column pass)
  const double* Y;          // the chunk's outputs, row stride ldy
  long ldy;
  const uint8_t* obs;       // [rows][D] non-zero = observed; NULL: every entry
  long rows, g0;            // rows of the chunk, global index of its first row
  int D;
  __device__ bool scored(long i, int d) const { return !obs || obs[i * D + d]; }      // a hidden entry of Y is never read
  __device__ bool unfactorised(long) const { return false; }
  __device__ double var(long i, int d) const { return uvar ? uvar[i * D + d] : rowv[i]; }
  __device__ ScoreTerm term_under(long i, int d, double v) const { return score_term(Y[i * ldy + d], G[i * ldg + d], v); }
  __device__ ScoreTerm term(long i, int d) const { return term_under(i, d, var(i, d)); }
};
// the row pass's view of its row: the variance of deterministic inputs is still in its register
struct PredRow {
  const PredSrc& s;
  double vrow;
  __device__ bool scored(long i, int d) const { return s.scored(i, d); }
  __device__ ScoreTerm term(long i, int d) const { return s.term_under(i, d, s.uvar ? s.uvar[i * s.D + d] : vrow); }
};

struct ScoreArgs {
  PredSrc src;
  int M, Mp, Dp;
  double sf2, noise;
  double* rowo;             // [3][R] row_logp | row_sse | row_chi2 of the chunk
  long R;
};

__global__ void __launch_bounds__(256) score_rows_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
  const PredSrc& s = a.src;
  const int lane = threadIdx.x & 63;
  const long n = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (n >= s.rows) return;
  double vrow = 0.0;
  if (!s.uvar) {
    const FacNorms f = fac_norms(s.G + n * s.ldg, a.M, a.Dp, a.Mp, lane);
    vrow = a.sf2 - f.a2 + f.b2 + a.noise;             // pred_det_rows_kernel's expression
  }
  const RowSums r = score_row_sums(PredRow{s, vrow}, n, s.D, lane);
  if (lane == 0) {
    a.rowo[n] = r.lp;
    a.rowo[a.R + n] = r.sse;
    a.rowo[2 * a.R + n] = r.chi;
    if (!s.uvar) s.rowv[n] = vrow;
  }
}

// ---- the column totals (ScoreTotals, score_pass.h) ----------------------------------------------------------------------------------------------
// tot [D][5] and totbad [flags]: set from zero / none (first segments of a call) or carried on; the last workgroup takes the bad rows
__global__ void __launch_bounds__(256) score_cols_final_kernel(const double* __restrict__ part, const long long* __restrict__ bad, int segs, int tiles, int flags,
                                                               long d5, int first, double* __restrict__ tot, long long* __restrict__ totbad) {
  if (blockIdx.x + 1 < gridDim.x) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= d5) return;
    double s = first ? 0.0 : tot[e];
    for (int g = 0; g < segs; ++g) s += part[g * d5 + e];       // segments ascending, one by one into the running total
    tot[e] = s;
    return;
  }
  // one thread per flag, serially: at most (16384 / 128) x tiles slots per chunk (128 at D <= 128), fewer loads than a block_fold's barriers would
  // cost, and a minimum of integers has no order to fix
  if ((int)threadIdx.x < flags) {
    long long b = first ? SC_NONE : totbad[threadIdx.x];
    for (long g = 0; g < (long)segs * tiles; ++g) b = min(b, bad[flags * g + threadIdx.x]);
    totbad[threadIdx.x] = b;
  }
}

int ScoreTotals::alloc(gp_ctx* c, long segments, long D_, int flags_) {
  D = D_; flags = flags_; tiles = (int)((D + SC_DW - 1) / SC_DW);
  GP_TRY_RC(part.alloc(c, (size_t)(segments * D * 5), DA_RAW));
  GP_TRY_RC(tot.alloc(c, (size_t)(D * 5), DA_RAW));
  return bad.alloc(c, (size_t)(flags * segments * tiles + flags), DA_RAW);
}

int ScoreTotals::fold(gp_ctx* c, hipStream_t st, int segs, bool first) const {
  const long d5 = 5 * D;
  GP_LAUNCH(c, st, score_cols_final_kernel, dim3((unsigned)((d5 + 255) / 256) + 1), dim3(256), 0, (const double*)part, (const long long*)bad, segs, tiles, flags, d5,
            first ? 1 : 0, tot.get(), call_flags());
  return GP_OK;
}

int ScoreTotals::read(gp_ctx* c, hipStream_t st, double* cols, long long* out) const {
  if (cols) GP_HIP(c, hipMemcpyAsync(cols, tot, (size_t)(5 * D) * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipMemcpyAsync(out, call_flags(), (size_t)flags * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

int score_fail_variance(gp_ctx* c, const char* entry, const char* which, long long row, int flags) {
  return fail(c, GP_ERR_NON_FINITE, "%s: the %s variance of a scored entry is not > 0 (first in row %lld): its row's outputs and its columns' sums are NaN, "
              "every other row is valid%s", entry, which, row, (flags & 1) ? "" : " (the variance of f can round to zero or below: score y, flags bit 0)");
}

// the buffers of a call, rows = gp_predict's chunk length: replaced whole when that changes.  Y and obs hold a chunk of host rows and are allocated
// by the first call that brings some (resident rows never need Y; obs only with a mask)
struct ScorePlan {
  long rows = 0;
  DevBuf<double> Y;           // [rows][D]
  DevBuf<uint8_t> obs;        // [rows][D]
  DevBuf<double> rowo;        // [3][rows] row_logp | row_sse | row_chi2
  DevBuf<double> rowv;        // [rows] the rows' variance (deterministic inputs)
  ScoreTotals totals;         // rows / SC_SEG segments, one flag
};
void ScorePlanDelete::operator()(ScorePlan* p) const { delete p; }

static int score_alloc(gp_ctx* c, long R, bool host_y, bool mask) {
  const long D = c->D;
  if (!c->score || c->score->rows != R) {
    c->score.reset();
    std::unique_ptr<ScorePlan, ScorePlanDelete> p(new ScorePlan());
    GP_TRY_RC(p->rowo.alloc(c, (size_t)(3 * R), DA_RAW));
    GP_TRY_RC(p->rowv.alloc(c, (size_t)R, DA_RAW));
    GP_TRY_RC(p->totals.alloc(c, R / SC_SEG, D, PredSrc::NFLAGS));
    p->rows = R;
    c->score = std::move(p);
  }
  if (host_y) GP_TRY_RC(c->score->Y.grow(c, (size_t)(R * D), DA_RAW));
  if (mask) GP_TRY_RC(c->score->obs.grow(c, (size_t)(R * D), DA_RAW));
  return GP_OK;
}

// resident: the inputs are the context's X_mu (and, resident_S, its X_S in the form it was uploaded in); Y == NULL then means the resident Y.
// The arguments have been checked (api.hip); n > 0 and at least one output is wanted.
int run_predict_score(gp_ctx* c, long n, const double* X_mu, const double* X_S, int raw, bool resident, bool resident_S, const double* Y,
                      const uint8_t* observed, int flags, double* row_logp, double* row_sse, double* row_chi2, double* cols) {
  if (resident) {
    X_mu = c->Xmu;
    X_S = resident_S ? c->Xs.get() : nullptr;
    raw = resident_S && c->xs_raw ? 1 : 0;
  }
  const bool unc = X_S != nullptr;
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, unc, &k));
  const long R = k.rows;
  GP_TRY_RC(score_alloc(c, R, Y != nullptr, observed != nullptr));
  const ScorePlan& p = *c->score;
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Dp = c->Dp, D = c->D;
  if (unc) GP_TRY_RC(pred_unc_begin(c));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X_mu).uncertain(X_S, raw).on_device(resident), n0, cnt, pred_into(k.mu).factors(unc ? nullptr : k.G + Dp, k.ldg)));
    ScoreArgs a;
    PredSrc& s = a.src;
    s.G = k.G; s.ldg = k.ldg; s.uvar = nullptr;
    if (unc) {
      GP_TRY_RC(pred_chunk_var_unc(c, cnt, (flags & 1) ? 1.0 / c->beta : 0.0, k.var));
      s.uvar = k.var;
    }
    if (Y) {
      GP_HIP(c, hipMemcpyAsync(p.Y, Y + n0 * D, (size_t)(cnt * D) * 8, hipMemcpyHostToDevice, st));
      s.Y = p.Y; s.ldy = D;
    } else {
      s.Y = c->Kaug + n0 * c->LDK + Mp; s.ldy = c->LDK;       // the resident Y: the columns of Kaug behind Psi1
    }
    s.obs = nullptr;
    if (observed) {
      GP_HIP(c, hipMemcpyAsync(p.obs, observed + n0 * D, (size_t)(cnt * D), hipMemcpyHostToDevice, st));
      s.obs = p.obs;
    }
    s.rowv = p.rowv; s.rows = cnt; s.g0 = n0; s.D = (int)D;
    a.M = c->M; a.Mp = (int)Mp; a.Dp = (int)Dp; a.sf2 = c->sf2; a.noise = (flags & 1) ? 1.0 / c->beta : 0.0;
    a.rowo = p.rowo; a.R = R;
    GP_LAUNCH(c, st, score_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, a);
    GP_TRY_RC(p.totals.add_segments(c, st, s, (int)((cnt + SC_SEG - 1) / SC_SEG), n0 == 0));
    if (row_logp) GP_HIP(c, hipMemcpyAsync(row_logp + n0, p.rowo, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (row_sse) GP_HIP(c, hipMemcpyAsync(row_sse + n0, p.rowo + R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (row_chi2) GP_HIP(c, hipMemcpyAsync(row_chi2 + n0, p.rowo + 2 * R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
  }
  long long bad = SC_NONE;
  GP_TRY_RC(p.totals.read(c, st, cols, &bad));
  if (bad != SC_NONE) return score_fail_variance(c, "gp_predict_score", "predictive", bad, flags);
  return GP_OK;
}

}  // namespace gp
