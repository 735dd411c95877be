// Held-out scoring on the device (gp_predict_score): the Gaussian log predictive density, the squared error and the normalised squared error of
// given outputs Y under gp_predict's mean and variance, reduced to one value per row and five sums per output column.
//
// For every observed entry (i, d), with m = gp_predict's mean, v = its variance (one per row for deterministic inputs, one per entry for uncertain
// ones, 1/beta added with flags bit 0) and e = y - m:
//   e2 = e e,   q = e2 / v,   logp = -1/2 (ln(2 pi v) + q)          each operation rounded once, no contraction (score_term)
//   row_logp[i] = sum_d logp,  row_sse[i] = sum_d e2,  row_chi2[i] = sum_d q,   cols[d] = [count, sum_i e, sum_i e2, sum_i q, sum_i logp].
// Nothing of size n x D leaves the device: per chunk of gp_predict's pipeline
//   pred_chunk_front (predict.hip, as gp_predict runs it: the same kernels on the same buffers, so m and v are gp_predict's bits): G = [mean | Lk^-1 k |
//     La^-1 k]; uncertain inputs: pred_chunk_var_unc (LEA, pred_psi2w_kernel) -> var [cnt][D];
//   score_rows_kernel: one wave per row.  Deterministic inputs: the row's variance sf2 - |Lk^-1 k|^2 + |La^-1 k|^2 (+ 1/beta) in the operation order of
//     pred_det_rows_kernel, kept in rowv for the column pass.  Lane l adds the terms of d = l, l + 64, .. in ascending order, then the xor butterfly of
//     distance 32 .. 1 (wave_sum): an order that is a function of D alone.  Loads run along d (coalesced); no LDS, no scratch.
//   score_cols_kernel: workgroup (segment of 128 rows, tile of 128 columns).  The per-entry terms are RECOMPUTED from the same inputs by the same
//     function (score_term) rather than stored by the row pass: four n x D arrays less to write and read.  Thread (column c, half h) adds the rows
//     64 h .. 64 h + 63 of the segment in ascending order, the two halves are added as half 0 + half 1: one partial [D][5] per segment.
//   score_cols_final_kernel: the running totals [D][5] take the chunk's segments one by one in ascending order (the first segment of a call is added
//     to zero), so the ORDER of the column sums depends on the global row index alone: segments are 128 rows, the chunk length is a multiple of 128.
// Row invariance has gp_predict's limit: pred_chunk_front leaves the choice of the GEMM kernel to launch_gemm (32 x 32 tiles up to 256 tiles of 128 x 128
// in the launch, 128 x 128 tiles beyond; their k order differs), as gp_predict does, so that a row is scored on gp_predict's bits.  A row's mean and
// variance are the same bits in any two launches that put each product on the same kernel, and equal to rounding otherwise (include/gparml_hip.h).
// A scored entry whose variance is not > 0 has NaN terms: its row's three outputs and its column's five sums become NaN through the sums themselves.
// The column pass also notes the first such row per (segment, tile) -- plain stores, integer minimum -- and the final kernel carries the least one
// along: the host reads one integer with the totals; there is no second pass.
// Resident rows (X_mu == NULL): device pointers into the context's X_mu / X_S go straight to pred_prep_kernel and Y is read where it lies, in the
// columns of Kaug behind Psi1 (leading dimension LDK): nothing is uploaded but an optional mask, nothing is staged.
// Buffers: ScorePlan, built aside and published whole; every element is written before it is read (DA_RAW: NaN-filled in the poison test mode).
#include "pred_chunk.h"
#include "lane_reduce.h"
#include "score_term.h"
#include <algorithm>
#include <cmath>

namespace gp {

struct ScoreArgs {
  const double* G;          // [rows][ldg] the chunk's products: mean in columns 0 .. D, deterministic inputs [Lk^-1 k | La^-1 k] behind Dp
  long ldg;
  const double* var;        // [cnt][D] uncertain inputs: the variance of every entry; NULL: deterministic
  const double* Y;          // the chunk's outputs, row stride ldy
  long ldy;
  const uint8_t* obs;       // [cnt][D] non-zero = observed; NULL: every entry
  long cnt, n0;             // rows of the chunk, global index of its first row
  int M, Mp, D, Dp;
  double sf2, noise;
  double* rowv;             // [cnt] deterministic inputs: the row's variance (written by the row pass, read by the column pass)
  double* rowo;             // [3][R] row_logp | row_sse | row_chi2 of the chunk
  long R;
  double* part;             // [segments][D][5]
  long long* bad;           // [segments][tiles] first row with a variance that is not > 0, SC_NONE without one
};

__global__ void __launch_bounds__(256) score_rows_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long n = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (n >= a.cnt) return;
  const double* g = a.G + n * a.ldg;
  double vrow = 0.0;
  if (!a.var) {
    // pred_det_rows_kernel's variance, operation for operation
    double sk = 0.0, sa = 0.0;
    for (int i = lane; i < a.M; i += 64) {
      const double x = g[a.Dp + i], b = g[a.Dp + a.Mp + i];
      sk = fma(x, x, sk);
      sa = fma(b, b, sa);
    }
    sk = wave_sum(sk);
    sa = wave_sum(sa);
    vrow = a.sf2 - sk + sa + a.noise;
  }
  const double* y = a.Y + n * a.ldy;
  const uint8_t* o = a.obs ? a.obs + n * a.D : nullptr;
  const double* vr = a.var ? a.var + n * a.D : nullptr;
  double lp = 0.0, sse = 0.0, chi = 0.0;
  for (int d = lane; d < a.D; d += 64) {
    if (o && !o[d]) continue;                       // a hidden entry of Y is never read
    const ScoreTerm t = score_term(y[d], g[d], vr ? vr[d] : vrow);
    lp += t.lp;
    sse += t.e2;
    chi += t.q;
  }
  lp = wave_sum(lp);
  sse = wave_sum(sse);
  chi = wave_sum(chi);
  if (lane == 0) {
    a.rowo[n] = lp;
    a.rowo[a.R + n] = sse;
    a.rowo[2 * a.R + n] = chi;
    if (!a.var) a.rowv[n] = vrow;
  }
}

// grid (segments of the chunk, ceil(D / SC_DW))
__global__ void __launch_bounds__(256) score_cols_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
  __shared__ double sh[5 * SC_DW];
  __shared__ long long fb[256];
  const int tid = threadIdx.x, cc = tid & (SC_DW - 1), half = tid >> 7;
  const int d = blockIdx.y * SC_DW + cc;
  const long r0 = (long)blockIdx.x * SC_SEG + 64L * half;
  const long r1 = min(r0 + 64, a.cnt);
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long first = SC_NONE;
  if (d < a.D) {
    for (long i = r0; i < r1; ++i) {
      if (a.obs && !a.obs[i * a.D + d]) continue;
      const double v = a.var ? a.var[i * a.D + d] : a.rowv[i];
      const ScoreTerm t = score_term(a.Y[i * a.ldy + d], a.G[i * a.ldg + d], v);
      s[0] += (v > 0.0) ? 1.0 : t.e;
      s[1] += t.e;
      s[2] += t.e2;
      s[3] += t.q;
      s[4] += t.lp;
      if (!(v > 0.0) && first == SC_NONE) first = a.n0 + i;
    }
  }
  fb[tid] = first;
  if (half == 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[k * SC_DW + cc] = s[k];
  }
  __syncthreads();
  if (half == 0 && d < a.D) {
    double* out = a.part + ((long)blockIdx.x * a.D + d) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = s[k] + sh[k * SC_DW + cc];
  }
  block_fold<256>([&](int i, int j) { fb[i] = min(fb[i], fb[j]); });
  if (tid == 0) a.bad[(long)blockIdx.x * gridDim.y + blockIdx.y] = fb[0];
}

// tot [D][5] and totbad [1]: set from zero / none (first chunk of a call) or carried on; the last workgroup takes the rows with a bad variance
__global__ void __launch_bounds__(256) score_cols_final_kernel(const double* __restrict__ part, const long long* __restrict__ bad, int segs, int tiles, long d5,
                                                               int first, double* __restrict__ tot, long long* __restrict__ totbad) {
  if (blockIdx.x + 1 < gridDim.x) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= d5) return;
    double s = first ? 0.0 : tot[e];
    for (int g = 0; g < segs; ++g) s += part[g * d5 + e];       // segments ascending, one by one into the running total
    tot[e] = s;
    return;
  }
  // one thread, serially: at most (16384 / 128) x tiles slots per chunk (128 at D <= 128), fewer loads than a block_fold's barriers would cost, and a
  // minimum of integers has no order to fix
  if (threadIdx.x == 0) {
    long long b = first ? SC_NONE : totbad[0];
    for (long g = 0; g < (long)segs * tiles; ++g) b = min(b, bad[g]);
    totbad[0] = b;
  }
}

// the buffers of a call, rows = gp_predict's chunk length: replaced whole when that changes.  Y and obs hold a chunk of host rows and are allocated
// by the first call that brings some (resident rows never need Y; obs only with a mask)
struct ScorePlan {
  long rows = 0;
  DevBuf<double> Y;           // [rows][D]
  DevBuf<uint8_t> obs;        // [rows][D]
  DevBuf<double> rowo;        // [3][rows] row_logp | row_sse | row_chi2
  DevBuf<double> rowv;        // [rows] the rows' variance (deterministic inputs)
  DevBuf<double> part;        // [rows / SC_SEG][D][5]
  DevBuf<double> tot;         // [D][5]
  DevBuf<long long> bad;      // [rows / SC_SEG][tiles] | [1] the call's first bad row
};
void ScorePlanDelete::operator()(ScorePlan* p) const { delete p; }

static int score_alloc(gp_ctx* c, long R, bool host_y, bool mask) {
  const long D = c->D, segs = R / SC_SEG, tiles = (D + SC_DW - 1) / SC_DW;
  if (!c->score || c->score->rows != R) {
    c->score.reset();
    std::unique_ptr<ScorePlan, ScorePlanDelete> p(new ScorePlan());
    GP_TRY_RC(p->rowo.alloc(c, (size_t)(3 * R), DA_RAW));
    GP_TRY_RC(p->rowv.alloc(c, (size_t)R, DA_RAW));
    GP_TRY_RC(p->part.alloc(c, (size_t)(segs * D * 5), DA_RAW));
    GP_TRY_RC(p->tot.alloc(c, (size_t)(D * 5), DA_RAW));
    GP_TRY_RC(p->bad.alloc(c, (size_t)(segs * tiles + 1), DA_RAW));
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
  const long Mp = c->Mp, Dp = c->Dp, D = c->D, d5 = 5 * D;
  const int tiles = (int)((D + SC_DW - 1) / SC_DW);
  long long* totbad = p.bad + (R / SC_SEG) * tiles;
  if (unc) GP_TRY_RC(pred_unc_begin(c));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    const int segs = (int)((cnt + SC_SEG - 1) / SC_SEG);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X_mu).uncertain(X_S, raw).on_device(resident), n0, cnt, pred_into(k.mu).factors(unc ? nullptr : k.G + Dp, k.ldg)));
    ScoreArgs a;
    a.G = k.G; a.ldg = k.ldg; a.var = nullptr;
    if (unc) {
      GP_TRY_RC(pred_chunk_var_unc(c, cnt, (flags & 1) ? 1.0 / c->beta : 0.0, k.var));
      a.var = k.var;
    }
    if (Y) {
      GP_HIP(c, hipMemcpyAsync(p.Y, Y + n0 * D, (size_t)(cnt * D) * 8, hipMemcpyHostToDevice, st));
      a.Y = p.Y; a.ldy = D;
    } else {
      a.Y = c->Kaug + n0 * c->LDK + Mp; a.ldy = c->LDK;       // the resident Y: the columns of Kaug behind Psi1
    }
    a.obs = nullptr;
    if (observed) {
      GP_HIP(c, hipMemcpyAsync(p.obs, observed + n0 * D, (size_t)(cnt * D), hipMemcpyHostToDevice, st));
      a.obs = p.obs;
    }
    a.cnt = cnt; a.n0 = n0; a.M = c->M; a.Mp = (int)Mp; a.D = (int)D; a.Dp = (int)Dp; a.sf2 = c->sf2; a.noise = (flags & 1) ? 1.0 / c->beta : 0.0;
    a.rowv = p.rowv; a.rowo = p.rowo; a.R = R; a.part = p.part; a.bad = p.bad;
    GP_LAUNCH(c, st, score_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, a);
    GP_LAUNCH(c, st, score_cols_kernel, dim3((unsigned)segs, (unsigned)tiles), dim3(256), 0, a);
    GP_LAUNCH(c, st, score_cols_final_kernel, dim3((unsigned)((d5 + 255) / 256) + 1), dim3(256), 0, p.part, p.bad, segs, tiles, d5, n0 == 0 ? 1 : 0, p.tot,
              totbad);
    if (row_logp) GP_HIP(c, hipMemcpyAsync(row_logp + n0, p.rowo, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (row_sse) GP_HIP(c, hipMemcpyAsync(row_sse + n0, p.rowo + R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (row_chi2) GP_HIP(c, hipMemcpyAsync(row_chi2 + n0, p.rowo + 2 * R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
  }
  long long bad = SC_NONE;
  if (cols) GP_HIP(c, hipMemcpyAsync(cols, p.tot, (size_t)d5 * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipMemcpyAsync(&bad, totbad, 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  if (bad != SC_NONE)
    return fail(c, GP_ERR_NON_FINITE, "gp_predict_score: the predictive variance of a scored entry is not > 0 (first in row %lld): its row's outputs and its "
                "columns' sums are NaN, every other row is valid%s", bad, (flags & 1) ? "" : " (the variance of f can round to zero or below: score y, flags bit 0)");
  return GP_OK;
}

}  // namespace gp
