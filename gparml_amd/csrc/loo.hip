// Exact leave-one-out and leave-block-out scoring of the resident training rows on the device (gp_loo_score).
//
// Fixed embeddings, fixed Z, sf2, alpha, beta.  With k_i = psi1(x_i), a_i = Lk^-1 k_i, b_i = La^-1 k_i, m_i = k_i^T W and e_i = y_i - m_i (gp_predict's
// quantities), row i contributes beta k_i k_i^T to A = Kmm + beta Psi2 and k_i y_i^T to Psi1^T Y.  For a block G of g rows, B_G (g, M) the rows b_i:
//   H = beta B_G B_G^T,  S = I - H = L L^T,  X = L^-1
//   E'_G  = S^-1 E_G = X^T (X E_G)                            the residuals of the model that never saw G
//   v'_i  = sf2 - |a_i|^2 + ([S^-1]_ii - 1) / beta (+ 1/beta)   [S^-1]_ii = the squared norm of column i of X
//   lev_i = beta |b_i|^2
// and for g = 1: e' = e / (1 - h), v' = sf2 - |a|^2 + |b|^2 / (1 - h), h = lev.  Every observed entry is then scored as gp_predict_score scores it, by
// the same passes (score_pass.h: the one definition of the terms, the row sums, the column sums and their order) on (e', v').
// Per chunk of gp_predict's pipeline, on the resident rows where they lie (X_mu, and Y in the columns of Kaug behind Psi1):
//   pred_chunk_front, factors on the 128 x 128-tile kernel (on_big: a row's bits do not depend on the chunk it falls in): G = [mean | a | b];
//   block > 1, per tile of 128 / block whole blocks (block-diagonal, so small blocks share one factorisation; `grp` = the tile's rows):
//     loo_s_kernel        S = I - beta B B^T of the tile's rows on the FP64 matrix core (k over M ascending, 128 columns of b staged in LDS at a time),
//                         entries outside the diagonal blocks and rows past the end set to the identity;
//     potrf_trinv128_kernel (potrf128.h, the global step's own, through linalg.hip's potrf_trinv128_tiles): L and X = L^-1 per tile, LDS-resident;
//     loo_solve_kernel    [S^-1]_ii from the columns of X; T = X E and E' = X^T T per 128 columns of D, E in LDS, X read as wave-uniform operands,
//                         k ascending inside the row's block; E' goes to the window buffer [rows][Dp] for the column pass;
//   loo_rows_kernel: one wave per row: |a|^2, |b|^2 (fac_norms), lev, v', and score_row_sums over the observed d;
//   ScoreTotals::add_segments on LooSrc: gp_predict_score's column pass over the window's whole segments -- segments of 128 rows BY GLOBAL ROW INDEX,
//     segments ascending into the running total.  block = 1 recomputes e' from (y, m, 1 - h) as the row pass did (LooSrc::resid).
// Chunks hold whole tiles (rows per chunk: gp_predict's, rounded down to a multiple of grp), so a chunk need not end on a segment: the rows behind
// the last whole segment stay in the window (E', v', mask: moved to its front) and are summed with the next chunk's.  A block's outputs and the
// column sums are therefore the same bits wherever a chunk boundary falls.
// A tile whose S does not factorise: its rows get NaN (E', v'), and so do the column sums they enter; with block <= 64 the tile holds several blocks
// and they share that fate (one factorisation).  A row with v' not > 0: NaN as in gp_predict_score.  Both are noted by the column pass with plain
// stores and an integer minimum; the host reads two integers with the totals, there is no second pass.
// Buffers: LooPlan, built aside and published whole; every element is written before it is read (DA_RAW).
#define POTRF128_NO_KERNEL
#include "potrf128.h"
#include "pred_chunk.h"
#include "score_pass.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int LOO_LOW_TILES = 36;       // 16 x 16 tiles on or below the diagonal of a 128 x 128 tile
constexpr int LOO_S_LDS = NB * PLD * 8;             // loo_s_kernel: 128 rows x 128 columns of b, row stride PLD (potrf128.h: conflict-free operand reads)
constexpr int LOO_SOLVE_LDS = NB * NB * 8;          // loo_solve_kernel: E, then T, [128][128]

// grid (tiles of the chunk), 512 threads.  Tile t holds the chunk's rows t grp .. t grp + grp - 1 (`valid` of them at the chunk's end).
__global__ void __launch_bounds__(512) loo_s_kernel(const double* __restrict__ G, long ldg, int boff, int M, long cnt, int block, int grp, double beta,
                                                    double* __restrict__ S, double* __restrict__ fail, double* __restrict__ logdet) {
  extern __shared__ __attribute__((aligned(16))) double sm[];      // [128][PLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long r0 = (long)blockIdx.x * grp;
  const int valid = (int)min((long)grp, cnt - r0);
  // the wave's 16 x 16 tiles of the lower triangle, row by row: 0 (0,0), 1 (1,0), 2 (1,1), ..; one that meets no diagonal block stays zero
  double acc[5][4];
  int ti[5], tj[5];
  bool need[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int t = wave + 8 * u;
    int r16 = 0, rem = t;
    while (rem > r16) { rem -= r16 + 1; ++r16; }
    ti[u] = r16; tj[u] = rem;
    need[u] = t < LOO_LOW_TILES && 16 * r16 < valid && (16 * rem + 15) / block >= (16 * r16) / block;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[u][j] = 0.0;
  }
  for (int k0 = 0; k0 < M; k0 += NB) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 512 * i, r = e >> 6, cc = 2 * (e & 63);
      double2 v = make_double2(0.0, 0.0);
      if (r < valid) {
        v = *reinterpret_cast<const double2*>(G + (r0 + r) * ldg + boff + k0 + cc);
        if (k0 + cc >= M) v.x = 0.0;
        if (k0 + cc + 1 >= M) v.y = 0.0;
      }
      *reinterpret_cast<double2*>(sm + r * PLD + cc) = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 5; ++u)
      if (need[u]) lds_mma16<true>(sm, 16 * ti[u], 0, 16 * tj[u], 0, 0, NB, lane, acc[u]);
    __syncthreads();
  }
  double* out = S + (long)blockIdx.x * NB * NB;
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    if (wave + 8 * u >= LOO_LOW_TILES) continue;
    const int R = 16 * ti[u] + t16_row(lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int C = 16 * tj[u] + t16_col(j, lane);
      const double delta = R == C ? 1.0 : 0.0;
      const bool in = R < valid && C < valid && R / block == C / block;
      out[R * NB + C] = in ? fma(-beta, acc[u][j], delta) : delta;
    }
  }
  if (tid == 0) { fail[blockIdx.x] = 0.0; logdet[blockIdx.x] = 0.0; }
}

// grid (tiles of the chunk, ceil(D / 128)), 512 threads: thread (column c, quarter q) owns the rows 32 q .. 32 q + 31 of column c.
// X = L^-1 of the tile is lower triangular and block-diagonal: the k range of a quarter is cut to the blocks its rows lie in (the terms left out are
// products with exact zeros).
__global__ void __launch_bounds__(512) loo_solve_kernel(const double* __restrict__ X, const double* __restrict__ fail, const double* __restrict__ G, long ldg,
                                                        const double* __restrict__ Y, long ldy, long cnt, int block, int grp, int D, int Dp,
                                                        double* __restrict__ Ew, double* __restrict__ sinv) {
  extern __shared__ __attribute__((aligned(16))) double E[];       // [128][128]
  const int tid = threadIdx.x, cc = tid & (NB - 1), q = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int d = blockIdx.y * NB + cc;
  const long r0 = (long)blockIdx.x * grp;
  const int valid = (int)min((long)grp, cnt - r0);
  const double* x = X + (long)blockIdx.x * NB * NB;
  const bool bad = fail[blockIdx.x] != 0.0;
  const double nan = __builtin_nan("");
  if (blockIdx.y == 0 && tid < valid) {
    double s = 0.0;
    for (int k = 0; k < NB; ++k) { const double w = x[k * NB + tid]; s = fma(w, w, s); }      // zeros above the diagonal: k < tid adds nothing
    sinv[r0 + tid] = bad ? nan : s;
  }
  const int i0 = 32 * q;
#pragma unroll 4
  for (int r = 0; r < 32; ++r) {
    const int k = i0 + r;
    E[k * NB + cc] = (k < valid && d < D) ? Y[(r0 + k) * ldy + d] - G[(r0 + k) * ldg + d] : 0.0;
  }
  __syncthreads();
  const int klo = i0 / block * block, khi = min(NB, ((i0 + 31) / block + 1) * block);
  double acc[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) acc[r] = 0.0;
  for (int k = klo; k < i0 + 32; ++k) {            // T = X E: row i takes k <= i (X is zero beyond)
    const double e = E[k * NB + cc];
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[r] = fma(x[(i0 + r) * NB + k], e, acc[r]);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 32; ++r) { E[(i0 + r) * NB + cc] = acc[r]; acc[r] = 0.0; }
  __syncthreads();
  for (int k = i0; k < khi; ++k) {                 // E' = X^T T: row i takes k >= i
    const double t = E[k * NB + cc];
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[r] = fma(x[k * NB + i0 + r], t, acc[r]);
  }
  if (d < D) {
#pragma unroll
    for (int r = 0; r < 32; ++r)
      if (i0 + r < valid) Ew[(r0 + i0 + r) * Dp + d] = bad ? nan : acc[r];
  }
}

// The entries of the window: row w = lead + (row of the chunk), lead = the rows of the segment the previous chunk ended in.  e' comes from Ew, or at
// block = 1 (no E' buffer; the window is the chunk: lead = 0) from (y - m) / den; it is scored as score_term(e', 0, v').
struct LooSrc {
  static constexpr int NFLAGS = 2;
  const double* Ew;         // [window][Dp] E', NULL with block = 1
  int Dp;
  const double* G;          // [rows][ldg] the chunk's products [mean | Lk^-1 k | La^-1 k]
  long ldg;
  const double* Y;          // the chunk's resident outputs, row stride ldy
  long ldy;
  double* den;              // [rows] block = 1: 1 - h, NaN when that is not > 0
  const uint8_t* obs;       // [window][D] non-zero = scored; NULL: every entry
  double* vw;               // [window] v'
  uint8_t* stw;             // [window] 1 = the row's S did not factorise
  long rows, g0;            // rows in the window (the column pass: those of its whole segments), global index of its first row (a multiple of SC_SEG)
  int D;
  // e' of window row w, column d; dn: the row's 1 - h (used at block = 1 only)
  __device__ double resid(long w, int d, double dn) const {
#pragma clang fp contract(off)
    if (Ew) return Ew[w * Dp + d];
    return (Y[w * ldy + d] - G[w * ldg + d]) / dn;
  }
  __device__ bool scored(long w, int d) const { return !obs || obs[w * D + d]; }
  __device__ uint8_t unfactorised(long w) const { return stw[w]; }          // the byte as it lies: the column pass tests it after the entry's loads
  __device__ double var(long w, int) const { return vw[w]; }
  __device__ ScoreTerm term(long w, int d) const { return score_term(resid(w, d, Ew ? 0.0 : den[w]), 0.0, vw[w]); }
};
// the row pass's view of its row: v' and 1 - h (NaN when that is not > 0, as the row pass stores it in den) are still in its registers
struct LooRow {
  const LooSrc& s;
  double v, dn;
  __device__ bool scored(long w, int d) const { return s.scored(w, d); }
  __device__ ScoreTerm term(long w, int d) const { return score_term(s.resid(w, d, dn), 0.0, v); }
};

struct LooArgs {
  LooSrc src;
  long cnt;                 // rows of the chunk
  long lead;                // window rows ahead of the chunk's first
  int M, Mp, block, grp;
  double sf2, beta, noise;
  const double* sinv;       // [rows] block > 1: [S^-1]_ii
  const double* fail;       // [tiles] block > 1: non-zero = the tile's S did not factorise
  double* rowo;             // [5][R] row_logp | row_sse | row_chi2 | lev | var_loo of the chunk
  long R;
};

__global__ void __launch_bounds__(256) loo_rows_kernel(LooArgs a) {
#pragma clang fp contract(off)
  const LooSrc& s = a.src;
  const int lane = threadIdx.x & 63;
  const long n = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (n >= a.cnt) return;
  const long w = a.lead + n;
  const FacNorms f = fac_norms(s.G + n * s.ldg, a.M, s.Dp, a.Mp, lane);
  const double h = a.beta * f.b2;
  double den = 1.0 - h, extra;
  bool ok;
  if (a.block == 1) {
    ok = den > 0.0;
    extra = f.b2 / den;
  } else {
    ok = a.fail[n / a.grp] == 0.0;
    extra = (a.sinv[n] - 1.0) / a.beta;
  }
  const double nan = __builtin_nan("");
  const double vrow = ok ? a.sf2 - f.a2 + extra + a.noise : nan;
  const double dn = ok ? den : nan;
  if (lane == 0) {
    if (a.block == 1) s.den[n] = dn;
    s.vw[w] = vrow;
    s.stw[w] = ok ? 0 : 1;
  }
  const RowSums r = score_row_sums(LooRow{s, vrow, dn}, w, s.D, lane);
  if (lane == 0) {
    a.rowo[n] = r.lp;
    a.rowo[a.R + n] = r.sse;
    a.rowo[2 * a.R + n] = r.chi;
    a.rowo[3 * a.R + n] = h;
    a.rowo[4 * a.R + n] = vrow;
  }
}

// the buffers of a call: rows = gp_predict's chunk length, grp = the rows of a factorisation tile (0: block = 1, nothing to factorise); replaced whole
// when either changes.  The window buffers hold up to SC_SEG - 1 rows of the previous chunk ahead of the chunk's own.
struct LooPlan {
  long rows = 0;
  int grp = 0;
  DevBuf<double> rowo;        // [5][rows]
  DevBuf<double> den;         // [rows] 1 - h (block = 1)
  DevBuf<double> sinv;        // [rows] [S^-1]_ii
  DevBuf<double> vw;          // [SC_SEG + rows] v'
  DevBuf<uint8_t> stw;        // [SC_SEG + rows]
  DevBuf<uint8_t> obs;        // [SC_SEG + rows][D] (first call with a mask)
  DevBuf<double> Ew;          // [SC_SEG + rows][Dp] E'
  DevBuf<double> S, X;        // [tiles][128][128] S -> L, and L^-1
  DevBuf<double> flag;        // [2][tiles] the factorisation's failure flag | its log-determinant (not used)
  ScoreTotals totals;         // rows / SC_SEG + 1 segments, two flags: first row with v' not > 0 | first row whose S did not factorise
  long tiles = 0;
};
void LooPlanDelete::operator()(LooPlan* p) const { delete p; }

static int loo_alloc(gp_ctx* c, long R, int grp, bool mask) {
  const long D = c->D, Dp = c->Dp, W = R + SC_SEG;
  if (!c->loo || c->loo->rows != R || c->loo->grp != grp) {
    c->loo.reset();
    std::unique_ptr<LooPlan, LooPlanDelete> p(new LooPlan());
    GP_TRY_RC(p->rowo.alloc(c, (size_t)(5 * R), DA_RAW));
    GP_TRY_RC(p->den.alloc(c, (size_t)R, DA_RAW));
    GP_TRY_RC(p->vw.alloc(c, (size_t)W, DA_RAW));
    GP_TRY_RC(p->stw.alloc(c, (size_t)W, DA_RAW));
    if (grp) {
      p->tiles = R / grp;
      GP_TRY_RC(p->sinv.alloc(c, (size_t)R, DA_RAW));
      GP_TRY_RC(p->Ew.alloc(c, (size_t)(W * Dp), DA_RAW));
      GP_TRY_RC(p->S.alloc(c, (size_t)(p->tiles * NB * NB), DA_RAW));
      GP_TRY_RC(p->X.alloc(c, (size_t)(p->tiles * NB * NB), DA_RAW));
      GP_TRY_RC(p->flag.alloc(c, (size_t)(2 * p->tiles), DA_RAW));
    }
    GP_TRY_RC(p->totals.alloc(c, R / SC_SEG + 1, D, LooSrc::NFLAGS));
    p->rows = R;
    p->grp = grp;
    c->loo = std::move(p);
  }
  if (mask) GP_TRY_RC(c->loo->obs.grow(c, (size_t)(W * D), DA_RAW));
  return GP_OK;
}

int run_loo_score(gp_ctx* c, int block, const uint8_t* observed, int flags, double* row_logp, double* row_sse, double* row_chi2, double* lev,
                  double* var_loo, double* cols) {
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  const long R = k.rows, n = c->N;
  const int grp = block == 1 ? 0 : NB / block * block;          // whole blocks per 128 x 128 factorisation
  const long Rc = grp ? R / grp * grp : R;                       // whole tiles per chunk (R >= 128 >= grp)
  GP_TRY_RC(loo_alloc(c, R, grp, observed != nullptr));
  const LooPlan& p = *c->loo;
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Dp = c->Dp, D = c->D;
  if (grp) {
    GP_HIP(c, hipFuncSetAttribute((const void*)loo_s_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LOO_S_LDS));
    GP_HIP(c, hipFuncSetAttribute((const void*)loo_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LOO_SOLVE_LDS));
  }
  long lead = 0;
  bool started = false;
  for (long n0 = 0; n0 < n; n0 += Rc) {
    const long cnt = std::min(Rc, n - n0);
    const bool last = n0 + cnt == n;
    GP_TRY_RC(pred_chunk_front(c, pred_at(c->Xmu).on_device(true), n0, cnt, pred_into(k.mu).factors(k.G + Dp, k.ldg).on_big()));
    LooArgs a;
    LooSrc& s = a.src;
    s.G = k.G; s.ldg = k.ldg;
    s.Y = c->Kaug + n0 * c->LDK + Mp; s.ldy = c->LDK;            // the resident Y: the columns of Kaug behind Psi1
    s.Ew = grp ? p.Ew.get() : nullptr; s.Dp = (int)Dp; s.den = p.den; s.obs = nullptr; s.vw = p.vw; s.stw = p.stw;
    s.rows = lead + cnt; s.g0 = n0 - lead; s.D = (int)D;
    a.cnt = cnt; a.lead = lead;
    a.M = c->M; a.Mp = (int)Mp; a.block = block; a.grp = grp ? grp : 1;
    a.sf2 = c->sf2; a.beta = c->beta; a.noise = (flags & 1) ? 1.0 / c->beta : 0.0;
    a.sinv = p.sinv; a.fail = p.flag; a.rowo = p.rowo; a.R = R;
    if (grp) {
      const int tiles = (int)((cnt + grp - 1) / grp);
      GP_LAUNCH(c, st, loo_s_kernel, dim3((unsigned)tiles), dim3(512), LOO_S_LDS, (const double*)k.G, k.ldg, (int)(Dp + Mp), c->M, cnt, block, grp, c->beta, p.S.get(),
                p.flag.get(), p.flag + p.tiles);
      GP_TRY_RC(potrf_trinv128_tiles(c, st, tiles, p.S, p.X, p.flag, p.flag + p.tiles));
      GP_LAUNCH(c, st, loo_solve_kernel, dim3((unsigned)tiles, (unsigned)((D + NB - 1) / NB)), dim3(512), LOO_SOLVE_LDS, (const double*)p.X, (const double*)p.flag,
                (const double*)k.G, k.ldg, s.Y, s.ldy, cnt, block, grp, (int)D, (int)Dp, p.Ew + lead * Dp, p.sinv.get());
    }
    if (observed) {
      GP_HIP(c, hipMemcpyAsync(p.obs + lead * D, observed + n0 * D, (size_t)(cnt * D), hipMemcpyHostToDevice, st));
      s.obs = p.obs;
    }
    GP_LAUNCH(c, st, loo_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, a);
    const int segs = (int)(last ? (s.rows + SC_SEG - 1) / SC_SEG : s.rows / SC_SEG);
    if (segs > 0) {
      if (!last) s.rows = (long)segs * SC_SEG;                    // the whole segments; the rest waits for the next chunk
      GP_TRY_RC(p.totals.add_segments(c, st, s, segs, !started));
      started = true;
    }
    double* const outs[5] = {row_logp, row_sse, row_chi2, lev, var_loo};
    for (int o = 0; o < 5; ++o)
      if (outs[o]) GP_HIP(c, hipMemcpyAsync(outs[o] + n0, p.rowo + o * R, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    // the rows behind the last whole segment wait at the window's front for the next chunk's (source and destination never overlap: the source
    // starts at least SC_SEG rows in, fewer than SC_SEG rows move)
    const long done = (long)segs * SC_SEG, tail = last ? 0 : lead + cnt - done;
    if (tail > 0 && done > 0) {
      GP_HIP(c, hipMemcpyAsync(p.vw, p.vw + done, (size_t)tail * 8, hipMemcpyDeviceToDevice, st));
      GP_HIP(c, hipMemcpyAsync(p.stw, p.stw + done, (size_t)tail, hipMemcpyDeviceToDevice, st));
      if (grp) GP_HIP(c, hipMemcpyAsync(p.Ew, p.Ew + done * Dp, (size_t)(tail * Dp) * 8, hipMemcpyDeviceToDevice, st));
      if (observed) GP_HIP(c, hipMemcpyAsync(p.obs, p.obs + done * D, (size_t)(tail * D), hipMemcpyDeviceToDevice, st));
    }
    lead = tail;
  }
  long long bad[2] = {SC_NONE, SC_NONE};
  GP_TRY_RC(p.totals.read(c, st, cols, bad));
  if (bad[1] != SC_NONE)
    return fail(c, GP_ERR_NOT_PD, "gp_loo_score: S = I - beta B B^T of the rows left out does not factorise (first in row %lld): the model without them is "
                "not proper, or the statistics do not contain these rows.  The outputs of the rows factorised with it (its block; with block <= 64 the "
                "%d rows of its tile) and the column sums they enter are NaN, every other row is valid", bad[1], grp ? grp : 1);
  if (bad[0] != SC_NONE) return score_fail_variance(c, "gp_loo_score", "leave-out", bad[0], flags);
  return GP_OK;
}

}  // namespace gp
