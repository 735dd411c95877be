// Posterior predictive mean and variance at new inputs (gp_predict), after a global step of this context.
//
// With Ki = K_mm^-1, P = (K_mm + beta Psi2)^-1, C = Psi1^T Y and E = P C (the global step's refined product), Titsias' optimal q(u) gives
//   W = beta E  (M x D),   B = Ki - P.
// Deterministic inputs x* (X_S == NULL), k* = psi1(x*):
//   mean = k*^T W,   var_f = sf2 - k*^T B k*   (one value per point)
// where k*^T B k* is formed as |Lk^-1 k*|^2 - |La^-1 k*|^2 from the global step's inverse Cholesky factors (Linv = [Lk^-1 ; La^-1], lower):
// two sums of squares of O(sf2) vectors instead of a quadratic form in Ki - P, whose elements are O(cond / sf2) and cancel.
//   Psi1* rows: psi1_rows (psi1.hip's generic Psi1 kernel on prediction-owned buffers);
//   [mean | Lk^-1 k* | La^-1 k*] = Psi1* [beta E | Linv^T]: two products on the MFMA GEMM core (launch_gemm);
//   pred_det_rows_kernel: one wave per point, mean out and var = sf2 - sum of squares + sum of squares (+ 1/beta); the two sums are fac_norms
//     (score_pass.h), the one definition gp_predict_score and gp_loo_score build their variances from too.
// Uncertain inputs x* ~ N(mu*, diag S*), psi1* = psi1(mu*, S*), psi2* = psi2_point(mu*, S*):
//   mean_d = psi1*^T W_d,   var_d = sf2 - tr(B psi2*) + W_d^T psi2* W_d - mean_d^2
//   mean: the same product as above (beta E only);
//   pred_psi2w_kernel: one workgroup per (point, 128 output columns); psi2* is generated tile by tile from the factorised form of psi2.hip's header,
//     psi2[m, m'] = exp(LEA[m] + LEA[m'] + sum_q v2_q z_mq z_m'q),  v2 = (alpha - w) / 2,
//   and fed as the A operand of v_mfma_f64_4x4x4_4b_f64 against E; the epilogue folds the column dot with E and sum(B o psi2) (both in fixed order).
// Nothing of [n][M][M] is ever stored.  Every prediction buffer is owned by the context, allocated on first use and bounded by the chunk size
// (rows points per pass, PredPlan); deleting the context frees them.  The evaluation's buffers are only read: phase 2 / gp_finish after a prediction give the same bits.
#include "pred_chunk.h"
#include "fexp.h"
#include "lane_reduce.h"
#include "score_pass.h"
#include "varpoint.h"
#include <algorithm>
#include <cmath>

namespace gp {

// per point of the chunk (n < rows; rows >= cnt are zero / padding): mu, u = alpha / (alpha S + 1), ln c1 = ln sf2 - 1/2 sum ln(alpha S + 1);
// uncertain inputs also w = alpha / (2 alpha S + 1), v2 = (alpha - w) / 2 and 1/2 ln c2 = ln sf2 - 1/4 sum ln(2 alpha S + 1)
__global__ void __launch_bounds__(256) pred_prep_kernel(const double* __restrict__ Xin, const double* __restrict__ Sin, int raw, const double* __restrict__ alpha,
                                                        const double* __restrict__ shift, long cnt, long rows, int Q, double sf2, double* __restrict__ mu, double* __restrict__ U,
                                                        double* __restrict__ lnc1, double* __restrict__ Wq, double* __restrict__ V2, double* __restrict__ lnc2h) {
  for (long n = blockIdx.x * 256L + threadIdx.x; n < rows; n += (long)gridDim.x * 256L) {
    double l1 = log(sf2), l2 = log(sf2);
    for (int q = 0; q < Q; ++q) {
      const long i = n * Q + q;
      const double a = alpha[q];
      double m = 0.0, s = 0.0;
      if (n < cnt) {
        m = Xin[i] - shift[q];      // centred like the model's Z (gp_ctx::shift)
        if (Sin) { s = Sin[i]; if (raw) s = softplus(s); }
      }
      const VarQ f = var_q(a, s);
      mu[i] = m;
      U[i] = f.u;
      l1 -= var_log1(f);
      if (Wq) { Wq[i] = f.w; V2[i] = f.v2; l2 -= var_half_log2(f); }
    }
    lnc1[n] = l1;
    if (lnc2h) lnc2h[n] = l2;
  }
}

// B = Ki - P on [Mp][Mp], zero outside M x M
__global__ void __launch_bounds__(256) pred_bmat_kernel(const double* __restrict__ Inv, int M, int Mp, double* __restrict__ B) {
  const long mm = (long)Mp * Mp;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < mm; e += (long)gridDim.x * 256L) {
    const long i = e / Mp, j = e - i * Mp;
    B[e] = (i < M && j < M) ? Inv[e] - Inv[mm + e] : 0.0;
  }
}

// deterministic inputs: row n of G = [mean (Dp) | Lk^-1 k* (Mp) | La^-1 k* (Mp)] -> mean[n][0..D), var[n]; one wave per point, fixed summation order
__global__ void __launch_bounds__(256) pred_det_rows_kernel(const double* __restrict__ G, long ldg, long cnt, int M, int Mp, int D, int Dp, double sf2,
                                                            double noise, double* __restrict__ mean, double* __restrict__ var) {
  const int lane = threadIdx.x & 63;
  const long n = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (n >= cnt) return;
  const double* g = G + n * ldg;
  for (int d = lane; d < D; d += 64) mean[n * D + d] = g[d];
  const FacNorms f = fac_norms(g, M, Dp, Mp, lane);
  if (lane == 0) var[n] = sf2 - f.a2 + f.b2 + noise;
}

// C[i][col] = mean[i][col mod D] for i < n and col < used, else 0: the caller's product then adds its terms on top (beta = 1)
__global__ void __launch_bounds__(256) fill_mean_kernel(const double* __restrict__ mean, long n, int D, long rows, long cols, long used, double* __restrict__ C) {
  const long total = rows * cols;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long i = e / cols, col = e - i * cols;
    C[e] = (i < n && col < used) ? mean[i * D + col % D] : 0.0;
  }
}

// the same from a source with a leading dimension (the Jacobian rows of gp_paths_grad): C[i][col] = src[i lds + col mod D]
__global__ void __launch_bounds__(256) fill_rows_kernel(const double* __restrict__ src, long lds, long n, int D, long rows, long cols, long used, double* __restrict__ C) {
  const long total = rows * cols;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long i = e / cols, col = e - i * cols;
    C[e] = (i < n && col < used) ? src[i * lds + col % D] : 0.0;
  }
}

// ---- uncertain inputs: psi2* E on the FP64 matrix core ---------------------------------------------------------------------------------------
// Workgroup (point n, column tile c0 = 128 blockIdx.y), four waves.  A pass covers 64 rows m (16 per wave); for every chunk of PW_KC rows m' the
// workgroup stages E[m'][c0 ..] (pW), z_m' (pZ) and LEA[n][m'] (pL) in LDS, and every wave steps through the chunk four m' at a time:
//   lane l generates psi2[m = row0 + (l & 15)][m' = k + (l >> 4)] (the A-operand element of the 16 x 4 x 4 product, mma_f64.h's lane map),
//   adds B[m][m'] psi2 to its trace partial, and issues 32 MFMAs against the 32 four-column groups of the tile (B operand E[m'][c0 + 4j + (l & 3)]).
// After the pass the accumulators hold (psi2 E)[m][c] for the wave's 16 rows: the epilogue adds E[m][c] (psi2 E)[m][c] to the lane's column partials.
// QR: compile-time width of the row factors v2_q z_mq kept in registers (16 or 64, zero-padded); QR = 0 reads them from memory (any Q).
constexpr int PW_DW = 128;              // output columns per workgroup
constexpr int PW_KC = 32;               // m' rows per LDS chunk
constexpr int PW_LDW = PW_DW + 4;       // padded row stride of the E chunk: the four m' rows of one read land on different banks

struct PsiWArgs {
  const double* LEA;    // [rows][Mp]
  const double* V2;     // [rows][Q]
  const double* Z;      // [Mp][Q] (rows >= M zero)
  const double* E;      // [Mp][Dp]
  const double* B;      // [Mp][Mp]
  const double* G;      // [rows][ldg]: the mean in columns 0 .. D
  long ldg;
  int M, Mp, Q, D, Dp;
  double sf2, beta, noise;
  double* var;          // [cnt][D]
};

template <int QR>
__global__ void __launch_bounds__(256) pred_psi2w_kernel(PsiWArgs a) {
  constexpr int QS = QR > 0 ? QR : 1;
  __shared__ double pW[PW_KC * PW_LDW];
  __shared__ double pZ[PW_KC * QS];
  __shared__ double pL[PW_KC];
  __shared__ double red[4 * PW_DW + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;
  const int c0 = blockIdx.y * PW_DW;
  const int M = a.M, Mp = a.Mp, Q = a.Q;
  const double* lea = a.LEA + n * Mp;
  const double* v2 = a.V2 + n * Q;
  const int kend = (M + PW_KC - 1) / PW_KC * PW_KC;   // <= Mp (Mp is a multiple of 128)
  const int kq = lane >> 4;                           // m' offset inside a four-row step (A and B operands)
  double vpart[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) vpart[j] = 0.0;
  double tr = 0.0;
  for (int r0 = 0; r0 < M; r0 += 64) {
    const int row0 = r0 + 16 * wave;
    const int m = row0 + (lane & 15);                 // < Mp
    const double lm = lea[m];                         // kPadLog beyond M
    double f[QS];
    if constexpr (QR > 0) {
#pragma unroll
      for (int q = 0; q < QR; ++q) f[q] = (q < Q && m < M) ? v2[q] * a.Z[(long)m * Q + q] : 0.0;
    }
    double acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < kend; k0 += PW_KC) {
      __syncthreads();                                // the previous chunk has been consumed
      for (int e = tid; e < PW_KC * PW_DW; e += 256) {
        const int r = e >> 7, cc = e & 127, k = k0 + r, col = c0 + cc;
        pW[r * PW_LDW + cc] = (k < M && col < a.D) ? a.E[(long)k * a.Dp + col] : 0.0;
      }
      if constexpr (QR > 0) {
        for (int e = tid; e < PW_KC * QR; e += 256) {
          const int r = e / QR, q = e - r * QR, k = k0 + r;
          pZ[e] = (k < M && q < Q) ? a.Z[(long)k * Q + q] : 0.0;
        }
      }
      if (tid < PW_KC) pL[tid] = lea[k0 + tid];
      __syncthreads();
      if (row0 < M) {                                 // wave-uniform: a wave whose 16 rows lie beyond M only helps staging
#pragma unroll 1
        for (int kk = 0; kk < PW_KC; kk += 4) {
          const int r = kk + kq, k = k0 + r;
          double s = lm + pL[r];
          if constexpr (QR > 0) {
#pragma unroll
            for (int q = 0; q < QR; ++q) s = fma(f[q], pZ[r * QR + q], s);
          } else {
            const double* zm = a.Z + (long)min(m, M - 1) * Q;
            const double* zk = a.Z + (long)min(k, M - 1) * Q;
            for (int q = 0; q < Q; ++q) s = fma(v2[q] * zm[q], zk[q], s);
          }
          const double x = fexp(s);                   // exactly 0 when m or m' is padding (LEA = kPadLog)
          tr = fma(a.B[(long)m * Mp + k], x, tr);
          const double* wr = pW + r * PW_LDW + (lane & 3);
#pragma unroll
          for (int j = 0; j < 32; ++j) acc[j] = mfma444(x, wr[4 * j], acc[j]);
        }
      }
    }
    if (row0 < M) {
      const int mr = row0 + 4 * ((lane >> 2) & 3) + (lane >> 4);      // the accumulator's row (mma_f64.h lane map)
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const int col = c0 + 4 * j + (lane & 3);
        if (mr < M && col < a.D) vpart[j] = fma(a.E[(long)mr * a.Dp + col], acc[j], vpart[j]);
      }
    }
  }
  // column sums over the lanes of one column (same lane & 3), then over the waves in order
#pragma unroll
  for (int j = 0; j < 32; ++j)
#pragma unroll
    for (int sh = 4; sh < 64; sh <<= 1) vpart[j] += __shfl_xor(vpart[j], sh);
  tr = wave_sum(tr);
  __syncthreads();
  if (lane < 4) {
#pragma unroll
    for (int j = 0; j < 32; ++j) red[wave * PW_DW + 4 * j + lane] = vpart[j];
  }
  if (lane == 0) red[4 * PW_DW + wave] = tr;
  __syncthreads();
  if (tid < PW_DW) {
    const int d = c0 + tid;
    if (d < a.D) {
      const double t = ((red[4 * PW_DW] + red[4 * PW_DW + 1]) + red[4 * PW_DW + 2]) + red[4 * PW_DW + 3];
      const double v = ((red[tid] + red[PW_DW + tid]) + red[2 * PW_DW + tid]) + red[3 * PW_DW + tid];
      const double mean = a.G[n * a.ldg + d];
      a.var[n * a.D + d] = a.sf2 - t + a.beta * a.beta * v - mean * mean + a.noise;
    }
  }
}

// test hook (gp_debug_set_option "predict_rows"): points per chunk, rounded up to 128; 0 = the default below
std::atomic<int> g_opt_pred_rows{0};

static long pred_rows_for(const gp_ctx* c) {
  const int opt = g_opt_pred_rows.load();
  if (opt > 0) return round_up(opt, TILE);
  // the chunk's product buffer [rows][Dp + 2 Mp] stays near 64 MB
  const long per_row = 8L * (c->Dp + 2L * c->Mp);
  return std::max<long>(TILE, std::min<long>(16384, (64L << 20) / per_row / TILE * TILE));
}

// uncertain inputs: built on the first such prediction
struct PredUnc {
  DevBuf<double> W, V2;       // [rows][Q] w = alpha / (2 alpha S + 1), (alpha - w) / 2
  DevBuf<double> lnc2;        // [rows]    1/2 ln c2
  DevBuf<double> LEA;         // [rows][Mp]
  DevBuf<double> B;           // [Mp][Mp]  Ki - P
};

// the chunk buffers, rows points per chunk: replaced whole when the chunk size changes
struct PredPlan {
  long rows = 0;
  DevBuf<double> in;          // [2][rows][Q] X_mu | X_S of the chunk as given
  DevBuf<double> mu, U;       // [rows][Q] mu, alpha / (alpha S + 1)
  DevBuf<double> lnc1;        // [rows]
  DevBuf<double> P1;          // [rows][Mp] Psi1 of the chunk
  DevBuf<double> G;           // [rows][Dp + 2 Mp] [mean | Lk^-1 k* | La^-1 k*]
  DevBuf<double> out;         // [2][rows][D] mean | var
  std::unique_ptr<PredUnc> unc;
};
void PredPlanDelete::operator()(PredPlan* p) const { delete p; }

// Each group is built aside and published only when complete.  Every element of these buffers is written before it is read (DA_RAW: NaN-filled in
// the poison test mode).
static int pred_alloc(gp_ctx* c, bool uncertain) {
  const long R = pred_rows_for(c), Mp = c->Mp, Q = c->Q;
  auto A = [c](DevBuf<double>& b, long n) { return b.alloc(c, (size_t)n, DA_RAW); };
  if (!c->pred || c->pred->rows != R) {
    c->pred.reset();
    std::unique_ptr<PredPlan, PredPlanDelete> p(new PredPlan());
    GP_TRY_RC(A(p->in, 2 * R * Q)); GP_TRY_RC(A(p->mu, R * Q)); GP_TRY_RC(A(p->U, R * Q)); GP_TRY_RC(A(p->lnc1, R));
    GP_TRY_RC(A(p->P1, R * Mp)); GP_TRY_RC(A(p->G, R * (c->Dp + 2 * Mp))); GP_TRY_RC(A(p->out, 2 * R * c->D));
    p->rows = R;
    c->pred = std::move(p);
  }
  if (uncertain && !c->pred->unc) {
    auto u = std::make_unique<PredUnc>();
    GP_TRY_RC(A(u->W, R * Q)); GP_TRY_RC(A(u->V2, R * Q)); GP_TRY_RC(A(u->lnc2, R)); GP_TRY_RC(A(u->LEA, R * Mp)); GP_TRY_RC(A(u->B, Mp * Mp));
    c->pred->unc = std::move(u);
  }
  return GP_OK;
}

const double* pred_debug_lea(const gp_ctx* c, long* n) {
  const PredUnc* u = c->pred ? c->pred->unc.get() : nullptr;
  *n = u ? (long)u->LEA.size() : 0;
  return u ? u->LEA.get() : nullptr;
}

int pred_chunk_open(gp_ctx* c, bool uncertain, PredChunk* k) {
  GP_TRY_RC(pred_alloc(c, uncertain));
  const PredPlan& p = *c->pred;
  *k = PredChunk{p.rows, p.in, p.mu, p.P1, p.G, c->Dp + 2L * c->Mp, p.out + p.rows * c->D};
  return GP_OK;
}

int pred_project(gp_ctx* c, const double* A, long rows, GemmOut e, GemmOut fac, GemmTile tile) {
  const long Mp = c->Mp, Dp = c->Dp;
  if (e.p) GP_TRY_RC(launch_gemm(c, c->stream, K_CONTIG, FREE_CONTIG, (int)rows, (int)Dp, 1, gemm_of({A, Mp}, {c->gstep.E, Dp}, e, (int)Mp, c->beta).on_big(tile)));
  if (fac.p) GP_TRY_RC(launch_gemm(c, c->stream, K_CONTIG, K_CONTIG, (int)rows, (int)(2 * Mp), 1, gemm_of({A, Mp}, {c->gstep.Linv, Mp}, fac, (int)Mp).on_big(tile)));
  return GP_OK;
}

// gp_predict keeps the centred inputs and the factor rows in the chunk's own buffers (PredChunk::mu, G + Dp); joint.hip collects those of all chunks
int pred_chunk_front(gp_ctx* c, const PredIn& in, long n0, long cnt, const PredOut& out) {
  const PredPlan& p = *c->pred;
  const bool unc = in.X_S != nullptr;
  const PredUnc* u = p.unc.get();
  hipStream_t st = c->stream;
  const long R = p.rows, Mp = c->Mp, Dp = c->Dp, Q = c->Q, rows = round_up(cnt, TILE);
  const double* xin = in.device ? in.X_mu + n0 * Q : p.in.get();
  const double* sin = in.device ? (unc ? in.X_S + n0 * Q : nullptr) : p.in + R * Q;
  if (!in.device) {
    GP_HIP(c, hipMemcpyAsync(p.in, in.X_mu + n0 * Q, (size_t)cnt * Q * 8, hipMemcpyHostToDevice, st));
    if (unc) GP_HIP(c, hipMemcpyAsync(p.in + R * Q, in.X_S + n0 * Q, (size_t)cnt * Q * 8, hipMemcpyHostToDevice, st));
  }
  GP_LAUNCH(c, st, pred_prep_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, xin, unc ? sin : (const double*)nullptr, in.raw, c->alpha, c->shift, cnt,
            rows, (int)Q, c->sf2, out.mu, p.U, p.lnc1, unc ? u->W.get() : nullptr, unc ? u->V2.get() : nullptr, unc ? u->lnc2.get() : nullptr);
  GP_TRY_RC(launch_psi1_rows(c, out.mu, p.U, p.lnc1, p.P1, cnt, rows, Mp));
  // mean (and, deterministic inputs, the two inverse-factor products) on the MFMA GEMM core
  return pred_project(c, p.P1, rows, {p.G, Dp + 2 * Mp}, {out.fac, out.ldf}, out.tile);
}

// (the kernel's variance slot goes to the chunk's own variance buffer, which nobody reads before it is written again)
int pred_chunk_mean(gp_ctx* c, long cnt, double* mean) {
  const PredPlan& p = *c->pred;
  GP_LAUNCH(c, c->stream, pred_det_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, p.G, (long)c->Dp + 2L * c->Mp, cnt, 0, c->Mp, c->D, c->Dp, c->sf2,
            0.0, mean, p.out + p.rows * c->D);
  return GP_OK;
}

int pred_fill_mean(gp_ctx* c, const double* mean, long n, long rows, long cols, long used, double* C) {
  GP_LAUNCH(c, c->stream, fill_mean_kernel, dim3((unsigned)blocks_for(rows * cols)), dim3(256), 0, mean, n, c->D, rows, cols, used, C);
  return GP_OK;
}

int pred_fill_rows(gp_ctx* c, const double* src, long lds, long n, long rows, long cols, long used, double* C) {
  GP_LAUNCH(c, c->stream, fill_rows_kernel, dim3((unsigned)blocks_for(rows * cols)), dim3(256), 0, src, lds, n, c->D, rows, cols, used, C);
  return GP_OK;
}

// uncertain inputs, once per call before the first chunk: B = Ki - P of the model as it is now
int pred_unc_begin(gp_ctx* c) {
  const long Mp = c->Mp;
  GP_LAUNCH(c, c->stream, pred_bmat_kernel, dim3((unsigned)std::min<long>((Mp * Mp + 255) / 256, 4096)), dim3(256), 0, c->gstep.Inv, c->M, c->Mp,
            c->pred->unc->B);
  return GP_OK;
}

// the variances [cnt][D] of the chunk pred_chunk_front has just run with uncertain inputs (the plan built with them, pred_unc_begin called), into var
int pred_chunk_var_unc(gp_ctx* c, long cnt, double noise, double* var) {
  const PredPlan& p = *c->pred;
  const PredUnc* u = p.unc.get();
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Dp = c->Dp, M = c->M, Q = c->Q, D = c->D, ldg = Dp + 2 * Mp, rows = round_up(cnt, TILE);
  LeaRows t;
  t.mu = p.mu; t.w = u->W; t.v2 = u->V2; t.ld = Q; t.lnc2h = u->lnc2; t.ldl = 1; t.Z = c->Z; t.ldz = Q; t.Q = (int)Q;
  t.cnt = cnt; t.rows = rows; t.M = (int)M; t.Mp = (int)Mp; t.mask = nullptr; t.LE = nullptr; t.LEA = u->LEA;
  GP_TRY_RC(launch_lea_rows(c, st, t));
  PsiWArgs a;
  a.LEA = u->LEA; a.V2 = u->V2; a.Z = c->Z; a.E = c->gstep.E; a.B = u->B; a.G = p.G; a.ldg = ldg;
  a.M = (int)M; a.Mp = (int)Mp; a.Q = (int)Q; a.D = (int)D; a.Dp = (int)Dp; a.sf2 = c->sf2; a.beta = c->beta; a.noise = noise; a.var = var;
  const dim3 grid((unsigned)cnt, (unsigned)((D + PW_DW - 1) / PW_DW));
  // the latent width the kernel keeps in registers: 16, 64, or (0) a run-time Q beyond
  GP_TRY_RC((for_width<16, 64, 0>(c, "predictive variance kernel", Q <= 16 ? 16 : Q <= 64 ? 64 : 0,
                                  [&](auto W) -> int { GP_LAUNCH(c, st, pred_psi2w_kernel<W()>, grid, dim3(256), 0, a); return GP_OK; })));
  return GP_OK;
}

int run_predict(gp_ctx* c, long n, const double* X_mu, const double* X_S, int raw, int flags, double* mean, double* var) {
  const bool unc = X_S != nullptr;
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, unc, &k));
  hipStream_t st = c->stream;
  const long R = k.rows, D = c->D;
  const double noise = (flags & 1) ? 1.0 / c->beta : 0.0;
  if (unc && var) GP_TRY_RC(pred_unc_begin(c));
  double* out_mean = c->pred->out;
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X_mu).uncertain(X_S, raw), n0, cnt, pred_into(k.mu).factors(!unc && var ? k.G + c->Dp : nullptr, k.ldg)));
    if (!unc && var) {      // mean and variance of deterministic inputs in one kernel
      GP_LAUNCH(c, st, pred_det_rows_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, k.G, k.ldg, cnt, c->M, c->Mp, (int)D, c->Dp, c->sf2, noise, out_mean,
                k.var);
    } else if (mean) GP_TRY_RC(pred_chunk_mean(c, cnt, out_mean));
    if (mean) GP_HIP(c, hipMemcpyAsync(mean + n0 * D, out_mean, (size_t)cnt * D * 8, hipMemcpyDeviceToHost, st));
    if (!unc && var) GP_HIP(c, hipMemcpyAsync(var + n0, k.var, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (unc && var) {
      GP_TRY_RC(pred_chunk_var_unc(c, cnt, noise, k.var));
      GP_HIP(c, hipMemcpyAsync(var + n0 * D, k.var, (size_t)cnt * D * 8, hipMemcpyDeviceToHost, st));
    }
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
