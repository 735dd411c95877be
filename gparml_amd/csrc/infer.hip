// Latent inference for new, partially observed rows (gp_infer_objective, gp_infer_latent), after a global step of this context.
//
// q(u) is frozen at Titsias' optimum of the trained model: W = beta E (M x D), B = Ki - P as in predict.hip.  For a row y with observed columns O
// (|O| = D_o) and q(x) = N(mu, diag S) the bound is
//   L(mu, S) = -D_o/2 ln(2 pi / beta) - beta/2 [ |y_O|^2 - 2 psi1^T v + sum(G o psi2) + D_o sf2 ] - 1/2 sum_q (mu_q^2 + S_q - ln S_q - 1)
//   v = W_O y_O (M),   G = W_O W_O^T - D_o B (M x M, the same for every row of the call).
// Every row is an independent 2Q-dimensional problem: nothing M^3 and nothing D-wide happens per evaluation.
// Once per call:  Eo = the observed columns of E, zero-padded;  G = beta^2 Eo Eo^T - D_o B (one product on the MFMA GEMM core, inf_gfold_kernel);
// per chunk:      V = beta Yo Eo^T (n x M, the GEMM core again) and |y_O|^2.
// Per evaluation: inf_prep_kernel (per-row tables), lea_rows_kernel (lea.hip: LEA of psi2.hip's factorised form), inf_rows_kernel (the hot kernel).
//
// inf_rows_kernel: ONE WAVE PER ROW, lanes = inducing points m.  Everything that depends on the second index m' alone (z_m', z_m'^2, LEA[m']) is
// wave-uniform and arrives through scalar loads; G is read coalesced along m.  psi2 is symmetric, so only m' >= m is generated: G is stored FOLDED,
//   Gf[m'][m] = 2 G[m][m'] (m < m'),  G[m][m] (m = m'),  0 (m > m'),
// built from min/max indices so that both halves of G enter with the same bits.  With T = Gf o psi2 (upper part) and, per lane m,
//   r_m = sum_m' T,   tz_mq = sum_m' T z_m'q,   tzz_mq = sum_m' T z_m'q^2
// the three sums the value and both gradients of the psi2 term need are
//   sum T = sum_m r_m,   sum T (z_m + z_m')_q = sum_m (z_mq r_m + tz_mq),   sum T (z_m + z_m')_q^2 = sum_m (z_mq^2 r_m + 2 z_mq tz_mq + tzz_mq)
// (zb = (z_m + z_m') / 2 of the gradient formulas is half of that sum).  Per generated pair: Q + 1 (exponent) + 17 (exp) + 2 (T, r) + 2 Q FMA-rate
// instructions; M (M + 64) / 2 pairs per row.  The psi1 term and KL are O(M Q) and ride in the same kernel.  No [n][M][M] array, no LDS, no scratch.
// Summation order is fixed (m' ascending per lane, 64-row blocks ascending, one xor butterfly per sum): a row's result does not depend on the other
// rows of the call or on where a chunk boundary falls.  Latent tables are QP wide: 4, 10 or 16 (compile-time, row factors in registers), and a
// multiple of 16 beyond (the plain path: the exponent reads its factors from memory and the pair loop is repeated per 16 latent dimensions).
//
// gp_infer_latent: Moller's scaled conjugate gradient (the algorithm of scg_adapted.py) per row over x = (mu, softplus-raw S), minimising -L; one state
// record per row (lambda, kappa, theta, direction, success flag, ...), three small kernels per iteration and two masked evaluations (the probe for the
// curvature, only after a success, and the trial point).  The host only enqueues; every INF_POLL iterations it reads one integer, the number of rows
// still running.  Finished rows are skipped by the evaluation kernels at once.
//
// gp_infer_objective_rows / gp_infer_latent_rows: the same for rows that each observe their own columns, one G per distinct pattern of a chunk (the
// section "rows that each observe their own columns" below; the row kernel's RAGGED form).
#include "gp_common.h"
#include "fexp.h"
#include "lane_reduce.h"
#include "varpoint.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <unordered_map>

namespace gp {

constexpr int INF_POLL = 8;      // iterations between two reads of the active-row count
constexpr int INF_AHEAD = 4;     // ragged row kernel: elements of G a lane requests ahead of their use

// test hook (gp_debug_set_option "infer_rows"): rows per chunk, rounded up to 128; 0 = the default below
std::atomic<int> g_opt_inf_rows{0};

static inline int inf_qp(int Q) { return Q <= 4 ? 4 : Q <= 10 ? 10 : (int)round_up(Q, 16); }

static long inf_rows_for(const gp_ctx* c, long Dop) {
  const int opt = g_opt_inf_rows.load();
  if (opt > 0) return round_up(opt, TILE);
  // V, LEA and Yo of a chunk stay near 64 MB
  const long per_row = 8L * (2L * c->Mp + Dop);
  return std::max<long>(TILE, std::min<long>(16384, (64L << 20) / per_row / TILE * TILE));
}

// ---- once per call ---------------------------------------------------------------------------------------------------------------------------
// Eo[m][j] = E[m][cols[j]] for m < M, j < Do; zero elsewhere ([Mp][Dop])
__global__ void __launch_bounds__(256) inf_gather_e_kernel(const double* __restrict__ E, const int* __restrict__ cols, int M, int Mp, int Dp, int Do, int Dop,
                                                           double* __restrict__ Eo) {
  const long total = (long)Mp * Dop;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long m = e / Dop;
    const int j = (int)(e - m * Dop);
    Eo[e] = (m < M && j < Do) ? E[m * Dp + cols[j]] : 0.0;
  }
}

// Gf[k][m] from T = beta^2 Eo Eo^T and Inv = [Ki ; P]: element (a, b) = (min, max) of both, so G is symmetric bit for bit before it is folded
__device__ __forceinline__ double inf_gfold_element(const double* __restrict__ T, const double* __restrict__ Inv, int M, int Mp, double Do, long e) {
  const long mm = (long)Mp * Mp;
  const long k = e / Mp, m = e - k * Mp;
  double g = 0.0;
  if (k < M && m <= k) {
    const long u = m * Mp + k;                         // row = the smaller index
    g = T[u] - Do * (Inv[u] - Inv[mm + u]);
    if (m < k) g *= 2.0;
  }
  return g;
}
__global__ void __launch_bounds__(256) inf_gfold_kernel(const double* __restrict__ T, const double* __restrict__ Inv, int M, int Mp, double Do,
                                                        double* __restrict__ Gf) {
  const long mm = (long)Mp * Mp;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < mm; e += (long)gridDim.x * 256L) Gf[e] = inf_gfold_element(T, Inv, M, Mp, Do, e);
}

// ZP = Z, ZZ = Z o Z, both [Mp][QP] zero-padded
__global__ void __launch_bounds__(256) inf_ztab_kernel(const double* __restrict__ Z, int M, int Mp, int Q, int QP, double* __restrict__ ZP,
                                                       double* __restrict__ ZZ) {
  const long total = (long)Mp * QP;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long m = e / QP;
    const int q = (int)(e - m * QP);
    const double z = (m < M && q < Q) ? Z[m * Q + q] : 0.0;
    ZP[e] = z;
    ZZ[e] = z * z;
  }
}

// ---- once per chunk --------------------------------------------------------------------------------------------------------------------------
// Yo [rows][Dop] from the packed observed columns Yc [cnt][Do] (zero padding) and yy[n] = |y_O|^2; one thread per row
__global__ void __launch_bounds__(256) inf_ypad_kernel(const double* __restrict__ Yc, long cnt, long rows, int Do, int Dop, double* __restrict__ Yo,
                                                       double* __restrict__ yy) {
  for (long n = blockIdx.x * 256L + threadIdx.x; n < rows; n += (long)gridDim.x * 256L) {
    double s = 0.0;
    for (int j = 0; j < Dop; ++j) {
      const double y = (n < cnt && j < Do) ? Yc[n * Do + j] : 0.0;
      Yo[n * Dop + j] = y;
      s = fma(y, y, s);
    }
    yy[n] = s;
  }
}

// ---- per evaluation --------------------------------------------------------------------------------------------------------------------------
// Per-row tables of the evaluation point xe[n] = [mu (Q) | S or raw S (Q)], QP wide and zero-padded: TB[n] = [mu | S | u | w | v2] and
// LC[n] = [ln c1, 1/2 ln c2]; u = alpha / (alpha S + 1), w = alpha / (2 alpha S + 1), v2 = (alpha - w) / 2.  One thread per row.
__global__ void __launch_bounds__(256) inf_prep_kernel(const double* __restrict__ xe, int raw, const unsigned char* __restrict__ mask,
                                                       const double* __restrict__ alpha, const double* __restrict__ shift, long cnt, int Q, int QP, double sf2,
                                                       double* __restrict__ TB, double* __restrict__ LC) {
  for (long n = blockIdx.x * 256L + threadIdx.x; n < cnt; n += (long)gridDim.x * 256L) {
    if (mask && !mask[n]) continue;
    double l1 = log(sf2), l2 = l1;
    double* t = TB + n * 5 * QP;
    for (int q = 0; q < QP; ++q) {
      double m = 0.0, s = 0.0, u = 0.0, w = 0.0, v2 = 0.0;
      if (q < Q) {
        const double a = alpha[q];
        m = xe[n * 2 * Q + q] - shift[q];      // centred like the model's Z (gp_ctx::shift); the KL term adds the origin back (inf_rows_kernel)
        s = xe[n * 2 * Q + Q + q];
        if (raw) s = softplus(s);
        const VarQ f = var_q(a, s);
        u = f.u; w = f.w; v2 = f.v2;
        l1 -= var_log1(f);
        l2 -= var_half_log2(f);
      }
      t[q] = m; t[QP + q] = s; t[2 * QP + q] = u; t[3 * QP + q] = w; t[4 * QP + q] = v2;
    }
    LC[2 * n] = l1;
    LC[2 * n + 1] = l2;
  }
}

struct InfDims {
  long cnt;
  int M, Mp, Q, QP, raw;
  double sf2, beta, Do;
};
// the ragged form (gp_infer_*_rows): every row has its own observed set, so its own D_o and its own folded G, entry pat[n] of a table [P][Mp][Mp]
struct InfDimsRows : InfDims {
  const int* pat;      // [cnt] the row's pattern within the chunk's table
  const double* Dor;   // [cnt] the row's D_o
};

// QR: the table width when it is 4, 10 or 16 (one pass, the row factors v2_q z_mq in registers); WIDE: QP a multiple of 16, one pass per 16 latent
// dimensions with the exponent's factors read from the tables
// RAGGED: Gf is the chunk's pattern table and row n reads entry a.pat[n] of it and its own a.Dor[n] (both wave-uniform, loaded once per row); the
// pair loop then keeps the next INF_AHEAD elements of G in flight, because a row whose pattern no other row shares streams its G from HBM
template <int QR, bool WIDE, bool RAGGED>
// (the arrays are separate __restrict__ parameters: only then are the wave-uniform reads scalar loads)
//   xe [cnt][2Q] evaluation points (for the softplus derivative), TB [cnt][5 QP], LC [cnt][2], LEA [cnt][Mp], V [rows][Mp] = beta Yo Eo^T, yy [rows],
//   ZP, ZZ [Mp][QP], Gf [Mp][Mp] (element (m', m) at m' Mp + m), mask (NULL: every row); out: fe [cnt] = L, ge [cnt][2Q] = dL/dmu | dL/dS (or d/d raw), or NULL
__global__ void __launch_bounds__(256) inf_rows_kernel(const double* __restrict__ xe, const double* __restrict__ TB, const double* __restrict__ LC,
                                                       const double* __restrict__ LEA, const double* __restrict__ V, const double* __restrict__ yy,
                                                       const double* __restrict__ ZP, const double* __restrict__ ZZ, const double* __restrict__ Gf,
                                                       const double* __restrict__ shift, const unsigned char* __restrict__ mask, double* __restrict__ fe, double* __restrict__ ge,
                                                       std::conditional_t<RAGGED, InfDimsRows, InfDims> a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long n = blockIdx.x * 4L + wave;                 // wave-uniform
  if (n >= a.cnt) return;
  if (mask && !mask[n]) return;
  const int M = a.M, Mp = a.Mp, Q = a.Q, QP = a.QP;
  const double* tb = TB + n * 5 * QP;                  // wave-uniform: scalar loads
  const double* lea = LEA + n * Mp;
  const double* vrow = V + n * Mp;
  const double lnc1 = LC[2 * n];
  const double* Gn = Gf;
  double Dn = a.Do;
  if constexpr (RAGGED) { Gn = Gf + (long)a.pat[n] * Mp * Mp; Dn = a.Dor[n]; }
  for (int qc = 0; qc < QP; qc += QR) {                  // one trip unless WIDE
    // ---- psi1 term: p_m = psi1_m v_m; b0 = sum p, b1_q = sum p (mu_q - z_mq), b2_q = sum p (mu_q - z_mq)^2
    double b0 = 0.0, b1[QR], b2[QR];
#pragma unroll
    for (int j = 0; j < QR; ++j) b1[j] = b2[j] = 0.0;
    for (int r0 = 0; r0 < M; r0 += 64) {
      const int m = r0 + lane;                           // < Mp
      const double* zm = ZP + (long)m * QP;
      double s = 0.0;
      if constexpr (WIDE) {
        for (int q = 0; q < QP; ++q) { const double d = tb[q] - zm[q]; s = fma(tb[2 * QP + q] * d, d, s); }
      } else {
#pragma unroll
        for (int q = 0; q < QR; ++q) { const double d = tb[q] - zm[q]; s = fma(tb[2 * QP + q] * d, d, s); }
      }
      const double p = m < M ? fexp(lnc1 - 0.5 * s) * vrow[m] : 0.0;
      b0 += p;
#pragma unroll
      for (int j = 0; j < QR; ++j) {
        const double d = tb[qc + j] - zm[qc + j];
        const double pd = p * d;
        b1[j] += pd;
        b2[j] = fma(pd, d, b2[j]);
      }
    }
    // lane j keeps the sums of latent dimension qc + j (one register each instead of QR uniform ones)
    b0 = wave_sum(b0);
    double B1 = 0.0, B2 = 0.0, A1 = 0.0, A2 = 0.0;
#pragma unroll
    for (int j = 0; j < QR; ++j) {
      const double v1 = wave_sum(b1[j]), v2 = wave_sum(b2[j]);
      if (lane == j) { B1 = v1; B2 = v2; }
    }
    // ---- psi2 term, m' >= m only (the folded G)
    double sT = 0.0, a1[QR], a2[QR];
#pragma unroll
    for (int j = 0; j < QR; ++j) a1[j] = a2[j] = 0.0;
    for (int r0 = 0; r0 < M; r0 += 64) {
      const int m = r0 + lane;
      const double lm = lea[m];                          // kPadLog beyond M
      const double* zm = ZP + (long)m * QP;
      double f[QR], tz[QR];
#pragma unroll
      for (int j = 0; j < QR; ++j) { tz[j] = 0.0; if constexpr (!WIDE) f[j] = tb[4 * QP + j] * zm[j]; }
      double r = 0.0;
      const double* gcol = Gn + m;
      // RAGGED: m' in groups of INF_AHEAD, ascending all the same: while a group is worked on, the G elements of the next one are in flight (rows
      // clamped to M - 1: what is loaded beyond the column's end is never used)
      constexpr int STEP = RAGGED ? INF_AHEAD : 1;
      double ga[STEP], gb[STEP];
      if constexpr (RAGGED) {
#pragma unroll
        for (int u = 0; u < STEP; ++u) ga[u] = gcol[(long)min(r0 + u, M - 1) * Mp];
      }
#pragma unroll 1
      for (int k0 = r0; k0 < M; k0 += STEP) {            // wave-uniform m'
        if constexpr (RAGGED) {
#pragma unroll
          for (int u = 0; u < STEP; ++u) gb[u] = gcol[(long)min(k0 + STEP + u, M - 1) * Mp];
        }
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
          const int k = k0 + u;
          if (RAGGED && k >= M) break;
          const double* zk = ZP + (long)k * QP;
          const double* zzk = ZZ + (long)k * QP;
          double s = lm + lea[k];
          if constexpr (WIDE) {
            for (int q = 0; q < QP; ++q) s = fma(tb[4 * QP + q] * zm[q], zk[q], s);
          } else {
#pragma unroll
            for (int q = 0; q < QR; ++q) s = fma(f[q], zk[q], s);
          }
          double g;
          if constexpr (RAGGED) g = ga[u]; else g = gcol[(long)k * Mp];
          const double t = g * fexp(s);                  // exactly 0 for m > m' and for padding rows
          r += t;
#pragma unroll
          for (int j = 0; j < QR; ++j) {
            tz[j] = fma(t, zk[qc + j], tz[j]);
            a2[j] = fma(t, zzk[qc + j], a2[j]);
          }
        }
        if constexpr (RAGGED) {
#pragma unroll
          for (int u = 0; u < STEP; ++u) ga[u] = gb[u];
        }
      }
      sT += r;
#pragma unroll
      for (int j = 0; j < QR; ++j) {
        const double z = zm[qc + j];
        a1[j] += fma(z, r, tz[j]);
        a2[j] += z * fma(z, r, 2.0 * tz[j]);
      }
    }
    sT = wave_sum(sT);
#pragma unroll
    for (int j = 0; j < QR; ++j) {
      const double v1 = wave_sum(a1[j]), v2 = wave_sum(a2[j]);
      if (lane == j) { A1 = v1; A2 = v2; }
    }
    if (qc == 0) {
      double kl = 0.0;
      for (int q = 0; q < Q; ++q) { const double mq = tb[q] + shift[q], sq = tb[QP + q]; kl += mq * mq + sq - log(sq) - 1.0; }      // the caller's mu
      const double L = -0.5 * Dn * log(6.283185307179586477 / a.beta) - 0.5 * a.beta * (yy[n] - 2.0 * b0 + sT + Dn * a.sf2) - 0.5 * kl;
      if (lane == 0 && fe) fe[n] = L;
    }
    const int q = qc + lane;
    if (ge && lane < QR && q < Q) {
      const double mq = tb[q], sq = tb[QP + q], u = tb[2 * QP + q], w = tb[3 * QP + q];
      const double d1mu = -u * B1, d1s = 0.5 * (u * u * B2 - u * b0);
      const double d2mu = -2.0 * w * (mq * sT - 0.5 * A1);
      const double d2s = 2.0 * w * w * (mq * mq * sT - mq * A1 + 0.25 * A2) - w * sT;
      const double gmu = a.beta * d1mu - 0.5 * a.beta * d2mu - (mq + shift[q]);
      double gs = a.beta * d1s - 0.5 * a.beta * d2s - 0.5 * (1.0 - 1.0 / sq);
      if (a.raw) gs *= softplus_slope(xe[n * 2 * Q + Q + q]);
      ge[n * 2 * Q + q] = gmu;
      ge[n * 2 * Q + Q + q] = gs;
    }
  }
}

// ---- the optimiser's state: one record per row -------------------------------------------------------------------------------------------------
enum { IS_F = 0, IS_LAM, IS_MU, IS_KAPPA, IS_SIGMA, IS_THETA, IS_ALPHA, IS_COUNT };      // doubles per row (sc)
enum { II_STATUS = 0, II_SUCCESS, II_NSUCC, II_ITERS, II_COUNT };                        // ints per row (si); status 0 running, 1 gradient below gtol, 2 max_iters
struct ScgArgs {
  long cnt;
  int Q, QP, raw_in, max_iters;
  double gtol;
  double* x;        // [cnt][2Q] current point (mu | raw S)
  double* gn;       // gradient of -L at x
  double* go;       // the one before
  double* d;        // direction
  double* xe;       // evaluation point
  const double* ge; // the evaluation's gradient of L
  const double* fe; // the evaluation's L
  const double* TB; // the evaluation's tables (S in [QP, 2 QP))
  double* Scur;     // [cnt][Q] S at x
  double* sc;       // [cnt][IS_COUNT]
  int* si;          // [cnt][II_COUNT]
  unsigned char* mask;
};

__device__ __forceinline__ double inf_maxabs(const double* g, int n) {
  double m = 0.0;
  for (int i = 0; i < n; ++i) m = fmax(m, fabs(g[i]));
  return m;
}

// after the evaluation at the start: x, f, gradient (chain rule to the raw variances when S was given plainly), direction, status
__global__ void __launch_bounds__(256) inf_scg_init_kernel(ScgArgs a) {
  const int Q = a.Q, n2 = 2 * Q;
  for (long n = blockIdx.x * 256L + threadIdx.x; n < a.cnt; n += (long)gridDim.x * 256L) {
    double* x = a.x + n * n2; double* gn = a.gn + n * n2; double* go = a.go + n * n2; double* d = a.d + n * n2;
    const double* xe = a.xe + n * n2; const double* ge = a.ge + n * n2;
    bool finite = isfinite(a.fe[n]);
    for (int q = 0; q < Q; ++q) {
      const double s = a.TB[n * 5 * a.QP + a.QP + q];
      a.Scur[n * Q + q] = s;
      x[q] = xe[q];
      x[Q + q] = a.raw_in ? xe[Q + q] : (s > 40.0 ? s : log(expm1(s)));     // softplus^-1
      const double gm = -ge[q], gs = a.raw_in ? -ge[Q + q] : -ge[Q + q] * (1.0 - exp(-s));     // dS / d raw = 1 - exp(-S)
      gn[q] = go[q] = gm; d[q] = -gm;
      gn[Q + q] = go[Q + q] = gs; d[Q + q] = -gs;
      finite = finite && isfinite(gm) && isfinite(gs) && isfinite(x[Q + q]);
    }
    double* sc = a.sc + n * IS_COUNT; int* si = a.si + n * II_COUNT;
    sc[IS_F] = -a.fe[n]; sc[IS_LAM] = 1.0; sc[IS_MU] = sc[IS_KAPPA] = sc[IS_SIGMA] = sc[IS_THETA] = sc[IS_ALPHA] = 0.0;
    si[II_SUCCESS] = 1; si[II_NSUCC] = 0; si[II_ITERS] = 0;
    si[II_STATUS] = (finite && inf_maxabs(gn, n2) <= a.gtol) ? 1 : (a.max_iters <= 0 || !finite) ? 2 : 0;
    a.mask[n] = 0;
  }
}

// running rows whose last step succeeded: slope, length and the probe point x + sigma d for the curvature (scg_adapted.py: "if accepted")
__global__ void __launch_bounds__(256) inf_scg_probe_kernel(ScgArgs a) {
  const int n2 = 2 * a.Q;
  for (long n = blockIdx.x * 256L + threadIdx.x; n < a.cnt; n += (long)gridDim.x * 256L) {
    const int* si = a.si + n * II_COUNT;
    const bool go_on = si[II_STATUS] == 0 && si[II_SUCCESS];
    a.mask[n] = go_on ? 1 : 0;
    if (!go_on) continue;
    double* d = a.d + n * n2; const double* gn = a.gn + n * n2; const double* x = a.x + n * n2; double* xe = a.xe + n * n2;
    double mu = 0.0;
    for (int i = 0; i < n2; ++i) mu = fma(d[i], gn[i], mu);
    if (mu >= 0.0) {                                      // not a descent direction: restart along the gradient
      mu = 0.0;
      for (int i = 0; i < n2; ++i) { d[i] = -gn[i]; mu = fma(d[i], gn[i], mu); }
    }
    double kappa = 0.0;
    for (int i = 0; i < n2; ++i) kappa = fma(d[i], d[i], kappa);
    const double sigma = 1.0e-4 / sqrt(kappa);
    for (int i = 0; i < n2; ++i) xe[i] = fma(sigma, d[i], x[i]);
    double* sc = a.sc + n * IS_COUNT;
    sc[IS_MU] = mu; sc[IS_KAPPA] = kappa; sc[IS_SIGMA] = sigma;
  }
}

// running rows: curvature from the probe (after a success), the scale that makes the quadratic positive definite, the trial point x + alpha d
__global__ void __launch_bounds__(256) inf_scg_trial_kernel(ScgArgs a) {
  const int n2 = 2 * a.Q;
  for (long n = blockIdx.x * 256L + threadIdx.x; n < a.cnt; n += (long)gridDim.x * 256L) {
    const int* si = a.si + n * II_COUNT;
    const bool run = si[II_STATUS] == 0;
    const bool probed = run && si[II_SUCCESS];
    a.mask[n] = run ? 1 : 0;
    if (!run) continue;
    const double* d = a.d + n * n2; const double* gn = a.gn + n * n2; const double* x = a.x + n * n2; double* xe = a.xe + n * n2;
    const double* ge = a.ge + n * n2;
    double* sc = a.sc + n * IS_COUNT;
    if (probed) {
      double th = 0.0;
      for (int i = 0; i < n2; ++i) th = fma(d[i], -ge[i] - gn[i], th);
      sc[IS_THETA] = th / sc[IS_SIGMA];
    }
    const double theta = sc[IS_THETA], kappa = sc[IS_KAPPA];
    double lam = sc[IS_LAM];
    double delta = fma(lam, kappa, theta);      // spelt out: tests/infer_scg_ref.py emulates exactly this, one rounding
    if (!(delta > 0.0)) {
      delta = lam * kappa;
      lam = lam - theta / kappa;
    }
    const double alpha = -sc[IS_MU] / delta;
    sc[IS_LAM] = lam; sc[IS_ALPHA] = alpha;
    for (int i = 0; i < n2; ++i) xe[i] = fma(alpha, d[i], x[i]);
  }
}

// running rows: compare the actual with the predicted decrease; only an improving step moves the row; scale, direction and status
__global__ void __launch_bounds__(256) inf_scg_update_kernel(ScgArgs a) {
  const int Q = a.Q, n2 = 2 * Q;
  for (long n = blockIdx.x * 256L + threadIdx.x; n < a.cnt; n += (long)gridDim.x * 256L) {
    int* si = a.si + n * II_COUNT;
    if (si[II_STATUS] != 0) continue;
    double* x = a.x + n * n2; double* gn = a.gn + n * n2; double* go = a.go + n * n2; double* d = a.d + n * n2;
    const double* xe = a.xe + n * n2; const double* ge = a.ge + n * n2;
    double* sc = a.sc + n * IS_COUNT;
    const double ft = -a.fe[n], fp = sc[IS_F], mu = sc[IS_MU], alpha = sc[IS_ALPHA];
    bool finite = isfinite(ft);
    for (int i = 0; i < n2; ++i) finite = finite && isfinite(ge[i]);
    double Delta = 2.0 * (ft - fp) / (alpha * mu);
    if (!finite || !isfinite(Delta)) Delta = -1.0;
    const bool ok = Delta >= 0.0 && ft <= fp;
    int nsucc = si[II_NSUCC];
    if (ok) {
      ++nsucc;
      for (int i = 0; i < n2; ++i) { x[i] = xe[i]; go[i] = gn[i]; gn[i] = -ge[i]; }
      for (int q = 0; q < Q; ++q) a.Scur[n * Q + q] = a.TB[n * 5 * a.QP + a.QP + q];
      sc[IS_F] = ft;
    }
    const int it = ++si[II_ITERS];
    if (ok && inf_maxabs(gn, n2) <= a.gtol) si[II_STATUS] = 1;
    else if (it >= a.max_iters) si[II_STATUS] = 2;
    double lam = sc[IS_LAM];
    if (Delta < 0.25) lam = fmin(4.0 * lam, 1.0e100);
    if (Delta > 0.75) lam = fmax(0.5 * lam, 1.0e-60);
    sc[IS_LAM] = lam;
    if (nsucc == n2) {
      for (int i = 0; i < n2; ++i) d[i] = -gn[i];
      nsucc = 0;
    } else if (ok) {
      double gg = 0.0, og = 0.0;
      for (int i = 0; i < n2; ++i) { gg = fma(gn[i], gn[i], gg); og = fma(go[i], gn[i], og); }
      const double Gamma = (og - gg) / mu;
      for (int i = 0; i < n2; ++i) d[i] = fma(Gamma, d[i], -gn[i]);      // spelt out: tests/infer_scg_ref.py emulates exactly this, one rounding
    }
    si[II_NSUCC] = nsucc;
    si[II_SUCCESS] = ok ? 1 : 0;
  }
}

// one workgroup: *out = number of rows still running
__global__ void __launch_bounds__(256) inf_count_kernel(const int* __restrict__ si, long cnt, int* __restrict__ out) {
  __shared__ int part[256];
  int c = 0;
  for (long n = threadIdx.x; n < cnt; n += 256) c += si[n * II_COUNT + II_STATUS] == 0 ? 1 : 0;
  const int tot = block_sum<256>(part, c);
  if (threadIdx.x == 0) *out = tot;
}

// results of the chunk: out[n] = [mu (Q) | S or raw S (Q) | L | iterations]
__global__ void __launch_bounds__(256) inf_scg_out_kernel(ScgArgs a, double* __restrict__ out) {
  const int Q = a.Q, n2 = 2 * Q;
  for (long n = blockIdx.x * 256L + threadIdx.x; n < a.cnt; n += (long)gridDim.x * 256L) {
    double* o = out + n * (n2 + 2);
    for (int q = 0; q < Q; ++q) {
      o[q] = a.x[n * n2 + q];
      o[Q + q] = a.raw_in ? a.x[n * n2 + Q + q] : a.Scur[n * Q + q];
    }
    o[n2] = -a.sc[n * IS_COUNT + IS_F];
    o[n2 + 1] = (double)a.si[n * II_COUNT + II_ITERS];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// the optimiser's state (gp_infer_latent)
struct InfOpt {
  DevBuf<double> x, gn, go, d, Scur, sc, out;   // current point, gradients, direction, S at x, scalars, results
  DevBuf<unsigned char> mask;   // [rows] rows of the next evaluation
  DevBuf<int> si;               // [rows][4] status, success flag, successes in a row, iterations | the active-row count
};

// the chunk buffers, keyed on (rows per chunk, padded observed columns); the optimiser's state goes with them
struct InfChunk {
  long rows = 0, dop = 0;
  DevBuf<double> Eo;            // [Mp][dop] observed columns of E
  DevBuf<double> Yc, Yo;        // [rows][D_o] observed columns of the chunk as uploaded, [rows][dop] the same zero-padded
  DevBuf<double> yy;            // [rows] |y_O|^2
  DevBuf<double> V, LEA;        // [rows][Mp] beta Yo Eo^T, LEA of the evaluation point
  DevBuf<double> TB;            // [rows][5 QP] mu | S | u | w | v2 of the evaluation point
  DevBuf<double> LC;            // [rows][2] ln c1, 1/2 ln c2
  DevBuf<double> xe, fe, ge;    // the evaluation point [rows][2Q] (mu | S or raw S), L there [rows] and its gradient [rows][2Q]
  std::unique_ptr<InfOpt> opt;
};

struct InfRows;
struct InfRowsDelete { void operator()(InfRows* p) const; };

// the model tables (the plan itself: built by the first call, kept for the context's life)
struct InferPlan {
  DevBuf<int> cols;             // [D] observed output columns of the call
  DevBuf<double> ZP, ZZ;        // [Mp][QP] Z zero-padded to the latent table width, Z o Z
  DevBuf<double> T, Gf;         // [Mp][Mp] beta^2 Eo Eo^T, G = W_O W_O^T - D_o (Ki - P) folded onto m' >= m
  std::unique_ptr<InfChunk> chunk;
  std::unique_ptr<InfRows, InfRowsDelete> ragged;   // gp_infer_*_rows' own buffers
};
void InferPlanDelete::operator()(InferPlan* p) const { delete p; }

// Each group is built aside and published only when complete.  Every element is written before it is read (DA_RAW: NaN-filled in the poison mode).
static int inf_alloc(gp_ctx* c, long R, long Dop, int QP, bool latent) {
  const long Mp = c->Mp, Q = c->Q;
  auto A = [c](auto& b, long n) { return b.alloc(c, (size_t)n, DA_RAW); };
  if (!c->infer) {
    std::unique_ptr<InferPlan, InferPlanDelete> p(new InferPlan());
    GP_TRY_RC(A(p->cols, c->D)); GP_TRY_RC(A(p->ZP, Mp * QP)); GP_TRY_RC(A(p->ZZ, Mp * QP)); GP_TRY_RC(A(p->T, Mp * Mp)); GP_TRY_RC(A(p->Gf, Mp * Mp));
    c->infer = std::move(p);
  }
  InferPlan& p = *c->infer;
  if (!p.chunk || p.chunk->rows != R || p.chunk->dop != Dop) {
    p.chunk.reset();
    auto k = std::make_unique<InfChunk>();
    GP_TRY_RC(A(k->Eo, Mp * Dop)); GP_TRY_RC(A(k->Yc, R * Dop)); GP_TRY_RC(A(k->Yo, R * Dop)); GP_TRY_RC(A(k->yy, R)); GP_TRY_RC(A(k->V, R * Mp));
    GP_TRY_RC(A(k->LEA, R * Mp)); GP_TRY_RC(A(k->TB, R * 5 * QP)); GP_TRY_RC(A(k->LC, R * 2));
    GP_TRY_RC(A(k->xe, R * 2 * Q)); GP_TRY_RC(A(k->fe, R)); GP_TRY_RC(A(k->ge, R * 2 * Q));
    k->rows = R; k->dop = Dop;
    p.chunk = std::move(k);
  }
  if (latent && !p.chunk->opt) {
    auto o = std::make_unique<InfOpt>();
    GP_TRY_RC(A(o->x, R * 2 * Q)); GP_TRY_RC(A(o->gn, R * 2 * Q)); GP_TRY_RC(A(o->go, R * 2 * Q)); GP_TRY_RC(A(o->d, R * 2 * Q)); GP_TRY_RC(A(o->Scur, R * Q));
    GP_TRY_RC(A(o->sc, R * IS_COUNT)); GP_TRY_RC(A(o->out, R * (2 * Q + 2))); GP_TRY_RC(A(o->mask, R));
    GP_TRY_RC(A(o->si, R * II_COUNT + 1));      // the last int: the active-row count
    p.chunk->opt = std::move(o);
  }
  return GP_OK;
}

const double* infer_debug_lea(const gp_ctx* c, long* n) {
  const InfChunk* k = c->infer ? c->infer->chunk.get() : nullptr;
  *n = k ? (long)k->LEA.size() : 0;
  return k ? k->LEA.get() : nullptr;
}

// gp_debug_peek "infer_<t>": the chunk's optimiser state x, gn, go, d ([rows][2Q]), Scur ([rows][Q]), sc ([rows][IS_COUNT]), si ([rows][II_COUNT]
// ints, without the active-row count behind them: *ints set) and its last evaluation xe, ge ([rows][2Q]), fe ([rows]), as gp_infer_latent left them
// (tests/test_gpu_infer_scg.py).  NULL with *cnt = 0 before a gp_infer_latent call has built the state, NULL with *cnt = -1 for an unknown name.
const void* infer_debug_scg(const gp_ctx* c, const char* name, long* cnt, bool* ints) {
  const InfChunk* k = c->infer ? c->infer->chunk.get() : nullptr;
  const InfOpt* o = k ? k->opt.get() : nullptr;
  const char* t = name + 6;          // behind "infer_"
  const long R = k ? k->rows : 0, n2 = 2L * c->Q;
  const void* src = nullptr;
  long per = -1;
  *ints = false;
  auto is = [t](const char* s) { return !std::strcmp(t, s); };
  if (is("x")) { per = n2; if (o) src = o->x.get(); }
  else if (is("gn")) { per = n2; if (o) src = o->gn.get(); }
  else if (is("go")) { per = n2; if (o) src = o->go.get(); }
  else if (is("d")) { per = n2; if (o) src = o->d.get(); }
  else if (is("Scur")) { per = c->Q; if (o) src = o->Scur.get(); }
  else if (is("sc")) { per = IS_COUNT; if (o) src = o->sc.get(); }
  else if (is("si")) { per = II_COUNT; *ints = true; if (o) src = o->si.get(); }
  else if (is("xe")) { per = n2; if (o) src = k->xe.get(); }
  else if (is("ge")) { per = n2; if (o) src = k->ge.get(); }
  else if (is("fe")) { per = 1; if (o) src = k->fe.get(); }
  *cnt = per < 0 ? -1 : src ? R * per : 0;
  return src;
}

static inline unsigned inf_blocks(long n, long cap = 16384) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

// what the ragged form of the row kernel reads in place of the call's one G and D_o (NULL: the shared form)
struct InfRag {
  const double* Gf;    // the chunk's pattern table
  const int* pat;      // [cnt]
  const double* Dor;   // [cnt]
};

// one evaluation of the rows of the chunk that mask selects (NULL: all) at xe
static int inf_evaluate(gp_ctx* c, const InferPlan& p, const InfChunk& k, long cnt, int raw, const unsigned char* mask, bool want_grad, int QP, double Do,
                        const InfRag* rag) {
  hipStream_t st = c->stream;
  const int M = c->M, Mp = c->Mp, Q = c->Q;
  GP_LAUNCH(c, st, inf_prep_kernel, dim3(inf_blocks(cnt)), dim3(256), 0, k.xe, raw, mask, c->alpha, c->shift, cnt, Q, QP, c->sf2, k.TB, k.LC);
  // LEA from the w and v2 sections of TB and the 1/2 ln c2 column of LC
  LeaRows t;
  t.mu = k.TB; t.w = k.TB + 3 * QP; t.v2 = k.TB + 4 * QP; t.ld = 5 * QP; t.lnc2h = k.LC + 1; t.ldl = 2; t.Z = p.ZP; t.ldz = QP; t.Q = Q;
  t.cnt = cnt; t.rows = cnt; t.M = M; t.Mp = Mp; t.mask = mask; t.LE = nullptr; t.LEA = k.LEA;
  GP_TRY_RC(launch_lea_rows(c, st, t));
  InfDims a;
  a.cnt = cnt; a.M = M; a.Mp = Mp; a.Q = Q; a.QP = QP; a.raw = raw; a.sf2 = c->sf2; a.beta = c->beta; a.Do = Do;
  double* ge = want_grad ? k.ge.get() : nullptr;
  const dim3 grid((unsigned)((cnt + 3) / 4));
  // up to 16 latent columns one pass over the row tables at their own width; beyond, 16 columns at a time (width 0 here)
  return for_width<4, 10, 16, 0>(c, "latent inference row kernel", QP <= 16 ? QP : 0, [&](auto W) -> int {
    constexpr bool WIDE = W() == 0;
    constexpr int QR = WIDE ? 16 : W();
    if (rag) {
      InfDimsRows ar;
      static_cast<InfDims&>(ar) = a;
      ar.pat = rag->pat; ar.Dor = rag->Dor;
      GP_LAUNCH(c, st, (inf_rows_kernel<QR, WIDE, true>), grid, dim3(256), 0, k.xe.get(), k.TB.get(), k.LC.get(), k.LEA.get(), k.V.get(), k.yy.get(),
                p.ZP.get(), p.ZZ.get(), rag->Gf, (const double*)c->shift, mask, k.fe.get(), ge, ar);
      return GP_OK;
    }
    GP_LAUNCH(c, st, (inf_rows_kernel<QR, WIDE, false>), grid, dim3(256), 0, k.xe.get(), k.TB.get(), k.LC.get(), k.LEA.get(), k.V.get(), k.yy.get(), p.ZP.get(),
              p.ZZ.get(), p.Gf.get(), (const double*)c->shift, mask, k.fe.get(), ge, a);
    return GP_OK;
  });
}

// what the caller of an entry point handed in.  mode 0: the objective (L, grad_mu, grad_S out, any may be NULL); mode 1: the optimiser (X_mu, X_S
// in/out, L, iters out)
struct InfCall {
  int mode, raw, max_iters;
  double gtol;
  double* X_mu;
  double* X_S;
  double* L;
  double* grad_mu;
  double* grad_S;
  int* iters;
};

// A chunk whose V and yy are in place: rows 0 .. cnt - 1 of the chunk are rows dst[0 .. cnt) of the call.  Uploads their points, evaluates or
// optimises, and writes the results to the caller's rows.  Ends with the stream synchronised.
static int inf_chunk_solve(gp_ctx* c, const InferPlan& p, const InfChunk& k, const InfCall& a, long cnt, const long* dst, int QP, double Do, const InfRag* rag) {
  const long Q = c->Q, R = k.rows;
  hipStream_t st = c->stream;
  std::vector<double> hx((size_t)cnt * 2 * Q), hout;
  for (long i = 0; i < cnt; ++i)
    for (long q = 0; q < Q; ++q) {
      hx[i * 2 * Q + q] = a.X_mu[dst[i] * Q + q];
      hx[i * 2 * Q + Q + q] = a.X_S[dst[i] * Q + q];
    }
  GP_HIP(c, hipMemcpyAsync(k.xe, hx.data(), (size_t)cnt * 2 * Q * 8, hipMemcpyHostToDevice, st));
  if (a.mode == 0) {
    const bool grads = a.grad_mu || a.grad_S;
    GP_TRY_RC(inf_evaluate(c, p, k, cnt, a.raw, nullptr, grads, QP, Do, rag));
    hout.resize((size_t)cnt * (2 * Q + 1));
    double* hl = hout.data() + (size_t)cnt * 2 * Q;
    if (a.L) GP_HIP(c, hipMemcpyAsync(hl, k.fe, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (grads) GP_HIP(c, hipMemcpyAsync(hout.data(), k.ge, (size_t)cnt * 2 * Q * 8, hipMemcpyDeviceToHost, st));
    GP_HIP(c, hipStreamSynchronize(st));
    for (long i = 0; i < cnt; ++i) {
      if (a.L) a.L[dst[i]] = hl[i];
      for (long q = 0; grads && q < Q; ++q) {
        if (a.grad_mu) a.grad_mu[dst[i] * Q + q] = hout[i * 2 * Q + q];
        if (a.grad_S) a.grad_S[dst[i] * Q + q] = hout[i * 2 * Q + Q + q];
      }
    }
    return GP_OK;
  }
  const InfOpt* o = k.opt.get();
  ScgArgs s{};
  s.cnt = cnt; s.Q = (int)Q; s.QP = QP; s.raw_in = a.raw; s.max_iters = a.max_iters; s.gtol = a.gtol;
  s.xe = k.xe; s.ge = k.ge; s.fe = k.fe; s.TB = k.TB;
  s.x = o->x; s.gn = o->gn; s.go = o->go; s.d = o->d; s.Scur = o->Scur; s.sc = o->sc; s.si = o->si; s.mask = o->mask;
  GP_TRY_RC(inf_evaluate(c, p, k, cnt, a.raw, nullptr, true, QP, Do, rag));
  const dim3 rg(inf_blocks(cnt));
  GP_LAUNCH(c, st, inf_scg_init_kernel, rg, dim3(256), 0, s);
  int* d_active = o->si.get() + R * II_COUNT;
  for (int it = 0; it < a.max_iters; ++it) {
    if (it % INF_POLL == 0) {
      int active = 0;
      GP_LAUNCH(c, st, inf_count_kernel, dim3(1), dim3(256), 0, o->si, cnt, d_active);
      GP_HIP(c, hipMemcpyAsync(&active, d_active, sizeof(int), hipMemcpyDeviceToHost, st));
      GP_HIP(c, hipStreamSynchronize(st));
      if (active == 0) break;
    }
    GP_LAUNCH(c, st, inf_scg_probe_kernel, rg, dim3(256), 0, s);
    GP_TRY_RC(inf_evaluate(c, p, k, cnt, 1, o->mask, true, QP, Do, rag));
    GP_LAUNCH(c, st, inf_scg_trial_kernel, rg, dim3(256), 0, s);
    GP_TRY_RC(inf_evaluate(c, p, k, cnt, 1, o->mask, true, QP, Do, rag));
    GP_LAUNCH(c, st, inf_scg_update_kernel, rg, dim3(256), 0, s);
  }
  GP_LAUNCH(c, st, inf_scg_out_kernel, rg, dim3(256), 0, s, o->out.get());
  hout.resize((size_t)cnt * (2 * Q + 2));
  GP_HIP(c, hipMemcpyAsync(hout.data(), o->out, hout.size() * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  for (long i = 0; i < cnt; ++i) {
    const double* r = hout.data() + i * (2 * Q + 2);
    for (long q = 0; q < Q; ++q) { a.X_mu[dst[i] * Q + q] = r[q]; a.X_S[dst[i] * Q + q] = r[Q + q]; }
    if (a.L) a.L[dst[i]] = r[2 * Q];
    if (a.iters) a.iters[dst[i]] = (int)r[2 * Q + 1];
  }
  return GP_OK;
}

// gp_infer_objective (mode 0) / gp_infer_latent (mode 1)
int run_infer(gp_ctx* c, int mode, long n, const double* Y, const int* cols, int n_cols, double* X_mu, double* X_S, int raw, int max_iters, double gtol,
              double* L, double* grad_mu, double* grad_S, int* iters) {
  const long Mp = c->Mp, M = c->M, Q = c->Q, D = c->D;
  const int Do = cols ? n_cols : (int)D;
  const long Dop = round_up(Do, TILE);
  const int QP = inf_qp((int)Q);
  const long R = inf_rows_for(c, Dop);
  GP_TRY_RC(inf_alloc(c, R, Dop, QP, mode == 1));
  const InferPlan& p = *c->infer;
  const InfChunk& k = *p.chunk;
  hipStream_t st = c->stream;
  // ---- once per call: the observed columns, G and the latent tables
  std::vector<int> hc(Do);
  for (int j = 0; j < Do; ++j) hc[j] = cols ? cols[j] : j;
  GP_HIP(c, hipMemcpyAsync(p.cols, hc.data(), (size_t)Do * sizeof(int), hipMemcpyHostToDevice, st));
  GP_LAUNCH(c, st, inf_gather_e_kernel, dim3(inf_blocks(Mp * Dop)), dim3(256), 0, c->gstep.E, p.cols, (int)M, (int)Mp, c->Dp, Do, (int)Dop, k.Eo);
  GP_LAUNCH(c, st, inf_ztab_kernel, dim3(inf_blocks(Mp * QP)), dim3(256), 0, c->Z, (int)M, (int)Mp, (int)Q, QP, p.ZP, p.ZZ);
  GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)Mp, (int)Mp, 1, gemm_of({k.Eo, Dop}, {k.Eo, Dop}, {p.T, Mp}, (int)Dop, c->beta * c->beta)));
  GP_LAUNCH(c, st, inf_gfold_kernel, dim3(inf_blocks(Mp * Mp, 4096)), dim3(256), 0, p.T, c->gstep.Inv, (int)M, (int)Mp, (double)Do, p.Gf);
  // the observed columns of every row, packed on the host: the others are never read
  std::vector<double> yc((size_t)n * Do);
  for (long i = 0; i < n; ++i)
    for (int j = 0; j < Do; ++j) yc[(size_t)i * Do + j] = Y[i * D + hc[j]];
  const InfCall a{mode, raw, max_iters, gtol, X_mu, X_S, L, grad_mu, grad_S, iters};
  std::vector<long> dst((size_t)std::min(n, R));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0), rows = round_up(cnt, TILE);
    std::iota(dst.begin(), dst.begin() + cnt, n0);
    GP_HIP(c, hipMemcpyAsync(k.Yc, yc.data() + (size_t)n0 * Do, (size_t)cnt * Do * 8, hipMemcpyHostToDevice, st));
    GP_LAUNCH(c, st, inf_ypad_kernel, dim3(inf_blocks(rows)), dim3(256), 0, k.Yc, cnt, rows, Do, (int)Dop, k.Yo, k.yy);
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)rows, (int)Mp, 1, gemm_of({k.Yo, Dop}, {k.Eo, Dop}, {k.V, Mp}, (int)Dop, c->beta)));
    GP_TRY_RC(inf_chunk_solve(c, p, k, a, cnt, dst.data(), QP, (double)Do, nullptr));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

// ---- rows that each observe their own columns (gp_infer_objective_rows, gp_infer_latent_rows) ---------------------------------------------------
// The objective is the one above with O the row's own observed set.  What depends on O: v_n = W_{O_n} y_{n,O_n} = W y0_n (y0: y zero-filled where
// unobserved, so V is one product), |y_{O_n}|^2, D_o(n), and G_n = beta^2 E diag(o_n) E^T - D_o(n) (Ki - P), which does not depend on (mu, S): it is
// built once per distinct pattern of a chunk, into a table of folded matrices the row kernel indexes by the row's pattern.
//
// Host: the distinct rows of `observed` are numbered in order of first occurrence, the call's rows are ordered by that number (stably) and the results
// scattered back.  A chunk is a run of that order of at most inf_rows_for rows and at most inf_patterns_for distinct patterns; a pattern whose rows
// straddle a chunk boundary is rebuilt in the next chunk.  Rows of one pattern are adjacent, so their waves share the pattern's G through L2.
//
// Determinism: every product of this path runs on the 128 x 128-tile GEMM kernel without split-k (on_big), whatever the number of rows or patterns in
// the launch -- launch_gemm would otherwise pick the 32 x 32-tile kernel for small launches, whose k order differs -- and each element of a product is a
// sum over k in a fixed order that does not depend on the element's place in its tile or on the batch.  A row's outputs therefore depend on its y,
// pattern, start and the model only.

// the pattern table of a chunk: at most INF_PAT_BYTES of folded matrices (2 GiB: 1024 patterns at Mp = 512, 2 MiB each), a function of Mp alone
constexpr long INF_PAT_BYTES = 2L << 30;
// the unfolded products of the patterns are formed INF_SUB_BYTES at a time (32 patterns at Mp = 512), so that they do not double the table
constexpr long INF_SUB_BYTES = 64L << 20;
// test hook (gp_debug_set_option "infer_patterns"): distinct patterns per chunk; 0 = the default below
std::atomic<int> g_opt_inf_patterns{0};

static long inf_patterns_for(long Mp) {
  const int opt = g_opt_inf_patterns.load();
  return opt > 0 ? opt : std::max<long>(1, INF_PAT_BYTES / (Mp * Mp * 8));
}

// Em[p][m][j] = Eo[m][j] where pattern p observes column j, else 0 ([P][Mp][Dp]; Eo [Mp][Dp] is zero beyond M and D already)
__global__ void __launch_bounds__(256) inf_emask_kernel(const double* __restrict__ Eo, const unsigned char* __restrict__ pmask, int D, int Dp, long md, int P,
                                                        double* __restrict__ Em) {
  const long total = md * P;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long q = e / md, r = e - q * md;
    const int j = (int)(r % Dp);
    Em[e] = (j < D && pmask[q * D + j]) ? Eo[r] : 0.0;
  }
}

// inf_gfold_kernel for a batch of patterns: T [P][Mp][Mp] (only the tiles on or above the diagonal are formed: row <= column is all the fold reads),
// Do [P], Gf [P][Mp][Mp]
__global__ void __launch_bounds__(256) inf_gfold_rows_kernel(const double* __restrict__ T, const double* __restrict__ Inv, int M, int Mp,
                                                             const double* __restrict__ Do, int P, double* __restrict__ Gf) {
  const long mm = (long)Mp * Mp, total = mm * P;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long q = e / mm, r = e - q * mm;
    Gf[e] = inf_gfold_element(T + q * mm, Inv, M, Mp, Do[q], r);
  }
}

// the ragged call's own buffers, beside the chunk buffers (InfChunk at dop = Dp) it shares with the other two entries
struct InfRows {
  long rows = 0, cap = 0, sub = 0;   // rows per chunk; patterns the table holds; patterns per sub-batch of its build
  DevBuf<double> Gf;                 // [cap][Mp][Mp] the chunk's pattern table, every entry folded as InferPlan::Gf
  DevBuf<double> Em, T;              // [sub][Mp][Dp] E o mask_p and [sub][Mp][Mp] beta^2 Em Em^T of a sub-batch
  DevBuf<unsigned char> pmask;       // [cap][D] the chunk's patterns
  DevBuf<double> pDo;                // [cap] their D_o
  DevBuf<int> pat;                   // [rows] the pattern of each row of the chunk
  DevBuf<double> Dor;                // [rows] its D_o
};
void InfRowsDelete::operator()(InfRows* p) const { delete p; }

// after inf_alloc; cap: the patterns a chunk of this call can hold at most (the table only grows)
static int inf_alloc_rows(gp_ctx* c, long R, long cap) {
  InferPlan& p = *c->infer;
  if (p.ragged && p.ragged->rows == R && p.ragged->cap >= cap) return GP_OK;
  const long Mp = c->Mp, sub = std::min(cap, std::max<long>(1, INF_SUB_BYTES / (Mp * Mp * 8)));
  auto A = [c](auto& b, long n) { return b.alloc(c, (size_t)n, DA_RAW); };
  p.ragged.reset();
  std::unique_ptr<InfRows, InfRowsDelete> r(new InfRows());
  GP_TRY_RC(A(r->Gf, cap * Mp * Mp)); GP_TRY_RC(A(r->Em, sub * Mp * c->Dp)); GP_TRY_RC(A(r->T, sub * Mp * Mp)); GP_TRY_RC(A(r->pmask, cap * c->D));
  GP_TRY_RC(A(r->pDo, cap)); GP_TRY_RC(A(r->pat, R)); GP_TRY_RC(A(r->Dor, R));
  r->rows = R; r->cap = cap; r->sub = sub;
  p.ragged = std::move(r);
  return GP_OK;
}

// gp_infer_objective_rows (mode 0) / gp_infer_latent_rows (mode 1); observed (n, D), non-zero = observed, every row with at least one
int run_infer_rows(gp_ctx* c, int mode, long n, const double* Y, const unsigned char* observed, double* X_mu, double* X_S, int raw, int max_iters,
                   double gtol, double* L, double* grad_mu, double* grad_S, int* iters) {
  const long Mp = c->Mp, M = c->M, Q = c->Q, D = c->D, Dp = c->Dp;
  const int QP = inf_qp((int)Q);
  // ---- the patterns in order of first occurrence, and the rows in the order of their patterns
  std::vector<unsigned char> ob((size_t)n * D);
  for (size_t e = 0; e < ob.size(); ++e) ob[e] = observed[e] ? 1 : 0;
  std::unordered_map<std::string, int> number;
  std::vector<int> pid(n);
  std::vector<long> first, members;         // per pattern: its first row, the number of its rows
  for (long i = 0; i < n; ++i) {
    const auto at = number.emplace(std::string(reinterpret_cast<const char*>(ob.data() + i * D), (size_t)D), (int)first.size());
    if (at.second) { first.push_back(i); members.push_back(0); }
    pid[i] = at.first->second;
    ++members[pid[i]];
  }
  const long P_all = (long)first.size();
  std::vector<long> ord(n), next(P_all + 1, 0);
  for (long q = 0; q < P_all; ++q) next[q + 1] = next[q] + members[q];
  for (long i = 0; i < n; ++i) ord[next[pid[i]]++] = i;
  std::vector<double> pdo(P_all, 0.0);
  for (long q = 0; q < P_all; ++q)
    for (long j = 0; j < D; ++j) pdo[q] += ob[first[q] * D + j];
  // ---- buffers
  const long R = inf_rows_for(c, Dp), Pcap = inf_patterns_for(Mp);
  GP_TRY_RC(inf_alloc(c, R, Dp, QP, mode == 1));
  GP_TRY_RC(inf_alloc_rows(c, R, std::min({Pcap, R, P_all})));
  const InferPlan& p = *c->infer;
  const InfChunk& k = *p.chunk;
  const InfRows& r = *p.ragged;
  hipStream_t st = c->stream;
  // ---- once per call: E with its padding zeroed (every column "observed") and the latent tables
  std::vector<int> hc(D);
  std::iota(hc.begin(), hc.end(), 0);
  GP_HIP(c, hipMemcpyAsync(p.cols, hc.data(), (size_t)D * sizeof(int), hipMemcpyHostToDevice, st));
  GP_LAUNCH(c, st, inf_gather_e_kernel, dim3(inf_blocks(Mp * Dp)), dim3(256), 0, c->gstep.E, p.cols, (int)M, (int)Mp, (int)Dp, (int)D, (int)Dp, k.Eo);
  GP_LAUNCH(c, st, inf_ztab_kernel, dim3(inf_blocks(Mp * QP)), dim3(256), 0, c->Z, (int)M, (int)Mp, (int)Q, QP, p.ZP, p.ZZ);
  const InfCall a{mode, raw, max_iters, gtol, X_mu, X_S, L, grad_mu, grad_S, iters};
  const InfRag rag{r.Gf, r.pat, r.Dor};
  std::vector<double> y0, hdo, hpdo;
  std::vector<int> hpat;
  std::vector<unsigned char> hmask;
  for (long i0 = 0, i1; i0 < n; i0 = i1) {
    const int pf = pid[ord[i0]];
    for (i1 = i0; i1 < n && i1 - i0 < R && pid[ord[i1]] - pf < Pcap;) ++i1;
    const long cnt = i1 - i0, rows = round_up(cnt, TILE), P = pid[ord[i1 - 1]] - pf + 1;
    // the chunk's patterns and rows; y zero-filled where unobserved, so that what the caller left there (NaN, anything) never reaches the device
    hmask.resize((size_t)P * D); hpdo.resize(P); hpat.resize(cnt); hdo.resize(cnt); y0.resize((size_t)cnt * D);
    for (long q = 0; q < P; ++q) {
      std::copy_n(ob.data() + first[pf + q] * D, D, hmask.data() + q * D);
      hpdo[q] = pdo[pf + q];
    }
    for (long i = 0; i < cnt; ++i) {
      const long g = ord[i0 + i];
      hpat[i] = pid[g] - pf;
      hdo[i] = pdo[pid[g]];
      for (long j = 0; j < D; ++j) y0[i * D + j] = ob[g * D + j] ? Y[g * D + j] : 0.0;
    }
    GP_HIP(c, hipMemcpyAsync(r.pmask, hmask.data(), hmask.size(), hipMemcpyHostToDevice, st));
    GP_HIP(c, hipMemcpyAsync(r.pDo, hpdo.data(), hpdo.size() * 8, hipMemcpyHostToDevice, st));
    GP_HIP(c, hipMemcpyAsync(r.pat, hpat.data(), hpat.size() * sizeof(int), hipMemcpyHostToDevice, st));
    GP_HIP(c, hipMemcpyAsync(r.Dor, hdo.data(), hdo.size() * 8, hipMemcpyHostToDevice, st));
    GP_HIP(c, hipMemcpyAsync(k.Yc, y0.data(), y0.size() * 8, hipMemcpyHostToDevice, st));
    // the pattern table, a sub-batch of unfolded products at a time
    for (long q0 = 0; q0 < P; q0 += r.sub) {
      const int ps = (int)std::min(r.sub, P - q0);
      GP_LAUNCH(c, st, inf_emask_kernel, dim3(inf_blocks(ps * Mp * Dp)), dim3(256), 0, k.Eo.get(), r.pmask.get() + q0 * D, (int)D, (int)Dp, Mp * Dp, ps, r.Em.get());
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)Mp, (int)Mp, ps,
                            gemm_of({r.Em, Dp, Mp * Dp}, {r.Em, Dp, Mp * Dp}, {r.T, Mp, Mp * Mp}, (int)Dp, c->beta * c->beta).triangle(2).batched(ps).on_big(1)));
      GP_LAUNCH(c, st, inf_gfold_rows_kernel, dim3(inf_blocks(ps * Mp * Mp)), dim3(256), 0, r.T.get(), c->gstep.Inv.get(), (int)M, (int)Mp, r.pDo.get() + q0, ps,
                r.Gf.get() + q0 * Mp * Mp);
    }
    // V = beta Y0 E^T and |y_O|^2 (the unobserved entries add exact zeros)
    GP_LAUNCH(c, st, inf_ypad_kernel, dim3(inf_blocks(rows)), dim3(256), 0, k.Yc, cnt, rows, (int)D, (int)Dp, k.Yo, k.yy);
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)rows, (int)Mp, 1, gemm_of({k.Yo, Dp}, {k.Eo, Dp}, {k.V, Mp}, (int)Dp, c->beta).on_big(1)));
    GP_TRY_RC(inf_chunk_solve(c, p, k, a, cnt, ord.data() + i0, QP, 0.0, &rag));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
