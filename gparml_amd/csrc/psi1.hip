// Psi1 generation: the packed-record kernels (two columns per lane up to Q = 32, one column per lane up to Q = 64), the generic fallback and their
// dispatch.  Reference: kernel_exp.py:80.
#include "gp_common.h"
#include "fexp.h"

namespace gp {

// Kaug[n][m] = exp(ln c1_n - 1/2 sum_q u_nq (mu_nq - z_mq)^2), u = alpha/(alpha S + 1)   (kernel_exp.py:80)
// z_m lives in registers (QP = Q rounded up to 2, zero padded); the packed per-point records PU[n] = [mu_n | u_n | ln c1_n]
// (written by the prep kernels) are staged through LDS; no guards in the q loop (padding has u = 0).
constexpr int PSI1_ROWS = 128;   // row granule of the shard (Np is a multiple of it): eight 16-row groups.  A workgroup's rows: psi1_kernel takes `nblk` GROUPS, psi1_wide_kernel `nblk` GRANULES
// FIXA (fixed embeddings, every variance zero): u_nq = alpha_q and ln c1 = ln sf2 for every point, so the records carry only
// sqrt(alpha) o mu (scaled while they are staged), z is scaled once per lane and the exponent is -1/2 sum_q (mu' - z')^2:
// 2 Q + 18 issue slots per element instead of 3 Q + 20, and nothing per point depends on the hyper-parameters (the prep
// kernels are skipped from the second evaluation on).
// SL > 0 (int8 phase 1, p1i8.hip; only the WC = 4 form, where a wave walks all 16 rows of a group): the element is also written as SL signed
// 7-bit digits of t = Psi1 / (2 sf2) in (0, 1/2], sixteen consecutive rows packed into one 16-byte store per column and digit.
// The exponent sum and the record staging are written out here and again in psi1_wide_kernel: as a shared __forceinline__ function / struct they changed
// this kernel's instructions in the <10, false> and int8 forms (profiles/psi1_forms_asm_identity.txt), so each kernel keeps its own text.
template <int QP, bool FIXA, int SL = 0, bool TEMPORAL = false>
__global__ void __launch_bounds__(256) psi1_kernel(const double* __restrict__ PU, const double* __restrict__ Z, double* __restrict__ Kaug,
                                                   long N, long Np, int M, int Mp, int Q, long ld, int WC, const double* __restrict__ alpha,
                                                   double lnsf2, int nblk, int8_t* __restrict__ Sl = nullptr, long strideJ = 0, double hscale = 0.0,
                                                   double* __restrict__ Dpart = nullptr) {
  // A workgroup writes 16 rows x 512 columns: wave w owns 128 columns (two adjacent per lane -> one 16-byte store per lane),
  // so a row's 4 KB leave the CU together (one DRAM page) instead of from four workgroups on four XCDs.  The rows' packed
  // [mu | u | lnc1] records are staged in LDS (below).
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // WC = waves across the columns (4 for Mp >= 512; 1 or 2 for narrower matrices, where the other 4 / WC waves take every
  // (4 / WC)-th row of a 16-row group instead of idling: M = 128 ran at a quarter of the rate)
  const int RG = 4 / WC, rg = wave / WC;
  const int col = (blockIdx.x * WC + (wave % WC)) * 128 + 2 * lane;
  const long row0 = blockIdx.y * 16L * nblk;      // nblk = 16-row groups per workgroup (8 per 128-row granule): the per-lane set-up (z, sqrt(alpha)) is paid once
  const bool ok0 = col < M, ok1 = col + 1 < M;
  const ExpTab xt = exp_tab_lane();
  double z0[QP], z1[QP];
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    const double sa = (FIXA && q < Q) ? sqrt(alpha[q]) : 1.0;
    z0[q] = (q < Q && ok0) ? sa * Z[(long)col * Q + q] : 0.0;
    z1[q] = (q < Q && ok1) ? sa * Z[(long)(col + 1) * Q + q] : 0.0;
  }
  constexpr int W = 2 * QP + 2;          // row width of PU (doubles), a multiple of 2
  constexpr int WS = FIXA ? QP : W;      // staged doubles per row
  // Records of 16 rows at a time: one coalesced load into LDS, read back as broadcast operands; the next group's records
  // travel while the current group is computed.  (Per-row scalar loads cost a serial memory round trip per row and held the
  // kernel at 1.9 ms although plain stores reach 5.5 TB/s: tools/ubench/store_ubench.hip.)
  constexpr int GR = 16, RPT = (GR * WS + 255) / 256;
  const int NG = (int)min((long)nblk, (Np - row0) / GR);   // Np is a multiple of 128: whole groups only
  __shared__ double rec_s[2][GR * WS];
  double stage[RPT];
  double dsq0 = 0.0, dsq1 = 0.0;            // SL > 0: sum of squares of the lane's two columns over this workgroup's rows (the exact diagonal of Psi2, p1i8.hip)
  auto fetch = [&](int g, int i) -> double {
    const int e = threadIdx.x + 256 * i;
    if (e >= GR * WS) return 0.0;
    if (!FIXA) return PU[(row0 + GR * g) * W + e];
    const int r = e / QP, q = e - r * QP;
    return (q < Q ? sqrt(alpha[q]) : 0.0) * PU[(row0 + GR * g + r) * W + q];
  };
#pragma unroll
  for (int i = 0; i < RPT; ++i) { const int e = threadIdx.x + 256 * i; if (e < GR * WS) rec_s[0][e] = fetch(0, i); }
  __syncthreads();
  for (int g = 0; g < NG; ++g) {
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) stage[i] = fetch(g + 1, i);
    }
    const double* recs = rec_s[g & 1];
    // the rows of the group: rg, rg + RG, ... in a loop; SL > 0: all 16 by this wave (RG = 1), unrolled, so that the digits of the two columns collect in
    // 2 SL x 4 registers, one 16-byte store per digit and column (without digits pk0 / pk1 are unused [1][4] arrays: the price of one loop for both)
    constexpr bool ALL = SL > 0;
    unsigned pk0[ALL ? SL : 1][GR / 4], pk1[ALL ? SL : 1][GR / 4];
    if constexpr (ALL) {
#pragma unroll
      for (int j = 0; j < SL; ++j)
#pragma unroll
        for (int w = 0; w < GR / 4; ++w) { pk0[j][w] = 0u; pk1[j][w] = 0u; }
    }
#pragma unroll(ALL ? GR : 1)
    for (int r = ALL ? 0 : rg; r < GR; r += ALL ? 1 : RG) {
      const long n = row0 + GR * g + r;       // Np is a multiple of 128: always in range
      const double* row = recs + r * WS;
      double e0 = 0.0, e1 = 0.0;
#pragma unroll
      for (int q = 0; q < QP; ++q) {
        const double d0 = row[q] - z0[q], d1 = row[q] - z1[q];
        if (FIXA) {
          e0 = fma(d0, d0, e0);
          e1 = fma(d1, d1, e1);
        } else {
          e0 = fma(row[QP + q] * d0, d0, e0);
          e1 = fma(row[QP + q] * d1, d1, e1);
        }
      }
      const double l0 = FIXA ? lnsf2 : row[2 * QP];
      const double x0 = fexp_t(fma(-0.5, e0, l0), xt), x1 = fexp_t(fma(-0.5, e1, l0), xt);   // all lanes (cross-lane table lookup), then select
      double2 v;
      v.x = (n < N && ok0) ? x0 : 0.0;
      v.y = (n < N && ok1) ? x1 : 0.0;
      // non-temporal (one global_store_dwordx4 ... nt per lane): the 4.1 GB of Psi1 is next read after the whole array has been written,
      // so keeping it in L2 / MALL only evicts what the statistics kernels are about to use -- same-box A/B (three rounds): this kernel
      // 0.912 -> 0.932 ms, but p1v2_kernel 5.860 -> 5.795 and p2_fast8_kernel 10.051 -> 9.995 ms: evaluation 17.457 -> 17.354 ms
      // ... on a SHORT shard (temporal: [Psi1 | Y] <= 200 MB) plain stores: 50.6 -> 45.3 us at N = 1e5, M = 128 on one box (the kernels behind it do not change)
      // (a compile-time switch: as a run-time branch it broke the merge of the two non-temporal stores into one 16-byte store -- 0.96 -> 2.28 ms at N = 1e6)
      if (col < Mp) {
        if constexpr (TEMPORAL) *reinterpret_cast<double2*>(&Kaug[n * ld + col]) = v;
        else { __builtin_nontemporal_store(v.x, &Kaug[n * ld + col]); __builtin_nontemporal_store(v.y, &Kaug[n * ld + col + 1]); }
      }
      if constexpr (ALL) {
        dsq0 = fma(v.x, v.x, dsq0); dsq1 = fma(v.y, v.y, dsq1);
        // SL rounds of multiply, round to nearest, subtract: symmetric digits in [-64, 64] (mean zero: the dropped tail does not bias the sums; digits
        // cut from the bit fields of one integer lie in [-64, 63] and need a per-element offset hash for that -- r05, removed with the int8 phase 2)
        double t0 = v.x * hscale, t1 = v.y * hscale;
#pragma unroll
        for (int j = 0; j < SL; ++j) {
          t0 *= 128.0; t1 *= 128.0;
          const double g0 = __builtin_rint(t0), g1 = __builtin_rint(t1);
          t0 -= g0; t1 -= g1;
          pk0[j][r >> 2] |= ((unsigned)(int)g0 & 0xffu) << (8 * (r & 3));
          pk1[j][r >> 2] |= ((unsigned)(int)g1 & 0xffu) << (8 * (r & 3));
        }
      }
    }
    if constexpr (ALL) {
      if (col < Mp) {
        int8_t* dst = Sl + (((row0 + GR * g) / 16) * ld + col) * 16;
#pragma unroll
        for (int j = 0; j < SL; ++j) {
          uint4 a0 = {pk0[j][0], pk0[j][1], pk0[j][2], pk0[j][3]}, a1 = {pk1[j][0], pk1[j][1], pk1[j][2], pk1[j][3]};
          *(uint4*)(dst + (long)j * strideJ) = a0;
          *(uint4*)(dst + (long)j * strideJ + 16) = a1;
        }
      }
    }
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) { const int e = threadIdx.x + 256 * i; if (e < GR * WS) rec_s[(g + 1) & 1][e] = stage[i]; }
    }
    __syncthreads();
  }
  if constexpr (SL > 0) {
    if (Dpart && col < Mp) { Dpart[(long)blockIdx.y * Mp + col] = dsq0; Dpart[(long)blockIdx.y * Mp + col + 1] = dsq1; }
  }
}

// Wide latent spaces (33 <= Q <= 64, records padded to QP = 52 / 64): the same kernel with ONE column per lane (z_m is QP
// registers) and four waves = 256 columns per workgroup.  17 <= Q <= 32 (QP = 24 / 32) still fit two columns per lane and use psi1_kernel (142 / 170 VGPRs):
// N = 1e6, M = 512, Q = 30: 2.73 -> 2.47 ms.  Tried here and dropped (r04), all inside 3 % of this form once the fixed-variance arithmetic was used
// (the kernel is VALU-bound, not LDS-bound): the records as scalar loads / SGPR operands instead of LDS broadcasts (4.7 ms at Q = 30: hipcc waits for each
// s_load_dwordx16 right behind its issue); a lane PAIR per column pair with the latent dimensions split between the two lanes and one DPP exchange per
// row (half the LDS reads per output, z in 2 x QP/2 registers: 1.89 vs 1.89 ms at Q = 30, 1.49 vs 1.41 at Q = 20, 1.85 vs 2.03 at Q = 60); the same with
// explicit ds_read_b64 one chunk ahead (slower: 2.9 ms).
// This kernel keeps its own record staging, its own exponent sum (two interleaved chains) and `nblk` in 128-row granules: the staging as a shared struct
// and the 16-row unit each changed its vector instructions (v_mov / v_mad / v_lshl_add counts at QP = 52), and the shared exponent function had no
// second user (psi1_kernel's comment).  Figures: profiles/psi1_forms_asm_identity.txt.
template <int QP, bool FIXA>
__global__ void __launch_bounds__(256) psi1_wide_kernel(const double* __restrict__ PU, const double* __restrict__ Z, double* __restrict__ Kaug,
                                                        long N, long Np, int M, int Mp, int Q, long ld, const double* __restrict__ alpha,
                                                        double lnsf2, int nblk) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = (blockIdx.x * 4 + wave) * 64 + lane;
  const long row0 = blockIdx.y * (long)PSI1_ROWS * nblk;
  const bool ok = col < M;
  const ExpTab xt = exp_tab_lane();
  double z[QP];
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    const double sa = (FIXA && q < Q) ? sqrt(alpha[q]) : 1.0;
    z[q] = (q < Q && ok) ? sa * Z[(long)col * Q + q] : 0.0;
  }
  constexpr int W = 2 * QP + 2, WS = FIXA ? QP : W;
  constexpr int GR = 16, RPT = (GR * WS + 255) / 256;
  const int NG = (int)min((long)nblk * (PSI1_ROWS / GR), (Np - row0) / GR);
  __shared__ double rec_s[2][GR * WS];
  double stage[RPT];
  auto fetch = [&](int g, int i) -> double {
    const int e = threadIdx.x + 256 * i;
    if (e >= GR * WS) return 0.0;
    if (!FIXA) return PU[(row0 + GR * g) * W + e];
    const int r = e / QP, q = e - r * QP;
    return (q < Q ? sqrt(alpha[q]) : 0.0) * PU[(row0 + GR * g + r) * W + q];
  };
#pragma unroll
  for (int i = 0; i < RPT; ++i) { const int e = threadIdx.x + 256 * i; if (e < GR * WS) rec_s[0][e] = fetch(0, i); }
  __syncthreads();
  for (int g = 0; g < NG; ++g) {
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) stage[i] = fetch(g + 1, i);
    }
    const double* recs = rec_s[g & 1];
#pragma unroll 1
    for (int r = 0; r < GR; ++r) {
      const long n = row0 + GR * g + r;
      const double* row = recs + r * WS;
      double e0 = 0.0, e1 = 0.0;               // two partial sums: the chain of QP dependent FMAs is the latency here
#pragma unroll
      for (int q = 0; q < QP; q += 2) {
        const double d0 = row[q] - z[q], d1 = row[q + 1] - z[q + 1];
        if (FIXA) { e0 = fma(d0, d0, e0); e1 = fma(d1, d1, e1); }
        else { e0 = fma(row[QP + q] * d0, d0, e0); e1 = fma(row[QP + q + 1] * d1, d1, e1); }
      }
      const double x = fexp_t(fma(-0.5, e0 + e1, FIXA ? lnsf2 : row[2 * QP]), xt);   // all lanes, then select
      if (col < Mp) Kaug[n * ld + col] = (n < N && ok) ? x : 0.0;
    }
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) { const int e = threadIdx.x + 256 * i; if (e < GR * WS) rec_s[(g + 1) & 1][e] = stage[i]; }
    }
    __syncthreads();
  }
}

// generic fallback (any Q): operands from global memory
__global__ void __launch_bounds__(256) psi1_generic_kernel(const double* __restrict__ mu, const double* __restrict__ U,
                                                           const double* __restrict__ lnc1, const double* __restrict__ Z,
                                                           double* __restrict__ Kaug, long N, long Np, int M, int Q, long ld) {
  const int col = blockIdx.x * 128 + (threadIdx.x & 127);
  const int half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
  const long row0 = blockIdx.y * 64L + half * 32;
  const bool colok = col < M;
  for (int r = 0; r < 32; ++r) {
    const long n = row0 + r;
    double e = 0.0;
    for (int q = 0; q < Q; ++q) {
      const double d = mu[n * Q + q] - (colok ? Z[(long)col * Q + q] : 0.0);
      e = fma(U[n * Q + q] * d, d, e);
    }
    Kaug[n * ld + col] = (n < N && colok) ? exp(lnc1[n] - 0.5 * e) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// Psi1 of `n` points given as [mu | u | ln c1] tables of `rows` (a multiple of 64) rows into out[rows][ld] (columns >= M and rows >= n zero): the
// generic kernel above on buffers the caller owns (gp_predict's chunks)
int launch_psi1_rows(gp_ctx* c, const double* mu, const double* U, const double* lnc1, double* out, long n, long rows, long ld) {
  GP_LAUNCH(c, c->stream, psi1_generic_kernel, dim3(c->Mp / 128, (unsigned)(rows / 64)), dim3(256), 0, mu, U, lnc1, c->Z, out, n, rows, c->M, c->Q, ld);
  return GP_OK;
}

// The record kernels' launch: `grid`, the arguments both families share, then the family's own.  (A macro, so that a refused launch still names the
// instantiation.)
#define PSI1_LAUNCH(kernel, ...) \
  GP_LAUNCH(c, c->stream, kernel, grid, dim3(256), 0, c->PU, c->Z, c->Kaug, (long)c->N, (long)c->Np, c->M, c->Mp, c->Q, (long)c->LDK, __VA_ARGS__)

// 16-row groups per workgroup: 512 rows on large shards (still >= 7 workgroups per CU at N = 1e6), 128 rows below 2^17 rows (64-row workgroups on
// configs[1]'s 1e5 x 128 shard -- every workgroup resident at once -- changed nothing: 43-44 us, r05).  Whole granules: launch_psi1_wide counts those.
constexpr int PSI1_GROUPS_LARGE = 32, PSI1_GROUPS_SMALL = 8;
static_assert(PSI1_GROUPS_LARGE % (PSI1_ROWS / 16) == 0 && PSI1_GROUPS_SMALL % (PSI1_ROWS / 16) == 0, "launch_psi1_wide divides by the groups of a granule");
static int psi1_groups(const gp_ctx* c) { return c->Np >= (1L << 17) ? PSI1_GROUPS_LARGE : PSI1_GROUPS_SMALL; }

template <int QP>
static int launch_psi1(gp_ctx* c, bool fixa) {
  const int WC = c->Mp >= 512 ? 4 : (c->Mp >= 256 ? 2 : 1);
  const int ngrp = psi1_groups(c);
  static const int temporal_env = env_int("GPARML_PSI1_TEMPORAL", -1);
  const int temporal = temporal_env >= 0 ? temporal_env : ((size_t)c->Np * c->LDK * sizeof(double) <= ((size_t)200 << 20) ? 1 : 0);
  const dim3 grid((c->Mp + 128 * WC - 1) / (128 * WC), (unsigned)((c->Np / 16 + ngrp - 1) / ngrp));
  const double* alpha = c->alpha;
  if constexpr (QP <= 16) if (fixa && WC == 4 && c->i8.active) {
    // int8 phase 1 (p1i8.hip): Psi1's digits are written next to Psi1 itself
    int8_t* Sl = nullptr; long strideJ = 0; double* Dpart = nullptr;
    if (p1i8_prepare(c, &Sl, &strideJ, &Dpart, (int)grid.y) == GP_OK) {
      PSI1_LAUNCH((psi1_kernel<QP, true, GP_I8_DIGITS>), WC, alpha, log(c->sf2), ngrp, Sl, strideJ, 0.5 / c->sf2, Dpart);
      return GP_OK;
    }
    c->i8.active = false;
  }
  if (fixa && temporal) PSI1_LAUNCH((psi1_kernel<QP, true, 0, true>), WC, alpha, log(c->sf2), ngrp);
  else if (fixa) PSI1_LAUNCH((psi1_kernel<QP, true>), WC, alpha, log(c->sf2), ngrp);
  else PSI1_LAUNCH((psi1_kernel<QP, false>), WC, alpha, 0.0, ngrp);
  return GP_OK;
}

template <int QP>
static int launch_psi1_wide(gp_ctx* c, bool fixa) {
  const int nblk = psi1_groups(c) / (PSI1_ROWS / 16);     // this kernel counts 128-row granules (whole ones: the static_assert at psi1_groups)
  const dim3 grid((c->Mp + 255) / 256, (unsigned)((c->Np / PSI1_ROWS + nblk - 1) / nblk));
  const double* alpha = c->alpha;
  if (fixa) PSI1_LAUNCH((psi1_wide_kernel<QP, true>), alpha, log(c->sf2), nblk);
  else PSI1_LAUNCH((psi1_wide_kernel<QP, false>), alpha, 0.0, nblk);
  return GP_OK;
}
#undef PSI1_LAUNCH

// Psi1 of the shard's trial point (run_prep_and_generate has prepared it) into Kaug, by the kernel of the latent width.  kfix: the fixed-variance form.
int run_psi1(gp_ctx* c, bool kfix) {
  const int QP = psi1_qp(c->Q);
  if (QP > 16) {
    // two columns per lane as long as 4 QP registers of z fit (psi1_wide_kernel's comment)
    return for_width<24, 32, 52, 64>(c, "wide Psi1 kernel", QP, [&](auto W) {
      if constexpr (W() <= 32) return launch_psi1<W()>(c, kfix);
      else return launch_psi1_wide<W()>(c, kfix);
    });
  }
  if (QP > 0) return for_width<2, 4, 6, 8, 10, 12, 14, 16>(c, "Psi1 kernel", QP, [&](auto W) { return launch_psi1<W()>(c, kfix); });
  return launch_psi1_rows(c, c->mu, c->U, c->lnc1, c->Kaug, c->N, c->Np, c->LDK);
}

}  // namespace gp
