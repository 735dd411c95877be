// Global step: the replicated M x M algebra on the all-reduced statistics.
//   Kmm build (kernels.py:72-113), blocked Cholesky of Kmm and A = Kmm + beta*Psi2 with LDS-resident 128x128
//   diagonal panels, triangular inverse by recursive doubling, explicit inverses (partial_terms.py:60, 95),
//   the bound (partial_terms.py:436-473), its partials (partial_terms.py:102-138), grad_beta (:340-360) and the
//   Kmm-dependent parts of grad_Z / grad_alpha / grad_sf2 (:146-160, 207-240, 247-254, 286-333).
// All matrices are padded to multiples of 128 with an identity block, which leaves log-determinants, inverses
// and every trace unchanged.
#include "gp_common.h"
#include "potrf128.h"
#include "gemm32.h"
#include "lane_reduce.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

namespace gp {

// switches of the global step's extended-precision pieces (default on; environment at load time, gp_debug_set_option at run time: bench.py
// prices them by timing the global step with and without)
std::atomic<int> g_opt_dd_kipsi2{env_flag("GPARML_DD_KIPSI2", true)};
std::atomic<int> g_opt_refine_E{env_flag("GPARML_REFINE_E", true)};

// r05, the global step at M >= 1024 (each switchable for same-box A/B through gp_debug_set_option):
std::atomic<int> g_opt_xtx_tri{1};       // A^-1 = X^T X from its lower tiles, k from the tile's first non-zero row, mirrored store (bit-identical, split or not: tests/test_gpu_linalg.py)
std::atomic<int> g_opt_residual_dd{1};   // the refinement residual through ddacc_block (two rows per wave share E's loads) for Mp >= 256
std::atomic<int> g_opt_trtri_rec{1};     // L^-1 by halves: two batched launches per level instead of two per block row
std::atomic<int> g_opt_gemm_big{1};      // the M x M x {M, D} products on the 128 x 128-tile kernel (split-k 8 at M = 1024) for Mp >= 1024

// split-k factor for a product of `tiles` 128 x 128 output tiles (batch included) with contraction length K on the 128-tile kernel: about 512 workgroups
// (two per CU), a power of two <= 8 that divides the number of k-chunks, and whose partial tiles fit the workspace (cap doubles)
static int choose_splits(long tiles, int K, size_t cap) {
  int s = 8;
  while (s > 1 && (tiles * s > 512 || (K / KC) % s != 0 || (size_t)tiles * s * TILE * TILE > cap)) s >>= 1;
  return s;
}
// The one big-tile / split-k decision of the M x M x {M, D} products and X^T X: the 128 x 128-tile kernel with split-k where that gives >= 256
// workgroups (M >= 1024: 72-74 -> 63 us per product incl. the reduce at M = 1024; at M = 2048 the M x M x M product 616 -> 392 us without a split, the
// M x M x D ones have 128 tiles and lose to the small tiles unless split), the small tiles otherwise.  tiles: 128 x 128 output tiles, batch included;
// cap: doubles of split-k workspace, 0 when there is none (callers pass ws ? capacity : 0; a workspace of no capacity is no workspace: the shared one
// has a floor of 1100 tiles); gemm_big: g_opt_gemm_big.
struct GemmPlan { int big, splits; };
static GemmPlan gemm_plan(long tiles, int K, size_t cap, int gemm_big, int Mp) {
  if (!gemm_big || Mp < 1024 || cap == 0) return {0, 1};
  const int s = choose_splits(tiles, K, cap);
  return tiles * s >= 256 ? GemmPlan{1, s} : GemmPlan{0, 1};
}

// dst[b][r][0:128] = src[b][r][0:128] for r < rows: the panel solve's result from the work panel into the factor (two doubles per thread)
__global__ void __launch_bounds__(256) panel_copy_kernel(const double* __restrict__ src, long sstride, double* __restrict__ dst, long ld, long dstride, long rows) {
  const double* s = src + (long)blockIdx.y * sstride;
  double* d = dst + (long)blockIdx.y * dstride;
  const long total = rows * (NB / 2);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const long r = i / (NB / 2), c2 = i - r * (NB / 2);
    *reinterpret_cast<double2*>(d + r * ld + 2 * c2) = *reinterpret_cast<const double2*>(s + r * NB + 2 * c2);
  }
}

// `tiles` independent 128 x 128 SPD matrices, stored one after the other with row stride 128: each factorised in place (lower factor, upper part
// zeroed), its inverse factor into the same place of Linv.  fail [tiles] and logdet2 [tiles] must hold zeros on entry: the kernel raises / adds.
int potrf_trinv128_tiles(gp_ctx* c, hipStream_t st, int tiles, double* A, double* Linv, double* fail, double* logdet2) {
  GP_HIP(c, hipFuncSetAttribute((const void*)potrf_trinv128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, POTRF_LDS_DOUBLES * 8));
  GP_LAUNCH(c, st, potrf_trinv128_kernel, dim3((unsigned)tiles), dim3(512), POTRF_LDS_DOUBLES * 8, A, (long)NB, (long)NB * NB, 0, Linv, fail, logdet2);
  return GP_OK;
}

// A: [batch][Mp][Mp] SPD in, lower Cholesky factor out (upper zeroed); Linv: L^-1; Inv: A^-1; Twork: batch * Mp * Mp / 2 doubles
int potrf_inverse_batched(gp_ctx* c, hipStream_t st, int Mp, int batch, double* A, double* Linv, double* Inv, double* Twork,
                          double* logdet2, double* fail_flag, double* splitk_ws, size_t splitk_cap, bool factor_only, bool no_inverse) {
  const int nt = Mp / NB;
  const long ld = Mp, bs = (long)Mp * Mp;
  // a per-device attribute: set on every call (cheap) rather than once per process -- contexts may live on several GPUs
  GP_HIP(c, hipFuncSetAttribute((const void*)potrf_trinv128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, POTRF_LDS_DOUBLES * 8));
  // Linv's 128-blocks above the diagonal are never written and are zero from the allocation (gp_create / the test hook)
  for (int j = 0; j < nt; ++j) {
    GP_LAUNCH(c, st, potrf_trinv128_kernel, dim3(batch), dim3(512), POTRF_LDS_DOUBLES * 8, A, ld, bs, j, Linv, fail_flag, logdet2);
    const int rem = nt - j - 1;
    if (rem > 0) {
      double* Lpanel = A + ((long)(j + 1) * NB) * ld + (long)j * NB;
      // panel: L[i,j] = A[i,j] * inv(L_jj)^T, i > j   (rows rem*128, cols 128, k 128) -- through the work panel, see below
      // NOT in place (r06).  Until then C was A itself, and launch_gemm's small-tile path (32 x 32 tiles for <= 256 tiles) ran it with four workgroups per 32 rows,
      // each reading all 128 columns of the rows and overwriting 32 of them: a race that timing hid -- every workgroup resident and in step, the reads over long
      // before the first store -- except on a cold start: the FIRST evaluation of a fresh process at M = 1024 with free embeddings came back with both
      // factorisations flagged in 40-70 % of the processes (NaN from panel 1 on; the evaluator then repeats the step with the reference's 1e-7 jitter: F 2.9e-8,
      // grad_Z 4.1e-6 off -- inside the parity tolerance on a well-conditioned problem; on round 5's failing test_gpu_tile_phase2 shape 9.973e-5, the
      // logged 9.97e-5: that was this, its evaluations run in a fresh child process).  The product goes to the work panel and a copy kernel puts it
      // in place (+ ~5 us per panel; the 128 x 128-tile kernel in place -- one workgroup owns all columns of its rows -- is safe too but costs 20 us per panel).
      // profiles/r06_first_evaluation_race.txt, tests/test_gpu_first_evaluation.py.
      // B(k,c) = Xjj[c][k]: stored [c][k] -> K_CONTIG
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, rem * NB, NB, batch,
                            gemm_of({Lpanel, ld, bs}, {Linv + ((long)j * NB) * ld + (long)j * NB, ld, bs}, {Twork, NB, (long)rem * NB * NB}, NB)));
      GP_LAUNCH(c, st, panel_copy_kernel, dim3((unsigned)std::min<long>(((long)rem * NB * NB / 2 + 255) / 256, 512), batch), dim3(256), 0, (const double*)Twork,
                (long)rem * NB * NB, Lpanel, ld, bs, (long)rem * NB);
      // trailing update: A[i,k] -= L[i,j] L[k,j]^T for i >= k > j (lower tiles); B(k,c) = L[c][k] -> K_CONTIG
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, rem * NB, rem * NB, batch,
                            gemm_of({Lpanel, ld, bs}, {Lpanel, ld, bs}, {A + ((long)(j + 1) * NB) * ld + (long)(j + 1) * NB, ld, bs}, NB, -1.0, 1.0).triangle(1)));
    }
  }
  if (factor_only) return GP_OK;
  if (g_opt_trtri_rec.load()) {
    // X = L^-1 below the diagonal blocks by halves (r05): with L = [L11 0 ; L21 L22], X21 = -X22 (L21 X11).  Level h = 1, 2, 4, ... (half size in
    // 128-blocks): every pair of halves of that size is independent of the others, so a level is TWO batched launches whatever M -- 2 log2(M / 128)
    // launches with M / 256 ... 1 products each instead of 2 (M / 128 - 1) launches of one growing block row (M = 1024: 6 launches for 14, 115 us before).
    // A pair whose second half runs past the matrix (block counts that are no power of two) is launched on its own with the shorter row count.
    for (int h = 1; h < nt; h *= 2) {
      const long b = (long)h * NB, ps = 2 * b * (ld + 1);
      const int full = nt / (2 * h), rem = nt - full * 2 * h - h;
      auto level = [&](int p0, int np, int rows2) -> int {
        const long o11 = ((long)(2 * p0 * h) * NB) * (ld + 1), o22 = o11 + b * (ld + 1), o21 = o11 + b * ld;
        const long m2 = (long)rows2 * NB;
        const GemmOut T = {Twork, b, m2 * b, (long)np * m2 * b};
        // T = L21 X11: L21 [m][k], K_CONTIG; X11 stored [k][c], FREE_CONTIG
        GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)m2, (int)b, np * batch,
                              gemm_of({A + o21, ld, ps, bs}, {Linv + o11, ld, ps, bs}, T, (int)b).batched(np)));
        // X21 = -X22 T: X22 [m][k], K_CONTIG; T stored [k][c], FREE_CONTIG
        GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)m2, (int)b, np * batch,
                              gemm_of({Linv + o22, ld, ps, bs}, {T.p, T.ld, T.s, T.o}, {Linv + o21, ld, ps, bs}, (int)m2, -1.0).batched(np)));
        return GP_OK;
      };
      if (full > 0) GP_TRY_RC(level(0, full, h));
      if (rem > 0) GP_TRY_RC(level(full, 1, rem));
    }
  } else {
    // block rows of X = L^-1: X[i,0:i] = -X_ii * (L[i,0:i] * X[0:i,0:i])
    for (int i = 1; i < nt; ++i) {
      // T = L[i,0:i] X[0:i,0:i]: L row panel (128 x i*128), K_CONTIG; X[0:i,0:i] stored [k][c] -> FREE_CONTIG
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, NB, i * NB, batch,
                            gemm_of({A + ((long)i * NB) * ld, ld, bs}, {Linv, ld, bs}, {Twork, Mp, (long)NB * Mp}, i * NB)));
      // X[i,0:i] = -X_ii T: X_ii, K_CONTIG; T stored [k][c] -> FREE_CONTIG
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, NB, i * NB, batch,
                            gemm_of({Linv + ((long)i * NB) * ld + (long)i * NB, ld, bs}, {Twork, Mp, (long)NB * Mp}, {Linv + ((long)i * NB) * ld, ld, bs}, NB, -1.0)));
    }
  }
  if (no_inverse) return GP_OK;
  // A^-1 = X^T X: A(i,k) = X[k][i]: stored [k][i] -> FREE_CONTIG; B(k,j) = X[k][j] -> FREE_CONTIG.  xtx_tri: lower tiles, klow, mirror
  const int xt = g_opt_xtx_tri.load() ? 1 : 0;
  const GemmPlan pl = gemm_plan((long)(Mp / TILE) * (Mp / TILE) * batch, Mp, splitk_ws ? splitk_cap : 0, g_opt_gemm_big.load(), Mp);
  GP_TRY_RC(launch_gemm(c, st, FREE_CONTIG, FREE_CONTIG, Mp, Mp, batch,
                        gemm_of({Linv, ld, bs}, {Linv, ld, bs}, {Inv, ld, bs}, Mp).triangle(xt, xt, xt).on_big(pl.big).split(pl.splits, splitk_ws)));
  return GP_OK;
}

// ---------------------------------------------------------------------------------------------- global step kernels
// Kmm (kernels.py:108-111) and A = Kmm + beta * Psi2, identity in the padded block
// jitK / jitA: the 1e-7 * I the reference adds when a determinant sign is negative (partial_terms.py:452-456); 0 on the first attempt
__global__ void __launch_bounds__(256) build_kmm_kernel(const double* __restrict__ Z, const double* __restrict__ alpha, double sf2,
                                                         double beta, const double* __restrict__ Psi2, int M, int Mp, int Q,
                                                         double* __restrict__ Kmm, double* __restrict__ A, double* __restrict__ Keep,
                                                         double jitK, double jitA, double* __restrict__ gs_zero, double* __restrict__ Acopy) {
  // workgroup = 16 rows x 64 columns: the 64 columns' inducing points transposed into LDS ([q][column], conflict-free), the row's point wave-uniform
  // (scalar loads); one element per lane and row.  (The first form read Z[k * Q + q] with a stride of Q doubles across the lanes: 37 us at M = 1024,
  // Q = 50.)  The exponent is summed over q in the same order as before: same bits.
  __shared__ double zs[64 * 65];
  __shared__ double as[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k0 = blockIdx.x * 64, i0 = blockIdx.y * 16;
  // the global step's device scalars and failure flags start from zero (this used to be a hipMemsetAsync: a blit dispatch with ~10 us of idle
  // stream around it); the panel kernels that write them are later launches
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid < GS_COUNT + 8) gs_zero[tid] = 0.0;
  const int Qs = Q < 64 ? Q : 64;                     // latent dimensions beyond 64 are read from global memory
  for (int e = tid; e < 64 * Qs; e += 256) {
    const int kk = e / Qs, q = e - kk * Qs;
    zs[q * 65 + kk] = (k0 + kk < M) ? Z[(long)(k0 + kk) * Q + q] : 0.0;
  }
  if (tid < Qs) as[tid] = alpha[tid];
  __syncthreads();
  const int k = k0 + lane;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = i0 + 4 * wave + rr;
    const long idx = (long)i * Mp + k;
    double v;
    if (i < M && k < M) {
      const double* zi = Z + (long)i * Q;
      double e = 0.0;
      for (int q = 0; q < Qs; ++q) {
        const double d = zi[q] - zs[q * 65 + lane];
        e = fma(as[q] * d, d, e);
      }
      for (int q = Qs; q < Q; ++q) {
        const double d = zi[q] - Z[(long)k * Q + q];
        e = fma(alpha[q] * d, d, e);
      }
      v = sf2 * exp(-0.5 * e);
    } else {
      v = (i == k) ? 1.0 : 0.0;
    }
    const bool diag = (i == k) && i < M;
    Kmm[idx] = v + (diag ? jitK : 0.0);
    Keep[idx] = v;
    const double a = ((i < M && k < M) ? fma(beta, Psi2[idx], v) : v) + (diag ? jitA : 0.0);   // the same expression as in solve_residual_kernel
    A[idx] = a;
    if (Acopy) Acopy[idx] = a;                          // the factorisation overwrites A; the double-double residual reads this copy
  }
}

// One step of iterative refinement for E = A^-1 C (A = Kmm + beta Psi2, cond(A) ~ 1e10 at the benchmark's size): R = C - A E with the
// products and the sum carried in double-double (error-free product by FMA, two-sum accumulation), rounded to double at the end; the caller
// then adds P R.  A is rebuilt from Kmm and Psi2 exactly as build_kmm_kernel rounds it (the factorisation overwrote its copy).  One
// workgroup per row m: A[m][k] is wave-uniform, E[k][:] a coalesced row.  With float64 residuals the step is worthless (the residual IS the
// rounding error); with this one the error of grad_Z against an 80-bit evaluation drops from 1.3e-5 to 7.5e-6 at N = 1e6.
// `identity`: C = I (the residual of an inverse: refining P = A^-1 the same way was measured -- no change in grad_Z, +0.17 ms -- and is not done).
// the double-double partial of row m, column d over k in [k0, k1): the chain every quarter of solve_residual_kernel runs (and the fused tail)
__device__ __forceinline__ void residual_chain(const double* __restrict__ krow, const double* __restrict__ prow, const double* __restrict__ E, double beta,
                                               double jitA, int m, int d, int Dp, int k0, int k1, double& hi, double& lo) {
#pragma clang fp contract(off)   // the error-free transformations below must not be fused (hi + a e as one FMA breaks the two-sum)
  hi = 0.0; lo = 0.0;
#pragma unroll 8
  for (int k = k0; k < k1; ++k) {
    const double a = fma(beta, prow[k], krow[k]) + (k == m ? jitA : 0.0);
    const double e = E[(long)k * Dp + d];
    const double pr = a * e, pe = fma(a, e, -pr);           // a e = pr + pe exactly
    const double t = hi + pr, bb = t - hi;                   // two-sum
    lo += ((hi - (t - bb)) + (pr - bb)) + pe;
    hi = t;
  }
}
// (hi, lo) += (x, xl) in double-double
__device__ __forceinline__ void residual_add(double& hi, double& lo, double x, double xl) {
#pragma clang fp contract(off)
  const double t = hi + x, bb = t - hi;
  lo += ((hi - (t - bb)) + (x - bb)) + xl;
  hi = t;
}
__global__ void __launch_bounds__(512) solve_residual_kernel(const double* __restrict__ Keep, const double* __restrict__ Psi2, double beta, double jitA,
                                                             const double* __restrict__ C, const double* __restrict__ E, int M, int Mp, int Dp,
                                                             double* __restrict__ R, int identity) {
#pragma clang fp contract(off)
  // 128 columns x 4 quarters of the contraction range per workgroup: four waves per SIMD hide the latency of the E loads behind each other's
  // two-sum chains (one thread per column, 1024 waves in all: 44 us at M = 512).  The quarter is wave-uniform (readfirstlane), so A[m][k] stays a
  // scalar load.  The four double-double partials are added in order by the first quarter's thread.
  __shared__ double ph[3][128], pl[3][128];
  const int m = blockIdx.x, dl = threadIdx.x & 127, kq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
  const double* krow = Keep + (long)m * Mp;
  const double* prow = Psi2 + (long)m * Mp;
  const int kper = (M + 3) / 4, k0 = kq * kper, k1 = min(M, k0 + kper);
  for (int d0 = 0; d0 < Dp; d0 += 128) {
    const int d = d0 + dl;
    double hi = 0.0, lo = 0.0;
    if (d < Dp) residual_chain(krow, prow, E, beta, jitA, m, d, Dp, k0, k1, hi, lo);
    if (kq > 0) { ph[kq - 1][dl] = hi; pl[kq - 1][dl] = lo; }
    __syncthreads();
    if (kq == 0 && d < Dp) {
#pragma unroll
      for (int j = 0; j < 3; ++j) residual_add(hi, lo, ph[j][dl], pl[j][dl]);
      const double c0 = identity ? (d == m ? 1.0 : 0.0) : C[(long)m * Dp + d];
      R[(long)m * Dp + d] = (c0 - hi) - lo;
    }
    __syncthreads();
  }
}
// the same row by a 256-thread workgroup (Dp = 128): thread (dl, h) runs quarters h + 2 and h one after the other -- the arithmetic of every quarter
// and the order in which the four partials are added are those of solve_residual_kernel.  ph / pl: [3][128] doubles of LDS each.
__device__ __forceinline__ void residual_row256(int m, const double* __restrict__ Keep, const double* __restrict__ Psi2, double beta, double jitA,
                                                const double* __restrict__ C, const double* __restrict__ E, int M, int Mp, int Dp,
                                                double* __restrict__ R, double (*ph)[128], double (*pl)[128]) {
#pragma clang fp contract(off)
  const int dl = threadIdx.x & 127, h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
  const double* krow = Keep + (long)m * Mp;
  const double* prow = Psi2 + (long)m * Mp;
  const int kper = (M + 3) / 4;
  double hi, lo, hi2, lo2;
  { const int kq = h + 2, k0 = kq * kper, k1 = min(M, k0 + kper); residual_chain(krow, prow, E, beta, jitA, m, dl, Dp, k0, k1, hi2, lo2); }
  { const int kq = h, k0 = kq * kper, k1 = min(M, k0 + kper); residual_chain(krow, prow, E, beta, jitA, m, dl, Dp, k0, k1, hi, lo); }
  ph[h + 1][dl] = hi2; pl[h + 1][dl] = lo2;          // quarters 2 and 3 -> slots 1 and 2
  if (h == 1) { ph[0][dl] = hi; pl[0][dl] = lo; }    // quarter 1 -> slot 0
  __syncthreads();
  if (h == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) residual_add(hi, lo, ph[j][dl], pl[j][dl]);
    R[(long)m * Dp + dl] = (C[(long)m * Dp + dl] - hi) - lo;
  }
  __syncthreads();
}

// C = A B with the products error-free (FMA) and the sums carried in double-double (two-sum), rounded to double once at the end.
// A [rows][K] row-major with the wave's RB rows wave-uniform (scalar loads), B [K][cols] row-major (lane = column: coalesced), both float64.
// Used for G = K_mm^-1 Psi2, the one product of the global step whose float64 ACCUMULATION carries the whole remaining error of grad_Z at the
// benchmark's conditioning: K_mm^-1 has entries of both signs around 1e5, Psi2 entries around N, and the product is (K_mm^-1 A - I) / beta -- a
// small difference.  With this one product accumulated in double-double (inputs and output float64, everything else as before) grad_Z's
// distance from the 80-bit truth drops from 1.1e-5 to 1.6e-8 at N = 1e5 and stays at 1e-8 .. 2e-8 for every data / inducing-point draw tried
// (the same arithmetic emulated with numpy error-free transformations before it was built).  No extended-precision inverse,
// no Newton step, no double-double storage is needed.  1024 waves at M = 512 with RB = 4; the four waves of a workgroup share their column
// block, so B's rows are read from L2 once per workgroup.
// SUB: the residual of the refinement step, C = (Csub - hi) - lo (solve_residual_kernel's rounding), instead of C = hi + lo.
template <int RB, int KU, bool SUB = false>
__device__ __forceinline__ void ddacc_block(const double* __restrict__ A, long lda, const double* __restrict__ B, long ldb, int K,
                                            double* __restrict__ C, long ldc, int vbx, int vby, const double* __restrict__ Csub = nullptr) {
#pragma clang fp contract(off)   // hi + a b as one FMA would break the two-sum
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = vbx * 64 + lane;
  const int i0 = (vby * 4 + wave) * RB;
  double hi[RB], lo[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) { hi[r] = 0.0; lo[r] = 0.0; }
  const double* bp = B + j;
  const double* ap = A + (long)i0 * lda;
  for (int k = 0; k < K; k += KU) {
    double bv[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) bv[u] = bp[(long)(k + u) * ldb];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const double a = ap[(long)r * lda + k + u];              // wave-uniform: a scalar load
        const double pr = a * bv[u], pe = fma(a, bv[u], -pr);    // a b = pr + pe exactly
        const double t = hi[r] + pr, bb = t - hi[r];             // two-sum
        lo[r] += ((hi[r] - (t - bb)) + (pr - bb)) + pe;
        hi[r] = t;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if constexpr (SUB) C[(long)(i0 + r) * ldc + j] = (Csub[(long)(i0 + r) * ldc + j] - hi[r]) - lo[r];
    else C[(long)(i0 + r) * ldc + j] = hi[r] + lo[r];
  }
}
template <int RB, int KU>
__global__ void __launch_bounds__(256) ddacc_gemm_kernel(const double* __restrict__ A, long lda, const double* __restrict__ B, long ldb, int K,
                                                          double* __restrict__ C, long ldc) {
  ddacc_block<RB, KU>(A, lda, B, ldb, K, C, ldc, blockIdx.x, blockIdx.y);
}
// R = C - A E with the sum in double-double: the refinement residual for Mp >= 256 (solve_residual_kernel: one row per workgroup, every lane its own
// load of E per product and two extra instructions to rebuild A[m][k]; 570 us at M = 1024, D = 1000 against the 356 us of the equally large
// product above).  A is the copy build_kmm_kernel keeps, padded rows and columns included: R's padding comes out as exact zeros.
template <int RB, int KU>
__global__ void __launch_bounds__(256) ddacc_residual_kernel(const double* __restrict__ A, long lda, const double* __restrict__ E, long lde, int K,
                                                              const double* __restrict__ Csub, double* __restrict__ R) {
  ddacc_block<RB, KU, true>(A, lda, E, lde, K, R, lde, blockIdx.x, blockIdx.y, Csub);
}

// sum over the M x M (or M x D) block of x o y; one block per pair, results into out[slot]
// (DotJob, DotJobs, DOT_BLOCKS: gp_common.h -- svi.hip describes its traces the same way)
// virtual block (vbx of DOT_BLOCKS, job vby) by the calling 256-thread workgroup; red: 256 doubles of LDS
__device__ __forceinline__ void dots_block(const DotJobs& jobs, double* part, int vbx, int vby, double* red) {
  // per-block partial sums part[job][block]; scalars_kernel adds them in a fixed order, so the bound is
  // bit-identical from run to run (an atomicAdd here made the last bits of F depend on the block schedule)
  const DotJob jb = jobs.j[vby];
  double s = 0.0;
  for (int r = vbx; r < jb.rows; r += DOT_BLOCKS)
    for (int c = threadIdx.x; c < jb.cols; c += 256) s += jb.x[(long)r * jb.ld + c] * jb.y[(long)r * jb.ld + c];
  const double tot = block_sum<256>(red, s);
  if (threadIdx.x == 0) part[vby * DOT_BLOCKS + vbx] = tot;
  __syncthreads();
}
__global__ void __launch_bounds__(256) dots_kernel(DotJobs jobs, double* part) {
  // grid (DOT_BLOCKS, jobs)
  __shared__ double red[256];
  dots_block(jobs, part, blockIdx.x, blockIdx.y, red);
}

// Bbar, dF/dKmm, Abar and the phase-2 operand Bm = [2 Bbar ; Abar^T]
__device__ __forceinline__ void assemble_elem(long idx, const double* __restrict__ Ki, const double* __restrict__ P, const double* __restrict__ EEt,
                                              const double* __restrict__ KPK, const double* __restrict__ E, double beta, double Dd, int Mp, int Dp,
                                              double* __restrict__ Bbar, double* __restrict__ dFdK, double* __restrict__ Abar, double* __restrict__ Bm) {
  const long mm = (long)Mp * Mp;
  if (idx < mm) {
    const double kp = Ki[idx] - P[idx];
    const double b = 0.5 * beta * Dd * kp - 0.5 * beta * beta * beta * EEt[idx];
    Bbar[idx] = b;
    dFdK[idx] = 0.5 * Dd * kp - 0.5 * beta * Dd * KPK[idx] - 0.5 * beta * beta * EEt[idx];
    Bm[idx] = 2.0 * b;
  } else {
    const long e = idx - mm;
    const long m = e / Dp, d = e - m * Dp;
    const double a = beta * beta * E[e];
    Abar[e] = a;
    Bm[mm + d * Mp + m] = a;
  }
}
__global__ void __launch_bounds__(256) assemble_kernel(const double* __restrict__ Ki, const double* __restrict__ P,
                                                        const double* __restrict__ EEt, const double* __restrict__ KPK,
                                                        const double* __restrict__ E, double beta, double Dd, int Mp, int Dp,
                                                        double* __restrict__ Bbar, double* __restrict__ dFdK, double* __restrict__ Abar,
                                                        double* __restrict__ Bm) {
  const long mm = (long)Mp * Mp, md = (long)Mp * Dp;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < mm + md; idx += (long)gridDim.x * 256L)
    assemble_elem(idx, Ki, P, EEt, KPK, E, beta, Dd, Mp, Dp, Bbar, dFdK, Abar, Bm);
}

// F, grad_beta, grad_sf2 from the traces (partial_terms.py:464-472, 346-358, 322-333)
__device__ __forceinline__ void scalars_block(const double* sc, double* gs, const DotJobs& jobs, const double* part, double beta, double sf2, double Dd,
                                              double Nglob) {
  if (threadIdx.x < jobs.n) {
    double s = 0.0;
    for (int b = 0; b < DOT_BLOCKS; ++b) s += part[threadIdx.x * DOT_BLOCKS + b];
    gs[jobs.j[threadIdx.x].slot] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sumYY = sc[SC_SUM_YYT], Psi0 = sc[SC_PSI0], KL = sc[SC_KL];
  const double ldK = gs[GS_LOGDET_K], ldA = gs[GS_LOGDET_A];
  const double trKi = gs[GS_TR_KIPSI2], trP = gs[GS_TR_PPSI2], trCE = gs[GS_TR_CE], trEPE = gs[GS_TR_EPSI2E];
  const double two_pi = 6.283185307179586476925286766559;
  gs[GS_F] = -0.5 * Nglob * Dd * log(two_pi) + 0.5 * Dd * Nglob * log(beta) + 0.5 * Dd * ldK - 0.5 * Dd * ldA - 0.5 * beta * sumYY -
             0.5 * beta * Dd * Psi0 + 0.5 * beta * Dd * trKi + 0.5 * beta * beta * trCE - KL;
  gs[GS_GRAD_BETA] = 0.5 * Nglob * Dd / beta - 0.5 * Dd * trP - 0.5 * sumYY - 0.5 * Dd * Psi0 + 0.5 * Dd * trKi + beta * trCE -
                     0.5 * beta * beta * trEPE;
  gs[GS_GRAD_SF2] = (gs[GS_SUM_V] + gs[GS_SUM_AC] + 2.0 * gs[GS_SUM_BPSI2] + (-0.5 * beta * Dd) * Psi0) / sf2;
}
__global__ void scalars_kernel(const double* sc, double* gs, DotJobs jobs, const double* part, double beta, double sf2, double Dd, double Nglob) {
  if (blockIdx.x != 0) return;
  scalars_block(sc, gs, jobs, part, beta, sf2, Dd, Nglob);
}

// row j by 128 threads (tid 0..127: two waves); red: 2 * QC doubles of LDS owned by these 128 threads.  `active` false: the threads only keep the
// workgroup barriers in step (the fused tail runs two rows per 256-thread workgroup, and the last pair may be half empty).  This is the form the
// one-panel tail and kmm_grads_kernel run.
constexpr int KG_QC = 8;
__device__ __forceinline__ void kmm_grads_row(int j, bool active, int tid, double* red, const double* __restrict__ dFdK, const double* __restrict__ Kmm,
                                              const double* __restrict__ Bbar, const double* __restrict__ Psi2, const double* __restrict__ Z,
                                              const double* __restrict__ alpha, int M, int Mp, int Q, int regimeA, double* __restrict__ gZ,
                                              double* __restrict__ gapart) {
  // latent dimensions in chunks of 8: the sums of a chunk stay in registers over the row, then one butterfly per sum and one
  // LDS hand-over between the two waves (the first version ran two 7-step workgroup reductions per latent dimension)
  constexpr int QC = KG_QC;
  const int lane = tid & 63, wave = tid >> 6;
  for (int q0 = 0; q0 < Q; q0 += QC) {
    double sz[QC], sa[QC], zj[QC];
#pragma unroll
    for (int u = 0; u < QC; ++u) { sz[u] = 0.0; sa[u] = 0.0; zj[u] = (active && q0 + u < Q) ? Z[(long)j * Q + q0 + u] : 0.0; }
    if (active)
      for (int m = tid; m < M; m += 128) {
        const double k = Kmm[(long)j * Mp + m];
        const double fjm = dFdK[(long)j * Mp + m];
        const double sym = (fjm + dFdK[(long)m * Mp + j]) * k;
        double w = -0.5 * fjm * k;
        if (!regimeA) w += -0.25 * Bbar[(long)j * Mp + m] * Psi2[(long)j * Mp + m];
#pragma unroll
        for (int u = 0; u < QC; ++u) {
          const double dz = zj[u] - ((q0 + u < Q) ? Z[(long)m * Q + q0 + u] : 0.0);
          sz[u] = fma(sym, dz, sz[u]);
          sa[u] = fma(w * dz, dz, sa[u]);
        }
      }
#pragma unroll
    for (int u = 0; u < QC; ++u)
      for (int sh = 32; sh > 0; sh >>= 1) { sz[u] += __shfl_xor(sz[u], sh); sa[u] += __shfl_xor(sa[u], sh); }
    if (wave == 1 && lane == 0) {
#pragma unroll
      for (int u = 0; u < QC; ++u) { red[u] = sz[u]; red[QC + u] = sa[u]; }
    }
    __syncthreads();
    if (active && wave == 0 && lane == 0) {
#pragma unroll
      for (int u = 0; u < QC; ++u)
        if (q0 + u < Q) {
          gZ[(long)j * Q + q0 + u] = -alpha[q0 + u] * (sz[u] + red[u]);
          gapart[(long)j * Q + q0 + u] = sa[u] + red[QC + u];
        }
    }
    __syncthreads();
  }
}
// Kmm-dependent parts: gK[j*Q+k] = -alpha_k sum_m' (dFdK+dFdK^T)[j,m'] Kmm[j,m'] (z_jk - z_m'k)
//                      gK[M*Q+q] = sum_mm' (-1/2 dFdK o Kmm [- 1/4 Bbar o Psi2 if !regimeA]) (z_mq - z_m'q)^2
// one block per row j; alpha parts are accumulated per block into gKpart[j][Q] and summed by the caller's reduce
__global__ void __launch_bounds__(128) kmm_grads_kernel(const double* __restrict__ dFdK, const double* __restrict__ Kmm,
                                                         const double* __restrict__ Bbar, const double* __restrict__ Psi2,
                                                         const double* __restrict__ Z, const double* __restrict__ alpha, int M, int Mp,
                                                         int Q, int regimeA, double* __restrict__ gZ, double* __restrict__ gapart) {
  __shared__ double red[2 * KG_QC];
  kmm_grads_row(blockIdx.x, true, threadIdx.x, red, dFdK, Kmm, Bbar, Psi2, Z, alpha, M, Mp, Q, regimeA, gZ, gapart);
}
// The same row with the q-independent weights computed once (they wait in LDS: [t][tid] and [nm + t][tid], every thread reads back only what it wrote), the
// inducing points read from the transposed copy Zt [Q][Mp] (lanes = consecutive inducing points: one 512-byte run per load instead of 64 cache lines), and
// four inducing points per trip with clamped addresses and zero weights past M (fma(0, dz, s) = s exactly), so a trip's loads are in flight together.
// Same sums in the same order as kmm_grads_row: same bits.  Same-box A/B against the plain form at M = 1024, Q = 50: see run_global_step.
__global__ void __launch_bounds__(128) kmm_grads_lds_kernel(const double* __restrict__ dFdK, const double* __restrict__ Kmm,
                                                             const double* __restrict__ Bbar, const double* __restrict__ Psi2,
                                                             const double* __restrict__ Z, const double* __restrict__ Zt, const double* __restrict__ alpha,
                                                             int M, int Mp, int Q, int regimeA, double* __restrict__ gZ, double* __restrict__ gapart) {
  constexpr int QC = KG_QC;
  __shared__ double red[2 * KG_QC];
  extern __shared__ __attribute__((aligned(16))) double symw[];      // 2 * 128 * ceil(M / 128) doubles
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nm = (M + 127) / 128;
  for (int t0 = 0; t0 < nm; t0 += 4) {
    double k[4], fjm[4], fmj[4], bb[4], pp[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int m = min(tid + 128 * (t0 + tt), M - 1);
      k[tt] = Kmm[(long)j * Mp + m];
      fjm[tt] = dFdK[(long)j * Mp + m];
      fmj[tt] = dFdK[(long)m * Mp + j];
      if (!regimeA) { bb[tt] = Bbar[(long)j * Mp + m]; pp[tt] = Psi2[(long)j * Mp + m]; }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int t = t0 + tt;
      if (t < nm) {
        const bool ok = tid + 128 * t < M;
        const double sym = (fjm[tt] + fmj[tt]) * k[tt];
        double w = -0.5 * fjm[tt] * k[tt];
        if (!regimeA) w += -0.25 * bb[tt] * pp[tt];
        symw[t * 128 + tid] = ok ? sym : 0.0; symw[(nm + t) * 128 + tid] = ok ? w : 0.0;
      }
    }
  }
  for (int q0 = 0; q0 < Q; q0 += QC) {
    double sz[QC], sa[QC], zj[QC];
#pragma unroll
    for (int u = 0; u < QC; ++u) { sz[u] = 0.0; sa[u] = 0.0; zj[u] = (q0 + u < Q) ? Z[(long)j * Q + q0 + u] : 0.0; }
    for (int t0 = 0; t0 < nm; t0 += 4) {
      double zz[4][QC], sy[4], ww[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int t = t0 + tt, tc = t < nm ? t : nm - 1;
        const int m = min(tid + 128 * tc, M - 1);
        sy[tt] = t < nm ? symw[tc * 128 + tid] : 0.0;
        ww[tt] = t < nm ? symw[(nm + tc) * 128 + tid] : 0.0;
#pragma unroll
        for (int u = 0; u < QC; ++u) zz[tt][u] = (q0 + u < Q) ? Zt[(long)(q0 + u) * Mp + m] : 0.0;
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int u = 0; u < QC; ++u) {
          const double dz = zj[u] - zz[tt][u];
          sz[u] = fma(sy[tt], dz, sz[u]);
          sa[u] = fma(ww[tt] * dz, dz, sa[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < QC; ++u)
      for (int sh = 32; sh > 0; sh >>= 1) { sz[u] += __shfl_xor(sz[u], sh); sa[u] += __shfl_xor(sa[u], sh); }
    if (wave == 1 && lane == 0) {
#pragma unroll
      for (int u = 0; u < QC; ++u) { red[u] = sz[u]; red[QC + u] = sa[u]; }
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
#pragma unroll
      for (int u = 0; u < QC; ++u)
        if (q0 + u < Q) {
          gZ[(long)j * Q + q0 + u] = -alpha[q0 + u] * (sz[u] + red[u]);
          gapart[(long)j * Q + q0 + u] = sa[u] + red[QC + u];
        }
    }
    __syncthreads();
  }
}
// column q of part [rows][Q] summed by the calling 256-thread workgroup; red: 256 doubles of LDS
__device__ __forceinline__ void colsum_block(const double* __restrict__ part, int rows, int Q, double* __restrict__ out, int q, double* red) {
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += part[(long)r * Q + q];
  const double tot = block_sum<256>(red, s);
  if (threadIdx.x == 0) out[q] = tot;
  __syncthreads();
}
__global__ void __launch_bounds__(256) colsum_kernel(const double* __restrict__ part, int rows, int Q, double* __restrict__ out) {
  __shared__ double red[256];
  colsum_block(part, rows, Q, out, blockIdx.x, red);
}

// ---------------------------------------------------------------------------------------------- the step's operands and products, named once
// The global step's buffers (gs_view builds it from the context).  Both forms of the schedule -- run_global_step's launches and tail_stage_kernel's
// stages -- take their operands, their products and their trace jobs from here.
struct GsView {
  double *Ki, *P;                                     // GsState::Inv: [Kmm^-1 ; (Kmm + beta Psi2)^-1]
  const double *Psi2, *C, *sc;                        // the all-reduced statistics
  double *KmmKeep, *E, *PsiE, *T1, *T2, *dFdK, *Bbar, *Abar, *Bm, *gs, *gK;
  const double *Z, *Zt, *alpha;
};
static GsView gs_view(gp_ctx* c) {
  const long mm = (long)c->Mp * c->Mp;
  GsState& g = c->gstep;
  return {g.Inv, g.Inv + mm, c->stats, c->stats + mm, c->stats + mm + (long)c->Mp * c->Dp,
          g.KmmKeep, g.E, g.PsiE, g.T1, g.T2, g.dFdK, g.Bbar, g.Abar, g.Bm, g.gs, g.gK, c->Z, c->Zt, c->alpha};
}
// the seven traces of the bound and its partials
static DotJobs gs_dot_jobs(const GsView& v, int M, int D, int Mp, int Dp) {
  return {{{v.Ki, v.Psi2, Mp, M, M, GS_TR_KIPSI2},
           {v.P, v.Psi2, Mp, M, M, GS_TR_PPSI2},
           {v.C, v.E, Dp, M, D, GS_TR_CE},
           {v.E, v.PsiE, Dp, M, D, GS_TR_EPSI2E},
           {v.dFdK, v.KmmKeep, Mp, M, M, GS_SUM_V},
           {v.Abar, v.C, Dp, M, D, GS_SUM_AC},
           {v.Bbar, v.Psi2, Mp, M, M, GS_SUM_BPSI2}},
          7};
}
// The six products (five descriptions: E += P R is E_is_P_C's second form), each with its layouts (LA, LB: launch_gemm's la / lb, gemm32_tile's template arguments) and its operands.  The host path adds its
// big / split choice (gemm_plan), the tail its tile indices.  Mp, Dp are arguments so that the tail's stay compile-time constants.
struct E_is_P_C {          // E = P C, and the refinement's E += P R (the same product with beta = 1 and the residual R, held in PsiE, for C).  P [m][k] -> K_CONTIG, C / R stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static __host__ __device__ GemmP with(const GsView& v, int Mp, int Dp, const double* C, double beta) { return gemm_of({v.P, Mp}, {C, Dp}, {v.E, Dp}, Mp, 1.0, beta); }
  static __host__ __device__ GemmP of(const GsView& v, int Mp, int Dp) { return with(v, Mp, Dp, v.C, 0.0); }
  static __host__ __device__ GemmP plus_P_R(const GsView& v, int Mp, int Dp) { return with(v, Mp, Dp, v.PsiE, 1.0); }
};
struct T2_is_Ki_Psi2 {     // the float64 form of G = Kmm^-1 Psi2 (dd_kipsi2 = 0).  Ki [m][k] -> K_CONTIG, Psi2 stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static __host__ __device__ GemmP of(const GsView& v, int Mp) { return gemm_of({v.Ki, Mp}, {v.Psi2, Mp}, {v.T2, Mp}, Mp); }
};
struct dFdK_is_T2_Ki {     // Kmm^-1 Psi2 Kmm^-1, into dFdK until the assembly.  T2 [m][k] -> K_CONTIG, Ki stored [k][c] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static __host__ __device__ GemmP of(const GsView& v, int Mp) { return gemm_of({v.T2, Mp}, {v.Ki, Mp}, {v.dFdK, Mp}, Mp); }
};
struct PsiE_is_Psi2_E {    // Psi2 [m][k] -> K_CONTIG, E stored [k][d] -> FREE_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = FREE_CONTIG;
  static __host__ __device__ GemmP of(const GsView& v, int Mp, int Dp) { return gemm_of({v.Psi2, Mp}, {v.E, Dp}, {v.PsiE, Dp}, Mp); }
};
struct T1_is_E_Et {        // E [m][k] -> K_CONTIG; B(k,j) = E[j][k] -> K_CONTIG
  static constexpr Layout LA = K_CONTIG, LB = K_CONTIG;
  static __host__ __device__ GemmP of(const GsView& v, int Mp, int Dp) { return gemm_of({v.E, Dp}, {v.E, Dp}, {v.T1, Mp}, Dp); }
};

// ---------------------------------------------------------------------------------------------- short tail for one-panel problems
// M <= 128 and D <= 128 (BASELINE configs[1]: M = 128, D = 10): everything of the global step behind the panel factorisation -- the two inverses,
// E with its refinement step, Psi2 E, E E^T, K_mm^-1 Psi2 in double-double, its product with K_mm^-1, the assembled partials, the seven traces, the
// scalars and the K_mm parts of the gradients -- used to be FIFTEEN launches of 4-12 us each, every one of them at the launch floor
// (profiles/r05_config1_timeline.txt: 80 us for 2e7 flop).  Products that do not depend on each other now share a launch: SEVEN launches of one
// kernel (tail_stage_kernel, stage = 0..6), every workgroup taking one work item of its stage -- the same 32 x 32 tile products, double-double
// blocks, dot-product blocks and rows as the separate kernels (the device functions above are shared, so the results are bit-identical).
//   0: [Ki ; P] = X^T X (32 tiles)                         1: E = P C (16 tiles) | T2 = Ki Psi2 in double-double (64 blocks)
//   2: R = C - A E in double-double (128 rows) | T2 Ki (16 tiles)                    3: E += P R (16 tiles)
//   4: Psi2 E (16 tiles, then Abar and Bm's lower block for the tile) | E E^T (16 tiles, then Bbar, dF/dKmm, Bm's upper block for the tile)
//   5: the seven traces (7 x 64 blocks) | K_mm parts of grad_Z / grad_alpha (two rows per workgroup)        6: scalars | column sums
// Why launches and not one persistent kernel with grid barriers: that was built first (r05) and measured at 94 us against 80 for the fifteen
// launches -- on this part an agent-scope release + acquire (L2 write-back, L1 / L2 invalidate on eight XCDs) costs as much as a kernel boundary,
// which does the same thing in hardware (MI355X_MICROARCH.md, inter-workgroup visibility: 1.7 + 1.7 us of fences + the counter round trips).
constexpr int TAIL_STAGES = 7;
constexpr int TAIL_LDS_DOUBLES = 2 * SmallImg<FREE_CONTIG>::DOUBLES;     // the larger operand image, twice (12288 doubles = 96 KB)
struct TailP {
  GsView v;
  const double* Linv;                                 // [2][128][128]
  DotJobs jobs;
  double beta, sf2, Dd, Nglob, jitA;
  int M, Q, regimeA, refine, dd;
};
__host__ __device__ inline int tail_items(int stage, int M, int Q, int refine, int dd) {
  switch (stage) {
    case 0: return 32;
    case 1: return 16 + (dd ? 64 : 16);
    case 2: return 16 + (refine ? 128 : 0);
    case 3: return refine ? 16 : 0;
    case 4: return 32;
    case 5: return 7 * DOT_BLOCKS + (M + 1) / 2;
    default: return 1 + Q;
  }
}
__global__ void __launch_bounds__(256, 1) tail_stage_kernel(TailP p, int stage) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* sA = sm;
  double* sB = sm + SmallImg<FREE_CONTIG>::DOUBLES;
  double* red = sm;                                     // the items without tile products reuse the front of the images
  constexpr int Mp = 128, Dp = 128;
  constexpr long mm = (long)Mp * Mp;
  const int t = blockIdx.x;
  const GsView& v = p.v;
  if (stage == 0) {
    gemm32_tile<FREE_CONTIG, FREE_CONTIG>(gemm_of({p.Linv, Mp, mm}, {p.Linv, Mp, mm}, {v.Ki, Mp, mm}, Mp), t & 3, (t >> 2) & 3, t >> 4, sA, sB);
  } else if (stage == 1) {
    if (t < 16) {
      gemm32_tile<E_is_P_C::LA, E_is_P_C::LB>(E_is_P_C::of(v, Mp, Dp), t & 3, t >> 2, 0, sA, sB);
    } else if (p.dd) {
      // one row per wave: the rows are independent, so the bits are those of the two-rows-per-wave form; 4 us faster at M = 128 (profiles/r04_dd_variants.txt)
      ddacc_block<1, 8>(v.Ki, (long)Mp, v.Psi2, (long)Mp, Mp, v.T2, (long)Mp, (t - 16) & 1, (t - 16) >> 1);
    } else {
      gemm32_tile<T2_is_Ki_Psi2::LA, T2_is_Ki_Psi2::LB>(T2_is_Ki_Psi2::of(v, Mp), (t - 16) & 3, (t - 16) >> 2, 0, sA, sB);
    }
  } else if (stage == 2) {
    if (t < 16) {
      gemm32_tile<dFdK_is_T2_Ki::LA, dFdK_is_T2_Ki::LB>(dFdK_is_T2_Ki::of(v, Mp), t & 3, t >> 2, 0, sA, sB);
    } else {
      const int m = t - 16;
      double (*ph)[128] = reinterpret_cast<double (*)[128]>(red);
      double (*pl)[128] = reinterpret_cast<double (*)[128]>(red + 3 * 128);
      if (m < p.M) residual_row256(m, v.KmmKeep, v.Psi2, p.beta, p.jitA, v.C, v.E, p.M, Mp, Dp, v.PsiE, ph, pl);
      else if (threadIdx.x < Dp) v.PsiE[(long)m * Dp + threadIdx.x] = 0.0;
    }
  } else if (stage == 3) {
    gemm32_tile<E_is_P_C::LA, E_is_P_C::LB>(E_is_P_C::plus_P_R(v, Mp, Dp), t & 3, t >> 2, 0, sA, sB);
  } else if (stage == 4) {
    // the tile product, then the assembled outputs that need nothing but this tile and finished inputs: every element of the assembly is
    // computed once, by the expression of assemble_elem
    const int tt = t & 15, bx = tt & 3, by = tt >> 2;
    if (t < 16) {
      gemm32_tile<PsiE_is_Psi2_E::LA, PsiE_is_Psi2_E::LB>(PsiE_is_Psi2_E::of(v, Mp, Dp), bx, by, 0, sA, sB);
      for (int e = threadIdx.x; e < ST * ST; e += 256)      // Abar and Bm's lower block: only E (finished in stage 3)
        assemble_elem(mm + (long)(by * ST + (e >> 5)) * Dp + bx * ST + (e & 31), v.Ki, v.P, v.T1, v.dFdK, v.E, p.beta, p.Dd, Mp, Dp, v.Bbar, v.dFdK, v.Abar, v.Bm);
    } else {
      gemm32_tile<T1_is_E_Et::LA, T1_is_E_Et::LB>(T1_is_E_Et::of(v, Mp, Dp), bx, by, 0, sA, sB);
      __syncthreads();                                      // the tile of E E^T this workgroup just stored (same CU: visible after the barrier)
      for (int e = threadIdx.x; e < ST * ST; e += 256)
        assemble_elem((long)(by * ST + (e >> 5)) * Mp + bx * ST + (e & 31), v.Ki, v.P, v.T1, v.dFdK, v.E, p.beta, p.Dd, Mp, Dp, v.Bbar, v.dFdK, v.Abar, v.Bm);
    }
  } else if (stage == 5) {
    const int nd = p.jobs.n * DOT_BLOCKS;
    if (t < nd) dots_block(p.jobs, v.gs + GS_COUNT + 8, t % DOT_BLOCKS, t / DOT_BLOCKS, red);
    else {
      const int half = threadIdx.x >> 7, j = 2 * (t - nd) + half;
      kmm_grads_row(j, j < p.M, threadIdx.x & 127, red + 2 * KG_QC * half, v.dFdK, v.KmmKeep, v.Bbar, v.Psi2, v.Z, v.alpha, p.M, Mp, p.Q, p.regimeA,
                    v.gK, v.T2);
    }
  } else {
    if (t == 0) scalars_block(v.sc, v.gs, p.jobs, v.gs + GS_COUNT + 8, p.beta, p.sf2, p.Dd, p.Nglob);
    else colsum_block(v.T2, p.M, p.Q, v.gK + (long)p.M * p.Q, t - 1, red);
  }
}
std::atomic<int> g_opt_gs_tail{env_flag("GPARML_GS_TAIL", true)};

// Host side of the global step's outcome: one D2H of the scalars + failure flags, at the first call that needs them
// (gp_global_status, gp_finish, gp_download).  Returns GP_OK, GP_ERR_NOT_PD, GP_ERR_NON_FINITE or GP_RETRY_JITTER.
int check_global(gp_ctx* c) {
  if (c->life.step_outcome_pending()) {
    double h[GS_HOST];
    GP_HIP(c, hipMemcpyAsync(h, c->gstep.gs, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    GP_HIP(c, hipStreamSynchronize(c->stream));
    ++c->sync_epoch;
    return check_global_from(c, h);
  }
  return check_global_from(c, nullptr);
}

int check_global_from(gp_ctx* c, const double* h) {
  if (c->life.step_outcome_pending() && h) {
    for (int i = 0; i < GS_COUNT; ++i) c->gstep.h_gs[i] = h[i];
    c->life.step_read_back();
    const int failed = (h[GS_FLAGS] != 0.0 ? 1 : 0) | (h[GS_FLAGS + 1] != 0.0 ? 2 : 0);
    const bool singular = h[GS_FLAGS] == 2.0 || h[GS_FLAGS + 1] == 2.0;
    if (singular) {
      // an exactly zero pivot: the reference fails in linalg.inv before any jitter applies (partial_terms.py:60, 95)
      c->gstep.gs_status = GP_ERR_NOT_PD;
      c->gstep.gs_msg = std::string(h[GS_FLAGS] == 2.0 ? "Kmm" : c->gstep.svi_step ? "Lambda_v" : "Kmm + beta*Psi2") + " is singular (numpy.linalg.inv: Singular matrix)";
    } else if (c->gstep.svi_step && (failed & 2)) {
      // gp_svi_step: the second flag is Lambda_v's, the caller's state -- no jitter is added to it
      c->gstep.gs_status = GP_ERR_NOT_PD;
      c->gstep.gs_msg = "Lambda_v is not positive definite (gp_svi_set / gp_svi_natural_step left it so)";
    } else if (failed & ~c->gstep.jitter_mask) {
      // first failure of this matrix: the reference continues with 1e-7 * I added (partial_terms.py:452-456)
      c->gstep.retry_mask = c->gstep.jitter_mask | failed;
      c->gstep.gs_status = GP_RETRY_JITTER;
      c->gstep.gs_msg = std::string(failed & 1 ? "Kmm" : "Kmm + beta*Psi2") + " is not positive definite (Cholesky failed); retry with 1e-7 jitter";
    } else if (failed) {
      c->gstep.gs_status = GP_ERR_NOT_PD;
      c->gstep.gs_msg = std::string(failed & 1 ? "Kmm" : "Kmm + beta*Psi2") + " is not positive definite even with 1e-7 jitter (partial_terms.py:459-461 assertion)";
    } else if (!std::isfinite(h[GS_F])) {
      c->gstep.gs_status = GP_ERR_NON_FINITE;
      c->gstep.gs_msg = "bound is not finite";
    } else {
      c->gstep.gs_status = GP_OK;
    }
  }
  if (c->gstep.gs_status != GP_OK) return fail(c, c->gstep.gs_status, "%s", c->gstep.gs_msg.c_str());
  return GP_OK;
}

int GsState::alloc(gp_ctx* c) {
  const long Mp = c->Mp, Dp = c->Dp;
  int rc = GP_OK;
  auto A = [&](auto& b, size_t n, int mode = DA_INIT) { if (rc == GP_OK) rc = b.alloc(c, n, mode); };
  A(Kmm, (size_t)2 * Mp * Mp); A(Lmat, (size_t)2 * Mp * Mp); A(Inv, (size_t)2 * Mp * Mp);
  A(Linv, (size_t)2 * Mp * Mp, DA_ZERO);   // zero contract: the 128-blocks above the block diagonal are never written (potrf_inverse_batched's precondition)
  if (Mp >= 512 && Mp <= 2048) {
    // gsi8.hip: ten digit planes of W = [A | B] for the larger of the two products (K_mm^-1 | Psi2: 2 Mp columns; K_mm + beta Psi2 | E: Mp + Dp), and W's column scales
    const size_t wcols = (size_t)Mp + std::max(Mp, Dp);
    A(gsd, (size_t)10 * Mp * wcols);
    A(gss, wcols);
  }
  A(KmmKeep, (size_t)Mp * Mp); A(T1, (size_t)Mp * std::max<long>(std::max(Mp, Dp), 256)); A(T2, (size_t)Mp * std::max(Mp, Dp));
  A(dFdK, (size_t)Mp * Mp); A(Bbar, (size_t)Mp * Mp);
  A(E, (size_t)Mp * Dp); A(PsiE, (size_t)Mp * Dp); A(Abar, (size_t)Mp * Dp);
  A(Bm, (size_t)c->LDK * Mp);
  A(gs, (size_t)GS_TOTAL);
  A(gK, (size_t)c->M * c->Q + c->Q);
  return rc;
}
// (not Linv: its upper blocks are a zero contract)
int GsState::poison(gp_ctx* c) {
  for (const DevBuf<double>* b : {&Kmm, &Lmat, &Inv, &KmmKeep, &T1, &T2, &dFdK, &Bbar, &E, &PsiE, &Abar, &Bm, &gK, &gs}) GP_HIP(c, poison_fill(c, *b));
  return GP_OK;
}

// ---------------------------------------------------------------------------------------------- the two extended-precision products, dispatched once
// G = K_mm^-1 Psi2 and the refinement residual R = C - (K_mm + beta Psi2) E exist in four device forms; the step chooses here and nowhere else, and
// gp_debug_dd_product (below) runs either function on operands of its own, in the step's choice or a forced one (tests/test_gpu_dd_products.py).
enum { DD_FORM_GEMM = 1, DD_FORM_RESIDUAL = 2, DD_FORM_ROW = 3, DD_FORM_I8 = 4 };
// out [nA][nB] = sum_k A(i, k) B[k][j], or Csub - that sum.  The double-double kernels read A as [nA][K]; the int8 product reads it as [K][nA] (the
// step's A is symmetric in both uses).  B [K][nB], out and Csub [nA][nB]; the double-double residual takes out's and Csub's row stride from ldb.
struct DdProduct { const double* A; long lda; int nA; const double* B; long ldb; int nB; int K; double* out; long ldo; const double* Csub; };
// what only the row form reads: it rebuilds A = fma(beta, Psi2, Keep) + jitA I on the leading M x M block ([Mp][Mp] each, Mp = the product's nA)
struct RowOperands { const double* Keep; const double* Psi2; double beta, jitA; int M; };
static int G_form(bool gi8) { return gi8 ? DD_FORM_I8 : DD_FORM_GEMM; }
// narrow E: too few waves for ddacc_block (M = 512, D = 100: +21 us)
static int residual_form(bool gi8, int Mp, int Dp) { return gi8 ? DD_FORM_I8 : (g_opt_residual_dd.load() && Mp >= 256 && Dp >= 512) ? DD_FORM_RESIDUAL : DD_FORM_ROW; }
static int form_G(gp_ctx* c, hipStream_t st, int form, const DdProduct& p) {
  if (form == DD_FORM_I8) return run_gs_i8_product(c, st, p.A, p.lda, p.nA, p.B, p.ldb, p.nB, p.K, p.out, p.ldo, nullptr);
  GP_LAUNCH(c, st, (ddacc_gemm_kernel<2, 8>), dim3(p.nB / 64, p.nA / 8), dim3(256), 0, p.A, p.lda, p.B, p.ldb, p.K, p.out, p.ldo);
  return GP_OK;
}
static int form_residual(gp_ctx* c, hipStream_t st, int form, const DdProduct& p, const RowOperands& r) {
  if (form == DD_FORM_I8) return run_gs_i8_product(c, st, p.A, p.lda, p.nA, p.B, p.ldb, p.nB, p.K, p.out, p.ldo, p.Csub);
  if (form == DD_FORM_RESIDUAL) {
    GP_LAUNCH(c, st, (ddacc_residual_kernel<2, 8>), dim3(p.nB / 64, p.nA / 8), dim3(256), 0, p.A, p.lda, p.B, p.ldb, p.K, p.Csub, p.out);
    return GP_OK;
  }
  const int Mp = p.nA, Dp = p.nB;
  GP_LAUNCH(c, st, solve_residual_kernel, dim3(r.M), dim3(512), 0, r.Keep, r.Psi2, r.beta, r.jitA, p.Csub, p.B, r.M, Mp, Dp, p.out, 0);
  if (r.M < Mp) GP_HIP(c, hipMemsetAsync(p.out + (long)r.M * Dp, 0, (size_t)(Mp - r.M) * Dp * sizeof(double), st));
  return GP_OK;
}

// Kmm parts of grad_Z / grad_alpha from dFdK, Bbar, KmmKeep and Psi2 as they stand; alpha partials per row go through T2 (free again)
int launch_kmm_grads(gp_ctx* c, hipStream_t st) {
  const int Mp = c->Mp, M = c->M, Q = c->Q;
  const GsView v = gs_view(c);
  static const bool kmm_lds = env_flag("GPARML_KMM_LDS", true);
  if (kmm_lds && M <= 2048)
    GP_LAUNCH(c, st, kmm_grads_lds_kernel, dim3(M), dim3(128), (size_t)2 * 128 * ((M + 127) / 128) * sizeof(double), v.dFdK, v.KmmKeep, v.Bbar, v.Psi2, v.Z,
              v.Zt, v.alpha, M, Mp, Q, c->regime_A ? 1 : 0, v.gK, v.T2);
  else
    GP_LAUNCH(c, st, kmm_grads_kernel, dim3(M), dim3(128), 0, v.dFdK, v.KmmKeep, v.Bbar, v.Psi2, v.Z, v.alpha, M, Mp, Q, c->regime_A ? 1 : 0, v.gK, v.T2);
  GP_LAUNCH(c, st, colsum_kernel, dim3(Q), dim3(256), 0, v.T2, M, Q, v.gK + (long)M * Q);
  return GP_OK;
}
int launch_build_kmm(gp_ctx* c, hipStream_t st, double* Kmm, double* A, double jitK, double jitA, double* gs_zero, double* Acopy) {
  GP_LAUNCH(c, st, build_kmm_kernel, dim3(c->Mp / 64, c->Mp / 16), dim3(256), 0, c->Z, c->alpha, c->sf2, c->beta, c->stats.get(), c->M, c->Mp, c->Q, Kmm, A,
            c->gstep.KmmKeep.get(), jitK, jitA, gs_zero, Acopy);
  return GP_OK;
}
int launch_dots(gp_ctx* c, hipStream_t st, const DotJobs& jobs, double* part) {
  GP_LAUNCH(c, st, dots_kernel, dim3(DOT_BLOCKS, jobs.n), dim3(256), 0, jobs, part);
  return GP_OK;
}

int run_global_step(gp_ctx* c) {
  hipStream_t st = c->stream;
  const int Mp = c->Mp, Dp = c->Dp, M = c->M, D = c->D, Q = c->Q;
  const long mm = (long)Mp * Mp;
  const GsView v = gs_view(c);
  const DotJobs jobs = gs_dot_jobs(v, M, D, Mp, Dp);
  const double jitA = (c->gstep.jitter_mask & 2) ? 1e-7 : 0.0;
  c->gstep.gs_status = GP_OK;
  double* failf = v.gs + GS_FLAGS;  // [2]
  // T2 is free until G = K_mm^-1 Psi2 is formed: it keeps A for the double-double residual of the refinement step
  const bool gi8 = gs_i8_wanted(c);            // gsi8.hip: both double-double products on the int8 matrix core (M >= 1024)
  const int res_form = residual_form(gi8, Mp, Dp);
  const bool res_dd = g_opt_refine_E.load() && res_form != DD_FORM_ROW;     // the forms that read A's copy
  GP_TRY_RC(launch_build_kmm(c, st, c->gstep.Kmm, c->gstep.Kmm + mm, (c->gstep.jitter_mask & 1) ? 1e-7 : 0.0, jitA, v.gs, res_dd ? v.T2 : (double*)nullptr));
  // one-panel problems (M, D <= 128): the panel kernel, then seven launches of tail_stage_kernel instead of fifteen kernels
  if (Mp == NB && Dp == NB && g_opt_gs_tail.load()) {
    GP_HIP(c, hipFuncSetAttribute((const void*)potrf_trinv128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, POTRF_LDS_DOUBLES * 8));
    GP_HIP(c, hipFuncSetAttribute((const void*)tail_stage_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TAIL_LDS_DOUBLES * 8));
    GP_LAUNCH(c, st, potrf_trinv128_kernel, dim3(2), dim3(512), POTRF_LDS_DOUBLES * 8, c->gstep.Kmm, (long)Mp, mm, 0, c->gstep.Linv, failf, v.gs + GS_LOGDET_K);
    const TailP t = {v, c->gstep.Linv, jobs, c->beta, c->sf2, (double)D, (double)c->N_global, jitA, M, Q, c->regime_A ? 1 : 0, g_opt_refine_E.load(), g_opt_dd_kipsi2.load()};
    for (int stage = 0; stage < TAIL_STAGES; ++stage) {
      const int items = tail_items(stage, M, Q, t.refine, t.dd);
      // only the stages with tile products need the operand images
      const size_t lds = (stage <= 4) ? (size_t)TAIL_LDS_DOUBLES * 8 : 4096;
      if (items > 0) GP_LAUNCH(c, st, tail_stage_kernel, dim3(items), dim3(256), lds, t, stage);
    }
    return GP_OK;
  }
  // factorise [Kmm ; A] in place, invert.  T1 is the 2 x 128 x Mp work panel.
  // split-k workspace: the shared workspace is free during the global step (>= 600 tiles); the split factors follow its shape-derived capacity
  double* ws = nullptr;
  const size_t wcap = c->ws.capacity;
  GP_TRY_RC(c->ws.take(c, wcap, "global step", &ws));
  int rc = potrf_inverse_batched(c, st, Mp, 2, c->gstep.Kmm, c->gstep.Linv, c->gstep.Inv, v.T1, v.gs + GS_LOGDET_K, failf, ws, wcap);
  if (rc != GP_OK) return rc;
  // E = P C ; PsiE = Psi2 E ; T1 = E E^T   and, independent of it,   T2 = Ki Psi2 ; dFdK(tmp) = T2 Ki.   One stream: a side stream for the second
  // chain was measured slower (r03: 0.424 -> 0.455 ms at M = 512 -- every cross-stream event edge costs more than the 5-12 us product it hides)
  // and was removed in r06.  The M x M x D and M x M x M products take gemm_plan's choice; E E^T stays on the small tiles.
  const int gb = g_opt_gemm_big.load();
  const GemmPlan md = gemm_plan((long)(Mp / TILE) * (Dp / TILE), Mp, ws ? wcap : 0, gb, Mp);
  const GemmPlan sq = gemm_plan((long)(Mp / TILE) * (Mp / TILE), Mp, ws ? wcap : 0, gb, Mp);
  GP_TRY_RC(launch_gemm(c, st, E_is_P_C::LA, E_is_P_C::LB, Mp, Dp, 1, E_is_P_C::of(v, Mp, Dp).on_big(md.big).split(md.splits, ws)));
  // one refinement step of E with a double-double residual (PsiE is free until the next product); GPARML_REFINE_E=0 turns it off
  if (g_opt_refine_E.load()) {
    GP_TRY_RC(form_residual(c, st, res_form, {v.T2, (long)Mp, Mp, v.E, (long)Dp, Dp, Mp, v.PsiE, (long)Dp, v.C}, {v.KmmKeep, v.Psi2, c->beta, jitA, M}));
    GP_TRY_RC(launch_gemm(c, st, E_is_P_C::LA, E_is_P_C::LB, Mp, Dp, 1, E_is_P_C::plus_P_R(v, Mp, Dp).on_big(md.big).split(md.splits, ws)));
  }
  GP_TRY_RC(launch_gemm(c, st, PsiE_is_Psi2_E::LA, PsiE_is_Psi2_E::LB, Mp, Dp, 1, PsiE_is_Psi2_E::of(v, Mp, Dp).on_big(md.big).split(md.splits, ws)));
  GP_TRY_RC(launch_gemm(c, st, T1_is_E_Et::LA, T1_is_E_Et::LB, Mp, Mp, 1, T1_is_E_Et::of(v, Mp, Dp)));
  // G = Ki Psi2 with double-double accumulation (ddacc_gemm_kernel above: two rows per wave, eight k per trip -- same-box timing of six shapes
  // in profiles/r04_dd_variants.txt: +50 us at M = 512, +9 us at M = 128, +0.29 ms at M = 1024 over the float64 matrix-core product of r03, which
  // GPARML_DD_KIPSI2=0 or gp_debug_set_option("dd_kipsi2", 0) restores)
  if (g_opt_dd_kipsi2.load()) {
    GP_TRY_RC(form_G(c, st, G_form(gi8), {v.Ki, (long)Mp, Mp, v.Psi2, (long)Mp, Mp, Mp, v.T2, (long)Mp, nullptr}));
  } else {
    GP_TRY_RC(launch_gemm(c, st, T2_is_Ki_Psi2::LA, T2_is_Ki_Psi2::LB, Mp, Mp, 1, T2_is_Ki_Psi2::of(v, Mp).on_big(sq.big).split(sq.splits, ws)));
  }
  GP_TRY_RC(launch_gemm(c, st, dFdK_is_T2_Ki::LA, dFdK_is_T2_Ki::LB, Mp, Mp, 1, dFdK_is_T2_Ki::of(v, Mp).on_big(sq.big).split(sq.splits, ws)));
  // dFdK currently holds Ki Psi2 Ki; assemble in place is unsafe (reads KPK, writes dFdK at the same index: fine, same thread)
  GP_LAUNCH(c, st, assemble_kernel, dim3(1024), dim3(256), 0, v.Ki, v.P, v.T1, v.dFdK, v.E, c->beta, (double)D, Mp, Dp, v.Bbar, v.dFdK, v.Abar, v.Bm);
  double* dpart = v.gs + GS_DOTS;   // [jobs][DOT_BLOCKS]
  // the traces / scalars and the Kmm parts of the gradients both start from the assembled partials and do not touch each other's outputs
  GP_TRY_RC(launch_dots(c, st, jobs, dpart));
  GP_LAUNCH(c, st, scalars_kernel, dim3(1), dim3(64), 0, v.sc, v.gs, jobs, dpart, c->beta, c->sf2, (double)D, (double)c->N_global);
  GP_TRY_RC(launch_kmm_grads(c, st));
  return GP_OK;
}

}  // namespace gp

// ---- test hooks ------------------------------------------------------------------------------------------------
// The body of both factorisation hooks: pad, upload, potrf_inverse_batched as the global step runs it, download, unpad.  Per-entry outputs and the raw
// fail mask; with_workspace: the split-k workspace that takes the X^T X product onto the 128-tile kernel for Mp >= 1024.  The workspace has the floor of
// the shared workspace's capacity (workspace_capacity, api.hip: 1100 tiles); choose_splits never asks for more than 512 partial tiles, so a larger
// capacity decides nothing differently.
static int potrf_inverse_hook(int device, int n, int batch, int with_workspace, const double* A, double* L, double* Ainv, double* logdet, int* fail_mask) {
  using namespace gp;
  gp_ctx tmp;
  gp_ctx* c = &tmp;
  GP_HIP(c, hipSetDevice(device));
  const int Mp = (int)round_up(n, NB);
  const long mm = (long)Mp * Mp, nn = (long)n * n;
  const size_t wcap = (size_t)1100 * TILE * TILE;
  std::vector<double> h((size_t)batch * mm, 0.0);
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < Mp; ++i)
      for (int k = 0; k < Mp; ++k) h[b * mm + (long)i * Mp + k] = (i < n && k < n) ? A[b * nn + (long)i * n + k] : (i == k ? 1.0 : 0.0);
  DevBuf<double> dA, dLi, dInv, dT, dS, dW;     // (allocated without the context: a failure is reported by gp_last_error(NULL))
  GP_TRY_RC(dA.alloc(nullptr, batch * mm, DA_RAW)); GP_TRY_RC(dLi.alloc(nullptr, batch * mm, DA_RAW)); GP_TRY_RC(dInv.alloc(nullptr, batch * mm, DA_RAW));
  GP_TRY_RC(dT.alloc(nullptr, batch * mm / 2, DA_RAW)); GP_TRY_RC(dS.alloc(nullptr, 2 * batch, DA_RAW));
  if (with_workspace) GP_TRY_RC(dW.alloc(nullptr, wcap, DA_RAW));
  GP_HIP(c, hipMemcpy(dA, h.data(), dA.bytes(), hipMemcpyHostToDevice));
  GP_HIP(c, hipMemset(dS, 0, dS.bytes()));
  GP_HIP(c, hipMemset(dLi, 0, dLi.bytes()));          // the zero contract of Linv's upper blocks
  // NaN bytes in everything the call must write before it reads
  GP_HIP(c, hipMemset(dInv, 0xFF, dInv.bytes()));
  GP_HIP(c, hipMemset(dT, 0xFF, dT.bytes()));
  if (with_workspace) GP_HIP(c, hipMemset(dW, 0xFF, dW.bytes()));
  int rc = potrf_inverse_batched(c, nullptr, Mp, batch, dA, dLi, dInv, dT, dS, dS + batch, with_workspace ? dW.get() : nullptr, with_workspace ? wcap : 0);
  if (rc != GP_OK) { gp::g_create_error = c->err; return rc; }
  std::vector<double> s(2 * batch);
  GP_HIP(c, hipDeviceSynchronize());
  GP_HIP(c, hipMemcpy(s.data(), dS, dS.bytes(), hipMemcpyDeviceToHost));
  int mask = 0;
  for (int b = 0; b < batch; ++b) { if (logdet) logdet[b] = s[b]; if (s[batch + b] != 0.0) mask |= 1 << b; }
  *fail_mask = mask;           // known from here on, whatever the downloads below do
  if (L) {
    GP_HIP(c, hipMemcpy(h.data(), dA, dA.bytes(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) for (int i = 0; i < n; ++i) for (int k = 0; k < n; ++k) L[b * nn + (long)i * n + k] = (k <= i) ? h[b * mm + (long)i * Mp + k] : 0.0;
  }
  if (Ainv) {
    GP_HIP(c, hipMemcpy(h.data(), dInv, dInv.bytes(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) for (int i = 0; i < n; ++i) for (int k = 0; k < n; ++k) Ainv[b * nn + (long)i * n + k] = h[b * mm + (long)i * Mp + k];
  }
  return GP_OK;
}

extern "C" int gp_debug_potrf_inverse(int device, int n, const double* A, double* L, double* Ainv, double* logdet) {
  using namespace gp;
  if (n <= 0 || !A) return fail(nullptr, GP_ERR_BAD_ARG, "gp_debug_potrf_inverse: bad argument");
  int mask = 0;
  GP_TRY_RC(potrf_inverse_hook(device, n, 1, 0, A, L, Ainv, logdet, &mask));
  if (mask) return fail(nullptr, GP_ERR_NOT_PD, "matrix is not positive definite");
  return GP_OK;
}

// gp_debug_potrf_inverse for a batch
extern "C" int gp_debug_potrf_inverse_batched(int device, int n, int batch, int with_workspace, const double* A, double* L, double* Ainv, double* logdet,
                                              int* fail_mask) {
  using namespace gp;
  if (n <= 0 || batch < 1 || batch > 8 || !A) return fail(nullptr, GP_ERR_BAD_ARG, "gp_debug_potrf_inverse_batched: bad argument");
  int mask = -1;                // -1: the body failed before it read the flags back
  const int rc = potrf_inverse_hook(device, n, batch, with_workspace, A, L, Ainv, logdet, &mask);
  if (fail_mask && mask >= 0) *fail_mask = mask;
  if (rc != GP_OK) return rc;
  if (mask) return fail(nullptr, GP_ERR_NOT_PD, "gp_debug_potrf_inverse_batched: not positive definite (fail mask %d)", mask);
  return GP_OK;
}

// One of the two extended-precision products of the global step on the caller's operands (include/gparml_hip.h).  Everything the kernels take on
// trust is checked first and refused with GP_ERR_BAD_ARG before any HIP call; the context is a temporary one whose only device state is the int8
// workspace (gstep.gsd / gss, as GsState::alloc sizes it for form 0, as the product needs it for a forced int8 form).
namespace gp {
constexpr size_t DD_HOOK_I8_BYTES = (size_t)10 * 2048 * 4096;    // the largest workspace GsState::alloc gives a context with M, D <= 2048
static int dd_product_body(gp_ctx* c, int device, int residual, int form, const int* dims, double beta, double jitA, const double* A, const double* B,
                           const double* Csub, const double* Keep, const double* Psi2, double* out, int* form_ran) {
  auto bad = [&](const char* fmt, auto... a) {
    char what[200];
    snprintf(what, sizeof(what), fmt, a...);
    return fail(c, GP_ERR_BAD_ARG, "gp_debug_dd_product: %s", what);
  };
  if (!dims || !out || !form_ran || !B) return bad("NULL argument (dims, B, out and form_ran are always needed)");
  if (residual != 0 && residual != 1) return bad("product must be 0 (G) or 1 (residual), got %d", residual);
  if (form < 0 || form > DD_FORM_I8) return bad("form must be 0 (the step's choice) or 1 .. 4, got %d", form);
  const int M = dims[0], Mp = dims[1], Dp = dims[2];
  int nA = dims[3], nB = dims[4], K = dims[5];
  if (form == 0 || form == DD_FORM_ROW) {
    // the step's own shapes: a context pads M and D to multiples of 128
    if (Mp < NB || Mp % NB || Mp > 4096) return bad("Mp = %d must be a multiple of 128 in [128, 4096]", Mp);
    if (Dp < NB || Dp % NB || Dp > 4096) return bad("Dp = %d must be a multiple of 128 in [128, 4096]", Dp);
    if (nA || nB || K) return bad("nA, nB, K must be 0 with form %d: the sizes are Mp and Dp", form);
    nA = Mp; K = Mp; nB = residual ? Dp : Mp;
  }
  if (form == 0) {
    if (Mp == NB && Dp == NB && g_opt_gs_tail.load()) return bad("form 0 at Mp = Dp = 128: the step runs the fused one-panel tail there, not these products");
    if (!residual && !g_opt_dd_kipsi2.load()) return bad("form 0 with dd_kipsi2 off: the step forms G in plain float64");
    if (residual && !g_opt_refine_E.load()) return bad("form 0 with refine_E off: the step forms no residual");
  }
  if ((form == DD_FORM_GEMM && residual) || ((form == DD_FORM_RESIDUAL || form == DD_FORM_ROW) && !residual))
    return bad("form %d does not compute product %d", form, residual);
  if (form == DD_FORM_ROW && (M < 1 || M > Mp)) return bad("M = %d must be in [1, Mp]", M);
  if (form == DD_FORM_GEMM || form == DD_FORM_RESIDUAL) {
    if (nA < 8 || nA % 8 || nA > 4096) return bad("rows nA = %d must be a multiple of 8 in [8, 4096] (ddacc_block: 8 rows per workgroup)", nA);
    if (nB < 64 || nB % 64 || nB > 4096) return bad("cols nB = %d must be a multiple of 64 in [64, 4096] (ddacc_block: 64 columns per wave)", nB);
    if (K < 8 || K % 8 || K > 4096) return bad("K = %d must be a multiple of 8 in [8, 4096] (ddacc_block: 8 k per trip)", K);
  }
  if (form == DD_FORM_I8) {
    if (K < 32 || K % 32 || K > 2048) return bad("K = %d must be a multiple of 32 in [32, 2048] (int8 product: 32 k per step, int32 sums)", K);
    if (nA < 64 || nA % 64 || nA > 4096) return bad("nA = %d must be a multiple of 64 in [64, 4096] (int8 product: 64 x 64 per workgroup)", nA);
    if (nB < 64 || nB % 64 || nB > 4096) return bad("nB = %d must be a multiple of 64 in [64, 4096] (int8 product: 64 x 64 per workgroup)", nB);
    if ((size_t)10 * K * (nA + nB) > DD_HOOK_I8_BYTES) return bad("digit plane of %ld bytes: ten of them exceed the workspace (%zu bytes)", (long)K * (nA + nB), DD_HOOK_I8_BYTES);
  }
  if (residual && !Csub) return bad("the residual needs Csub");
  if (!residual && Csub) return bad("Csub given for G (the int8 product subtracts as product 1)");
  if (form == DD_FORM_ROW && (!Keep || !Psi2)) return bad("the row-residual form needs Keep and Psi2");
  if (form && form != DD_FORM_ROW && !A) return bad("form %d needs A", form);

  GP_HIP(c, hipSetDevice(device));
  c->device = device; c->M = M; c->Mp = Mp; c->Dp = Dp;
  size_t nd = 0, ns = 0;
  if (form == DD_FORM_I8) { nd = (size_t)10 * K * (nA + nB); ns = (size_t)nA + nB; }
  else if (form == 0 && Mp >= 512 && Mp <= 2048) { ns = (size_t)Mp + std::max(Mp, Dp); nd = (size_t)10 * Mp * ns; }     // GsState::alloc
  if (nd) {
    GP_TRY_RC(c->gstep.gsd.alloc(c, nd, DA_RAW)); GP_TRY_RC(c->gstep.gss.alloc(c, ns, DA_RAW));
    GP_HIP(c, hipMemset(c->gstep.gsd, 0xFF, c->gstep.gsd.bytes())); GP_HIP(c, hipMemset(c->gstep.gss, 0xFF, c->gstep.gss.bytes()));
  }
  if (form == 0) {
    const bool gi8 = gs_i8_wanted(c);
    form = residual ? residual_form(gi8, Mp, Dp) : G_form(gi8);
    if (form == DD_FORM_ROW) { if (!Keep || !Psi2) return bad("the step's choice here is the row-residual form: it needs Keep and Psi2"); if (M < 1 || M > Mp) return bad("M = %d must be in [1, Mp]", M); }
    else if (!A) return bad("the step's choice here is form %d: it needs A", form);
  }
  *form_ran = form;
  const size_t na = (size_t)nA * K, nb = (size_t)K * nB, no = (size_t)nA * nB, nout = no + 2 * (size_t)nB;
  DevBuf<double> dA, dB, dC, dKeep, dPsi2, dOut;
  auto up = [&](DevBuf<double>& d, const double* h, size_t n) {
    GP_TRY_RC(d.alloc(c, n, DA_RAW));
    GP_HIP(c, hipMemcpy(d, h, n * sizeof(double), hipMemcpyHostToDevice));
    return (int)GP_OK;
  };
  GP_TRY_RC(up(dB, B, nb));
  if (form != DD_FORM_ROW) GP_TRY_RC(up(dA, A, na));
  else { GP_TRY_RC(up(dKeep, Keep, na)); GP_TRY_RC(up(dPsi2, Psi2, na)); }
  if (Csub) GP_TRY_RC(up(dC, Csub, no));
  // NaN bytes in the result and its two sentinel rows: the product must write the first, and only the first
  GP_TRY_RC(dOut.alloc(c, nout, DA_RAW));
  GP_HIP(c, hipMemset(dOut, 0xFF, dOut.bytes()));
  const DdProduct p{dA, form == DD_FORM_I8 ? (long)nA : (long)K, nA, dB, (long)nB, nB, K, dOut, (long)nB, residual ? dC.get() : nullptr};
  if (residual) GP_TRY_RC(form_residual(c, nullptr, form, p, {dKeep, dPsi2, beta, jitA, M}));
  else GP_TRY_RC(form_G(c, nullptr, form, p));
  GP_HIP(c, hipDeviceSynchronize());
  GP_HIP(c, hipMemcpy(out, dOut, dOut.bytes(), hipMemcpyDeviceToHost));
  return GP_OK;
}
}  // namespace gp

extern "C" int gp_debug_dd_product(int device, int product, int form, const int* dims, double beta, double jitA, const double* A, const double* B,
                                   const double* Csub, const double* Keep, const double* Psi2, double* out, int* form_ran) {
  gp_ctx tmp;
  const int rc = gp::dd_product_body(&tmp, device, product, form, dims, beta, jitA, A, B, Csub, Keep, Psi2, out, form_ran);
  if (rc != GP_OK) gp::g_create_error = tmp.err;
  return rc;
}
