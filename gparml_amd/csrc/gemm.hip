// Generic FP64 GEMM on the 4x4x4 matrix-core instruction (see mma_f64.h): 128x128 tile per 256-thread
// workgroup, 16-deep k-chunks double-buffered through LDS, two workgroups per CU.
// Used by the global step (M x M algebra) and, through the same building blocks, by the phase kernels.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "gp_common.h"
#include "gemm32.h"
#include <algorithm>
#include <cstdlib>

namespace gp {

template <Layout LA, Layout LB>
__global__ void __launch_bounds__(256, 2) gemm128_kernel(GemmP p) {
  const int bx = blockIdx.x, by = blockIdx.y;
  const int bz = blockIdx.z / p.splits, sp = blockIdx.z % p.splits;
  if (p.tri == 1 && bx > by) return;
  if (p.tri == 2 && bx < by) return;
  __shared__ __attribute__((aligned(16))) double lds[2][2][TILE_LDS_DOUBLES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wrow0 = (wave >> 1) * WT, wcol0 = (wave & 1) * WT;
  const int bi = bz % p.inner, bo = bz / p.inner;
  const double* A = p.A + (long)bi * p.sA + (long)bo * p.oA;
  const double* B = p.B + (long)bi * p.sB + (long)bo * p.oB;
  double* C = p.C + (long)bi * p.sC + (long)bo * p.oC;
  const long row0 = (long)by * TILE, col0 = (long)bx * TILE;
  // klow (X^T X, X lower-triangular): the tile's k-range starts at its first possibly non-zero k, a multiple of 128.  The splits keep the boundaries of
  // the full product (K / splits each) and drop the chunks below klo from their own segment -- those are exact zeros at the head of a sequential sum, so
  // every partial tile, and with it the result, has the bits of the product without klow (a segment wholly below klo gives a zero partial at no cost;
  // the longest workgroup is a split of a klo = 0 tile either way)
  const long klo = p.klow ? (row0 > col0 ? row0 : col0) : 0;
  const int ncs = (int)(p.K / KC / p.splits);                 // chunks of a split's segment
  const long seg0 = (long)sp * ncs * KC;
  const int skip = klo <= seg0 ? 0 : (klo - seg0) / KC < ncs ? (int)((klo - seg0) / KC) : ncs;
  const int nc = ncs - skip;                                  // chunks of this split
  const long k0 = seg0 + (long)skip * KC;
  const double* Ab = (LA == K_CONTIG) ? A + row0 * p.lda + k0 : A + row0 + k0 * p.lda;
  const double* Bb = (LB == K_CONTIG) ? B + col0 * p.ldb + k0 : B + col0 + k0 * p.ldb;
  const long a_step = (LA == K_CONTIG) ? KC : (long)KC * p.lda;
  const long b_step = (LB == K_CONTIG) ? KC : (long)KC * p.ldb;

  Acc acc;
  acc.zero();
  const LaneOfs ofs = lane_offsets<LA, LB>(wrow0, wcol0, lane);
  if (nc > 0) {                                               // (workgroup-uniform; an empty segment stores its zero partial)
    tile_dma<LA>(lds[0][0], Ab, p.lda, wave, lane);
    tile_dma<LB>(lds[0][1], Bb, p.ldb, wave, lane);
    dma_wait();
    __syncthreads();
  }
  for (int c = 0; c < nc; ++c) {
    const int cur = c & 1;
    if (c + 1 < nc) {
      tile_dma<LA>(lds[cur ^ 1][0], Ab + (long)(c + 1) * a_step, p.lda, wave, lane);
      tile_dma<LB>(lds[cur ^ 1][1], Bb + (long)(c + 1) * b_step, p.ldb, wave, lane);
    }
    mma_chunk<LA, LB>(lds[cur][0], lds[cur][1], acc, ofs);
    dma_wait();
    __syncthreads();
  }
  acc.drain();
  if (p.splits > 1) {
    // raw partial tile, [z][by][bx][split][128*128]
    double* w = p.ws + ((((long)bz * gridDim.y + by) * gridDim.x + bx) * p.splits + sp) * (TILE * TILE);
#pragma unroll
    for (int ar = 0; ar < 4; ++ar)
#pragma unroll
      for (int bc = 0; bc < 16; ++bc) w[(wrow0 + acc_row(ar, lane)) * TILE + wcol0 + acc_col(bc, lane)] = acc.v[ar][bc];
    return;
  }
  if (p.beta != 0.0) {
#pragma unroll
    for (int ar = 0; ar < 4; ++ar)
#pragma unroll
      for (int bc = 0; bc < 16; ++bc) {
        const long r = row0 + wrow0 + acc_row(ar, lane), cc = col0 + wcol0 + acc_col(bc, lane);
        C[r * p.ldc + cc] = p.alpha * acc.v[ar][bc] + p.beta * C[r * p.ldc + cc];
      }
  } else {
#pragma unroll
    for (int ar = 0; ar < 4; ++ar)
#pragma unroll
      for (int bc = 0; bc < 16; ++bc) {
        const long r = row0 + wrow0 + acc_row(ar, lane), cc = col0 + wcol0 + acc_col(bc, lane);
        C[r * p.ldc + cc] = p.alpha * acc.v[ar][bc];
        if (p.mirror && bx != by) C[cc * p.ldc + r] = p.alpha * acc.v[ar][bc];
      }
  }
}

// Small-tile variant for the latency-bound products of the global step: see gemm32.h (the tile product is a device function shared with the
// fused small-M tail of the global step).
template <Layout LA, Layout LB>
__global__ void __launch_bounds__(256, 1) gemm32_kernel(GemmP p) {
  __shared__ __attribute__((aligned(16))) double sA[SmallImg<LA>::DOUBLES];
  __shared__ __attribute__((aligned(16))) double sB[SmallImg<LB>::DOUBLES];
  gemm32_tile<LA, LB>(p, blockIdx.x, blockIdx.y, blockIdx.z, sA, sB);
}

__global__ void __launch_bounds__(256) gemm_splitk_reduce_kernel(GemmP p, int tiles_x, int tiles_y) {
  // grid (tiles * 16, batch): 16 blocks of 256 threads per 128x128 tile, one 32 x 32 sub-block each (four elements per thread, rows of 32 doubles);
  // the mirrored copy of an off-diagonal tile (GemmP::mirror) goes through an LDS transposition so that it, too, is written in 256-byte runs
  // (as scattered 8-byte stores the reduce of X^T X took 29 us at M = 1024 against 15 us for the other products)
  __shared__ double tr[32][33];
  const int tile = blockIdx.x >> 4, sub = blockIdx.x & 15;
  const int bx = tile % tiles_x, by = tile / tiles_x, bz = blockIdx.y;
  if (p.tri == 1 && bx > by) return;
  if (p.tri == 2 && bx < by) return;
  const int bi = bz % p.inner, bo = bz / p.inner;
  double* C = p.C + (long)bi * p.sC + (long)bo * p.oC;
  const double* w = p.ws + (((long)bz * tiles_y + by) * tiles_x + bx) * p.splits * (TILE * TILE);
  const int sr = 32 * (sub >> 2), sc = 32 * (sub & 3), lc = threadIdx.x & 31, lr0 = threadIdx.x >> 5;
  const bool mir = p.mirror && bx != by;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = 8 * i + lr0;
    const int e = (sr + lr) * TILE + sc + lc;
    double s = 0.0;
    for (int sp = 0; sp < p.splits; ++sp) s += w[(long)sp * (TILE * TILE) + e];
    const long r = (long)by * TILE + sr + lr, cc = (long)bx * TILE + sc + lc;
    const double v = p.alpha * s + (p.beta != 0.0 ? p.beta * C[r * p.ldc + cc] : 0.0);
    C[r * p.ldc + cc] = v;
    if (mir) tr[lr][lc] = v;
  }
  if (mir) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = 8 * i + lr0;      // row of the transposed sub-block = column of the original
      C[((long)bx * TILE + sc + lr) * p.ldc + (long)by * TILE + sr + lc] = tr[lc][lr];
    }
  }
}

// Does the stored rectangle of an operand (rows x cols doubles, leading dimension ld, first element at element address x0) share an element with C (m x n, ldc, at c0)?
// Same leading dimension = two windows of one parent matrix: row and column ranges from the address difference; otherwise the address ranges decide (conservative).
bool windows_meet(long x0, long rows, long cols, long ld, long c0, long m, long n, long ldc) {
  const long x1 = x0 + (rows - 1) * ld + cols, c1 = c0 + (m - 1) * ldc + n;
  if (x1 <= c0 || c1 <= x0) return false;
  if (ld != ldc) return true;
  const long d = c0 - x0, dr = (d >= 0 ? d : d - (ld - 1)) / ld, dc = d - dr * ld;   // C(0,0) sits at row dr, column dc of X's frame (floor division)
  auto hit = [&](long r0, long k0) { return r0 < rows && r0 + m > 0 && k0 < cols && k0 + n > 0; };
  return hit(dr, dc) || hit(dr + 1, dc - ld);                                        // the same place one row further down, ld columns to the left
}
static bool operand_meets_c(const double* X, long rows, long cols, long ld, const double* C, long m, long n, long ldc) {
  return windows_meet((long)(reinterpret_cast<uintptr_t>(X) / sizeof(double)), rows, cols, ld, (long)(reinterpret_cast<uintptr_t>(C) / sizeof(double)), m, n, ldc);
}

// What launch_gemm refuses, as a reason, or NULL for an acceptable call.  Both are programming errors, never a user's.
//  - No product may write a tile another workgroup still reads: C must not share an element with A or B (the in-place panel solve of the blocked
//    Cholesky did until r06 -- a race visible only on a cold start, profiles/r06_first_evaluation_race.txt).  Only batch entry 0 is looked at;
//    gp_debug_gemm_modes checks every pair of entries itself.
//  - mirror is defined for beta == 0 only (GemmP): with a beta the three kernels would each do something else.
static const char* gemm_refusal(Layout la, Layout lb, int m, int n, const GemmP& p) {
  if (operand_meets_c(p.A, la == K_CONTIG ? m : p.K, la == K_CONTIG ? p.K : m, p.lda, p.C, m, n, p.ldc) ||
      operand_meets_c(p.B, lb == K_CONTIG ? n : p.K, lb == K_CONTIG ? p.K : n, p.ldb, p.C, m, n, p.ldc))
    return "C overlaps an operand";
  if (p.mirror && p.beta != 0.0) return "mirror with beta != 0";
  return nullptr;
}

int launch_gemm(gp_ctx* c, hipStream_t st, Layout la, Layout lb, int m, int n, int batch, const GemmP& p) {
  if (const char* why = gemm_refusal(la, lb, m, n, p)) return fail(c, GP_ERR_STATE, "launch_gemm: %s (m %d n %d k %d)", why, m, n, p.K);
  dim3 grid(n / TILE, m / TILE, batch * p.splits), block(256);
  if (!p.big && (long)(n / TILE) * (m / TILE) * batch <= 256) {
    // few tiles (the global step): 32 x 32 tiles spread the product over the chip; split-k is not needed there
    dim3 g32(n / ST, m / ST, batch);
    if (la == K_CONTIG && lb == FREE_CONTIG) GP_LAUNCH(c, st, (gemm32_kernel<K_CONTIG, FREE_CONTIG>), g32, block, 0, p);
    else if (la == K_CONTIG && lb == K_CONTIG) GP_LAUNCH(c, st, (gemm32_kernel<K_CONTIG, K_CONTIG>), g32, block, 0, p);
    else if (la == FREE_CONTIG && lb == FREE_CONTIG) GP_LAUNCH(c, st, (gemm32_kernel<FREE_CONTIG, FREE_CONTIG>), g32, block, 0, p);
    else GP_LAUNCH(c, st, (gemm32_kernel<FREE_CONTIG, K_CONTIG>), g32, block, 0, p);
    return GP_OK;
  }
  if (la == K_CONTIG && lb == FREE_CONTIG) GP_LAUNCH(c, st, (gemm128_kernel<K_CONTIG, FREE_CONTIG>), grid, block, 0, p);
  else if (la == K_CONTIG && lb == K_CONTIG) GP_LAUNCH(c, st, (gemm128_kernel<K_CONTIG, K_CONTIG>), grid, block, 0, p);
  else if (la == FREE_CONTIG && lb == FREE_CONTIG) GP_LAUNCH(c, st, (gemm128_kernel<FREE_CONTIG, FREE_CONTIG>), grid, block, 0, p);
  else GP_LAUNCH(c, st, (gemm128_kernel<FREE_CONTIG, K_CONTIG>), grid, block, 0, p);
  if (p.splits > 1)
    GP_LAUNCH(c, st, gemm_splitk_reduce_kernel, dim3((n / TILE) * (m / TILE) * 16, batch), block, 0, p, n / TILE, m / TILE);
  return GP_OK;
}

}  // namespace gp

// ---- test hook -------------------------------------------------------------------------------------------------
extern "C" int gp_debug_operands_overlap(long x_off, long rows, long cols, long ld, long c_off, long m, long n, long ldc) {
  return gp::windows_meet(x_off, rows, cols, ld, c_off, m, n, ldc) ? 1 : 0;
}

extern "C" int gp_debug_gemm(int device, int ta, int tb, int m, int n, int k, double alpha, const double* A, const double* B,
                             double beta, double* C) {
  using namespace gp;
  gp_ctx* ctx = nullptr;
  if (m <= 0 || n <= 0 || k <= 0 || !A || !B || !C) return fail(ctx, GP_ERR_BAD_ARG, "gp_debug_gemm: bad argument");
  GP_HIP(ctx, hipSetDevice(device));
  const long mp = round_up(m, TILE), np = round_up(n, TILE), kp = round_up(k, KC);
  // A stored (m,k) row-major [K_CONTIG] or (k,m) [FREE_CONTIG]; B stored (k,n) [FREE_CONTIG] or (n,k) [K_CONTIG]
  const long a_rows = ta ? kp : mp, a_cols = ta ? mp : kp, b_rows = tb ? np : kp, b_cols = tb ? kp : np;
  std::vector<double> hA(a_rows * a_cols, 0.0), hB(b_rows * b_cols, 0.0), hC(mp * np, 0.0);
  const long ar = ta ? k : m, ac = ta ? m : k, br = tb ? n : k, bc = tb ? k : n;
  for (long i = 0; i < ar; ++i) for (long j = 0; j < ac; ++j) hA[i * a_cols + j] = A[i * ac + j];
  for (long i = 0; i < br; ++i) for (long j = 0; j < bc; ++j) hB[i * b_cols + j] = B[i * bc + j];
  for (long i = 0; i < m; ++i) for (long j = 0; j < n; ++j) hC[i * np + j] = C[i * n + j];
  DevBuf<double> dA, dB, dC;
  GP_TRY_RC(dA.alloc(ctx, hA.size(), DA_RAW));
  GP_TRY_RC(dB.alloc(ctx, hB.size(), DA_RAW));
  GP_TRY_RC(dC.alloc(ctx, hC.size(), DA_RAW));
  GP_HIP(ctx, hipMemcpy(dA, hA.data(), hA.size() * 8, hipMemcpyHostToDevice));
  GP_HIP(ctx, hipMemcpy(dB, hB.data(), hB.size() * 8, hipMemcpyHostToDevice));
  GP_HIP(ctx, hipMemcpy(dC, hC.data(), hC.size() * 8, hipMemcpyHostToDevice));
  GP_TRY_RC(launch_gemm(ctx, nullptr, ta ? FREE_CONTIG : K_CONTIG, tb ? K_CONTIG : FREE_CONTIG, (int)mp, (int)np, 1,
                        gemm_of({dA, a_cols}, {dB, b_cols}, {dC, np}, (int)kp, alpha, beta)));
  GP_HIP(ctx, hipDeviceSynchronize());
  GP_HIP(ctx, hipMemcpy(hC.data(), dC, hC.size() * 8, hipMemcpyDeviceToHost));
  for (long i = 0; i < m; ++i) for (long j = 0; j < n; ++j) C[i * n + j] = hC[i * np + j];
  return GP_OK;
}

// One launch_gemm with every GemmP field chosen by the caller (include/gparml_hip.h).  Everything launch_gemm or a kernel takes on trust is checked here
// first -- windows inside their parents for every batch entry, 16-byte alignment, the split-k divisibility, mirror without beta, the overlap rule --
// and refused with GP_ERR_BAD_ARG: no call reaches launch_gemm's own refusals (GP_ERR_STATE) or reads or writes outside a parent buffer.
extern "C" int gp_debug_gemm_modes(int device, int la, int lb, int m, int n, int k, int batch_inner, int batch_outer, const long* geom, double alpha,
                                   double beta, const int* mode, const double* A, const double* B, double* C) {
  using namespace gp;
  gp_ctx* ctx = nullptr;
  auto bad = [&](const char* what) { return fail(ctx, GP_ERR_BAD_ARG, "gp_debug_gemm_modes: %s", what); };
  if (!geom || !mode || !A || !B || !C) return bad("NULL argument");
  if ((la != 0 && la != 1) || (lb != 0 && lb != 1)) return bad("layout must be 0 (free index contiguous) or 1 (k contiguous)");
  if (m <= 0 || n <= 0 || k <= 0 || m % TILE || n % TILE || k % KC) return bad("unaligned size (m, n multiples of 128, k of 16)");
  if (batch_inner < 1 || batch_outer < 1 || (long)batch_inner * batch_outer > 64) return bad("batch counts must be >= 1, at most 64 entries");
  const int tri = mode[0], klow = mode[1], mirror = mode[2], splits = mode[3], big = mode[4];
  if (tri < 0 || tri > 2 || (klow & ~1) || (mirror & ~1) || (big & ~1) || splits < 1 || splits > 16) return bad("mode out of range");
  if (mirror && beta != 0.0) return bad("mirror requires beta == 0");
  if (mirror && (m != n || tri != 1)) return bad("mirror needs a square result and tri == 1");
  if (klow && (m != n || k != m || la != FREE_CONTIG || lb != FREE_CONTIG)) return bad("klow needs m == n == k and both operands stored [k][free]");
  const int batch = batch_inner * batch_outer, tx = n / TILE, ty = m / TILE;
  for (int by = 0; by < ty; ++by)
    for (int bx = 0; bx < tx; ++bx) {
      if ((tri == 1 && bx > by) || (tri == 2 && bx < by)) continue;
      const long klo = klow ? (long)std::max(by, bx) * TILE : 0;
      if (((k - klo) / KC) % splits != 0) return bad("splits does not divide the k-chunks of every tile");
    }
  // the three windows: element offset, rows, cols, leading dimension, inner / outer batch stride, length of the parent
  struct Win { long off, rows, cols, ld, s, o, len; const void* host; };
  const Win w[3] = {{geom[9], la == K_CONTIG ? m : k, la == K_CONTIG ? k : m, geom[0], geom[3], geom[6], geom[12], A},
                    {geom[10], lb == K_CONTIG ? n : k, lb == K_CONTIG ? k : n, geom[1], geom[4], geom[7], geom[13], B},
                    {geom[11], m, n, geom[2], geom[5], geom[8], geom[14], C}};
  auto at = [&](const Win& x, int bz) { return x.off + (long)(bz % batch_inner) * x.s + (long)(bz / batch_inner) * x.o; };
  for (const Win& x : w) {
    if (x.ld < x.cols || x.off < 0 || x.s < 0 || x.o < 0 || x.len <= 0) return bad("leading dimension below the window's width, or a negative offset or stride");
    if ((x.ld | x.off | x.s | x.o) & 1) return bad("offsets, strides and leading dimensions must be even (16-byte rows)");
    for (int bz = 0; bz < batch; ++bz)
      if (at(x, bz) + (x.rows - 1) * x.ld + x.cols > x.len) return bad("a window runs past its parent buffer");
  }
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (w[i].host == w[j].host && w[i].len != w[j].len) return bad("one parent buffer passed with two lengths");
  // the overlap rule, for every pair of batch entries (launch_gemm checks the first): an operand in C's parent must not meet any C window,
  // and no two C windows may meet
  for (int bc = 0; bc < batch; ++bc) {
    for (int i = 0; i < 2; ++i)
      if (w[i].host == w[2].host)
        for (int bz = 0; bz < batch; ++bz)
          if (windows_meet(at(w[i], bz), w[i].rows, w[i].cols, w[i].ld, at(w[2], bc), m, n, w[2].ld)) return bad("C overlaps an operand");
    for (int bz = bc + 1; bz < batch; ++bz)
      if (windows_meet(at(w[2], bz), m, n, w[2].ld, at(w[2], bc), m, n, w[2].ld)) return bad("the C windows of two batch entries overlap");
  }
  GP_HIP(ctx, hipSetDevice(device));
  // one device buffer per distinct host parent (the trailing update of the Cholesky has A == B and C in the same matrix)
  DevBuf<double> d[3], dW;
  double* dev[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < i; ++j) if (w[j].host == w[i].host) dev[i] = dev[j];
    if (dev[i]) continue;
    GP_TRY_RC(d[i].alloc(ctx, (size_t)w[i].len, DA_RAW));
    GP_HIP(ctx, hipMemcpy(d[i], w[i].host, (size_t)w[i].len * 8, hipMemcpyHostToDevice));
    dev[i] = d[i];
  }
  if (splits > 1) {
    // split-k workspace: batch * tiles * splits partial tiles, filled with NaN bytes so that a partial nobody wrote shows in the sum
    GP_TRY_RC(dW.alloc(ctx, (size_t)batch * tx * ty * splits * TILE * TILE, DA_RAW));
    GP_HIP(ctx, hipMemset(dW, 0xFF, dW.bytes()));
  }
  auto in = [&](int i) { return GemmIn{dev[i] + w[i].off, w[i].ld, w[i].s, w[i].o}; };
  GP_TRY_RC(launch_gemm(ctx, nullptr, la == K_CONTIG ? K_CONTIG : FREE_CONTIG, lb == K_CONTIG ? K_CONTIG : FREE_CONTIG, m, n, batch,
                        gemm_of(in(0), in(1), {dev[2] + w[2].off, w[2].ld, w[2].s, w[2].o}, k, alpha, beta)
                            .triangle(tri, klow, mirror).batched(batch_inner).split(splits, dW.get()).on_big(big)));
  GP_HIP(ctx, hipDeviceSynchronize());
  GP_HIP(ctx, hipMemcpy(C, dev[2], (size_t)w[2].len * 8, hipMemcpyDeviceToHost));
  return GP_OK;
}

// device-resident timing of the GEMM core (tools/ only; not part of the public header)
extern "C" int gp_debug_gemm_bench(int device, int ta, int tb, int m, int n, int k, int iters, double* ms_out) {
  using namespace gp;
  const int fill = env_int("GP_BENCH_FILL", 0);  // 0 random, 1 zeros, 2 constant
  gp_ctx* ctx = nullptr;
  GP_HIP(ctx, hipSetDevice(device));
  const long mp = round_up(m, TILE), np = round_up(n, TILE), kp = round_up(k, KC);
  const long a_cols = ta ? mp : kp, b_cols = tb ? kp : np;
  const size_t na = (size_t)mp * kp, nb = (size_t)np * kp, ncc = (size_t)mp * np;
  std::vector<double> h(std::max(na, nb));
  unsigned long long s = 88172645463325252ULL;
  for (auto& x : h) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; x = (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; if (fill == 1) x = 0.0; if (fill == 2) x = 1.25; }
  DevBuf<double> dA, dB, dC;
  GP_TRY_RC(dA.alloc(ctx, na, DA_RAW)); GP_TRY_RC(dB.alloc(ctx, nb, DA_RAW)); GP_TRY_RC(dC.alloc(ctx, ncc, DA_RAW));
  GP_HIP(ctx, hipMemcpy(dA, h.data(), na * 8, hipMemcpyHostToDevice));
  GP_HIP(ctx, hipMemcpy(dB, h.data(), nb * 8, hipMemcpyHostToDevice));
  const GemmP p = gemm_of({dA, a_cols}, {dB, b_cols}, {dC, np}, (int)kp);
  hipEvent_t e0, e1;
  GP_HIP(ctx, hipEventCreate(&e0)); GP_HIP(ctx, hipEventCreate(&e1));
  GP_TRY_RC(launch_gemm(ctx, nullptr, ta ? FREE_CONTIG : K_CONTIG, tb ? K_CONTIG : FREE_CONTIG, (int)mp, (int)np, 1, p));
  GP_HIP(ctx, hipDeviceSynchronize());
  GP_HIP(ctx, hipEventRecord(e0));
  for (int i = 0; i < iters; ++i) GP_TRY_RC(launch_gemm(ctx, nullptr, ta ? FREE_CONTIG : K_CONTIG, tb ? K_CONTIG : FREE_CONTIG, (int)mp, (int)np, 1, p));
  GP_HIP(ctx, hipEventRecord(e1));
  GP_HIP(ctx, hipEventSynchronize(e1));
  float ms;
  GP_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
  *ms_out = ms / iters;
  return GP_OK;
}
