// Joint posterior predictive at new deterministic inputs (gp_predict_joint, gp_predict_sample), after a global step of this context.
//
// With k_i = psi1(x_i), a_i = Lk^-1 k_i and b_i = La^-1 k_i (the rows gp_predict's deterministic path forms from the global step's inverse Cholesky
// factors, predict.hip), the covariance of f between two new inputs is
//   cov_f[i][j] = k(x_i, x_j) - a_i . a_j + b_i . b_j          (one n x n matrix, shared by all D outputs)
// the inverse-factor form of gp_predict's variance (DESIGN.md sections 11 and 14): two Gram products of O(sqrt(sf2)) rows instead of a quadratic
// form in Ki - P.
//   R = [a | b] [np][2 Mp] and the centred inputs [np][Q] come from gp_predict's own chunk pipeline (pred_chunk_front), written into this plan;
//   pred_cov_kernel: one workgroup per 128 x 128 tile on or below the diagonal, four waves as 2 x 2 of 64 x 64 on the 4x4x4 FP64 MFMA (mma_f64.h:
//     tile_dma / mma_chunk / Acc, both operands K_CONTIG; a diagonal tile stages one operand and reads it twice).  k runs over [0, Mp) and then
//     [Mp, 2 Mp) in one accumulator set: at the boundary the matrix pipe is drained and the accumulators are negated, so the a-part enters with
//     weight -1.  The epilogue adds k(x_i, x_j) = sf2 exp(-1/2 sum_q alpha_q (x_iq - x_jq)^2) (difference first, q ascending, fexp) from the two
//     tiles' inputs transposed into LDS (Q <= JC_QS) or read from memory (any Q), and diag_add on the global diagonal; rows or columns >= n
//     become exact zeros, 1 on the diagonal.  The tile and, off the diagonal, its transpose (or zeros: the factorisation buffer) leave through
//     LDS in runs of 256 bytes and more.  cov[i][j] and cov[j][i] carry the same bits: an off-diagonal tile is stored twice, and on a diagonal
//     tile the two elements are the same products in the same k order and the same exponent ((alpha d) d does not see the sign of d).
//   draws: pred_cov_kernel with diag_add = noise + jitter sf2 straight into the factorisation buffer, potrf_inverse_batched (factor only), then
//     out = mean + Lc eps as launch_gemm products against the packed normals [np][draws x D], a group of draws at a time.
// No floating-point atomics, fixed summation order: results are bit-identical from run to run.  Every buffer belongs to the context's JointPlan
// (replaced whole when np grows); the evaluation's buffers are only read.
#include "pred_chunk.h"
#include "fexp.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int JC_QS = 32;            // latent width staged in LDS for k(x_i, x_j); beyond it the inputs are read from memory
constexpr int JC_XLD = TILE + 1;     // row stride of the transposed inputs [q][point]: the transposing stores of one point's q land on different banks
constexpr int JC_SLD = 65;           // row stride of the store image [128 rows][64 columns]: the accumulator layout writes, and rows and columns read, without conflicts
static_assert(2 * JC_QS * JC_XLD <= 4 * TILE_LDS_DOUBLES && TILE * JC_SLD <= 4 * TILE_LDS_DOUBLES, "the epilogue images overlay the operand tiles");

struct CovArgs {
  const double* R;      // [np][2 Mp] rows [a | b], k contiguous
  const double* X;      // [np][Q] centred inputs
  const double* alpha;  // [Q]
  double* cov;          // [np][np]
  long ld;              // np
  long n;
  int Mp, Q;
  double sf2, diag_add;
  int lower_only;       // 1: the tiles above the diagonal get zeros instead of the transpose (the factor's buffer: Lc is a GEMM operand afterwards)
};

// STAGED: the inputs of k(x_i, x_j) in LDS, two workgroups per CU; the plain path (any Q) takes one workgroup's register budget for its addresses
template <bool STAGED>
__global__ void __launch_bounds__(256, STAGED ? 2 : 1) pred_cov_kernel(CovArgs p) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][TILE_LDS_DOUBLES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wrow0 = (wave >> 1) * WT, wcol0 = (wave & 1) * WT;
  int ti = 0, rem = blockIdx.x;                               // tile pair ti >= tj of the lower triangle, row by row
  while (rem > ti) { rem -= ti + 1; ++ti; }
  const int tj = rem;
  const bool diag = ti == tj;
  const long row0 = (long)ti * TILE, col0 = (long)tj * TILE;
  const long ldr = 2L * p.Mp;
  const int nc = 2 * p.Mp / KC, nneg = p.Mp / KC;            // chunks in all, and of the a-part (>= 8: Mp is a multiple of 128)
  const double* Ab = p.R + row0 * ldr;
  const double* Bb = p.R + col0 * ldr;
  auto stage = [&](int buf, int c) {
    tile_dma<K_CONTIG>(lds[buf][0], Ab + (long)c * KC, ldr, wave, lane);
    if (!diag) tile_dma<K_CONTIG>(lds[buf][1], Bb + (long)c * KC, ldr, wave, lane);
  };

  Acc acc;
  const LaneOfs ofs = lane_offsets<K_CONTIG, K_CONTIG>(wrow0, wcol0, lane);
  stage(0, 0);
  dma_wait();
  __syncthreads();
  stage(1, 1);
  mma_chunk<K_CONTIG, K_CONTIG, true>(lds[0][0], lds[0][diag ? 0 : 1], acc, ofs);
  dma_wait();
  __syncthreads();
  for (int c = 1; c < nc; ++c) {
    const int cur = c & 1;
    if (c + 1 < nc) stage(cur ^ 1, c + 1);
    mma_chunk<K_CONTIG, K_CONTIG>(lds[cur][0], lds[cur][diag ? 0 : 1], acc, ofs);
    if (c + 1 == nneg) {
      // the a-part is complete: -sum a_i a_j, then the b-part accumulates on top.  Drained before the negation reads the accumulators; the fence and
      // the wait states keep the negating moves away from the next MFMA that takes them as SrcC (hipcc does not model the MFMAs inside the asm)
      acc.drain();
#pragma unroll
      for (int ar = 0; ar < 4; ++ar)
#pragma unroll
        for (int bc = 0; bc < 16; ++bc) acc.v[ar][bc] = -acc.v[ar][bc];
      acc.drain();
    }
    dma_wait();
    __syncthreads();
  }
  acc.drain();

  // ---- epilogue: + k(x_i, x_j), the diagonal term, the padding; every wave is past the barrier that ended the last chunk, the operand tiles are free
  double* img = &lds[0][0][0];
  if constexpr (STAGED) {
    for (int e = tid; e < TILE * p.Q; e += 256) {
      const int r = e / p.Q, q = e - r * p.Q;
      img[q * JC_XLD + r] = p.X[row0 * p.Q + e];
      img[(JC_QS + q) * JC_XLD + r] = p.X[col0 * p.Q + e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int ar = 0; ar < 4; ++ar) {
    // one 16-row group at a time, pinned by the volatile statements at both ends: hipcc otherwise runs the four exponent loops first and spills their sums
    int r = wrow0 + acc_row(ar, lane);
    asm volatile("" : "+v"(r));
    const long gi = row0 + r;
    // the columns in groups of GW: all 16 with the inputs in LDS; four at a time on the plain path, whose 64-bit addresses would not fit beside the accumulators
    constexpr int GW = STAGED ? 16 : 4;
#pragma unroll
    for (int b0 = 0; b0 < 16; b0 += GW) {
      double s[GW];
#pragma unroll
      for (int b = 0; b < GW; ++b) s[b] = 0.0;
#pragma unroll 1
      for (int q = 0; q < p.Q; ++q) {
        const double aq = p.alpha[q];
        const double xi = STAGED ? img[q * JC_XLD + r] : p.X[gi * p.Q + q];
#pragma unroll
        for (int b = 0; b < GW; ++b) {
          const int cc = wcol0 + acc_col(b0 + b, lane);
          const double xj = STAGED ? img[(JC_QS + q) * JC_XLD + cc] : p.X[(col0 + cc) * p.Q + q];
          const double d = xi - xj;
          s[b] = fma(aq * d, d, s[b]);
        }
      }
#pragma unroll
      for (int b = 0; b < GW; ++b) {
        const long gj = col0 + wcol0 + acc_col(b0 + b, lane);
        double v = p.sf2 * fexp(-0.5 * s[b]) + acc.v[ar][b0 + b];
        if (gi == gj) v += p.diag_add;
        if (gi >= p.n || gj >= p.n) v = gi == gj ? 1.0 : 0.0;
        acc.v[ar][b0 + b] = v;
      }
    }
    acc_fence(acc.v[ar]);
  }

  // ---- store: half of every wave's columns at a time through the image [128][64] (columns: 32 of the left waves' | 32 of the right waves')
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();                                          // the inputs / the previous half have been read
#pragma unroll
    for (int ar = 0; ar < 4; ++ar)
#pragma unroll
      for (int b8 = 0; b8 < 8; ++b8)
        img[(wrow0 + acc_row(ar, lane)) * JC_SLD + (wave & 1) * 32 + 4 * b8 + (lane & 3)] = acc.v[ar][8 * h + b8];
    __syncthreads();
    // rows: a half wave writes 32 consecutive columns (256 bytes)
#pragma unroll 4
    for (int it = 0; it < 32; ++it) {
      const int e = tid + 256 * it, r = e >> 6, cl = e & 63;
      const int tc = (cl >> 5) * WT + 32 * h + (cl & 31);
      p.cov[(row0 + r) * p.ld + col0 + tc] = img[r * JC_SLD + cl];
    }
    // the transpose of an off-diagonal tile: a wave writes 64 consecutive rows of one column as 512 bytes of the mirrored row
    if (!diag) {
#pragma unroll 4
      for (int it = 0; it < 32; ++it) {
        const int e = tid + 256 * it, cl = e >> 7, r = e & 127;
        const int tc = (cl >> 5) * WT + 32 * h + (cl & 31);
        p.cov[(col0 + tc) * p.ld + row0 + r] = p.lower_only ? 0.0 : img[r * JC_SLD + cl];
      }
    }
  }
}

// the draws' buffers: built on the first gp_predict_sample of a plan
struct JointDraw {
  DevBuf<double> Linv;        // [np][np] potrf_inverse_batched's inverse diagonal blocks (zero above the block diagonal: its precondition)
  DevBuf<double> Twork;       // [np][np / 2] its work panel
  DevBuf<double> flags;       // [2] log-determinant | failure flag
  DevBuf<double> eps;         // [np][cols] packed normals of a group of draws, one column per (draw, output); rows >= n and unused columns zero
  DevBuf<double> out;         // [np][cols] mean + Lc eps
};

struct JointPlan {
  long np = 0;
  DevBuf<double> R;           // [np][2 Mp] [Lk^-1 k* | La^-1 k*] of every point
  DevBuf<double> X;           // [np][Q] centred inputs
  DevBuf<double> mean;        // [np][D]
  DevBuf<double> cov;         // [np][np] the covariance; for draws the factorisation's matrix: cov_y + jitter sf2 I in, Lc out
  std::unique_ptr<JointDraw> draw;
};
void JointPlanDelete::operator()(JointPlan* p) const { delete p; }

// Built aside and published whole; replaced whole when np grows.  A smaller call runs in the larger plan's buffers with its own leading
// dimensions, so its results do not depend on what ran before.  Every element is written before it is read (DA_RAW) except Linv's zero contract.
static int joint_alloc(gp_ctx* c, long np, bool draws) {
  auto A = [c](DevBuf<double>& b, long n, int mode = DA_RAW) { return b.alloc(c, (size_t)n, mode); };
  if (!c->joint || c->joint->np < np) {
    c->joint.reset();
    std::unique_ptr<JointPlan, JointPlanDelete> p(new JointPlan());
    GP_TRY_RC(A(p->R, np * 2 * c->Mp)); GP_TRY_RC(A(p->X, np * c->Q)); GP_TRY_RC(A(p->mean, np * c->D)); GP_TRY_RC(A(p->cov, np * np));
    p->np = np;
    c->joint = std::move(p);
  }
  if (draws && !c->joint->draw) {
    const long P = c->joint->np;
    auto d = std::make_unique<JointDraw>();
    GP_TRY_RC(A(d->Linv, P * P, DA_ZERO));   // zero contract: the 128-blocks above the block diagonal are never written (potrf_inverse_batched's precondition)
    GP_TRY_RC(A(d->Twork, P * P / 2)); GP_TRY_RC(A(d->flags, 2));
    c->joint->draw = std::move(d);
  }
  return GP_OK;
}

// R, the centred inputs and the mean of all n points through gp_predict's chunk pipeline
static int joint_rows(gp_ctx* c, long n, const double* X) {
  const JointPlan& p = *c->joint;
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  for (long n0 = 0; n0 < n; n0 += k.rows) {
    const long cnt = std::min(k.rows, n - n0);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), n0, cnt, pred_into(p.X + n0 * c->Q).factors(p.R + n0 * 2 * c->Mp, 2L * c->Mp)));
    GP_TRY_RC(pred_chunk_mean(c, cnt, p.mean + n0 * c->D));
  }
  return GP_OK;
}

static int launch_cov(gp_ctx* c, long n, long np, double diag_add, int lower_only) {
  const JointPlan& p = *c->joint;
  CovArgs a;
  a.R = p.R; a.X = p.X; a.alpha = c->alpha; a.cov = p.cov; a.ld = np; a.n = n; a.Mp = c->Mp; a.Q = c->Q;
  a.sf2 = c->sf2; a.diag_add = diag_add; a.lower_only = lower_only;
  const long nt = np / TILE;
  const dim3 grid((unsigned)(nt * (nt + 1) / 2));
  if (c->Q <= JC_QS) GP_LAUNCH(c, c->stream, pred_cov_kernel<true>, grid, dim3(256), 0, a);
  else GP_LAUNCH(c, c->stream, pred_cov_kernel<false>, grid, dim3(256), 0, a);
  return GP_OK;
}

int run_predict_joint(gp_ctx* c, long n, const double* X, int flags, double* mean, double* cov) {
  const long np = round_up(n, TILE), D = c->D;
  GP_TRY_RC(joint_alloc(c, np, false));
  const JointPlan& p = *c->joint;
  hipStream_t st = c->stream;
  GP_TRY_RC(joint_rows(c, n, X));
  if (mean) GP_HIP(c, hipMemcpyAsync(mean, p.mean, (size_t)(n * D) * 8, hipMemcpyDeviceToHost, st));
  if (cov) {
    GP_TRY_RC(launch_cov(c, n, np, (flags & 1) ? 1.0 / c->beta : 0.0, 0));
    GP_HIP(c, hipMemcpy2DAsync(cov, (size_t)n * 8, p.cov, (size_t)np * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

int run_predict_sample(gp_ctx* c, long n, const double* X, int flags, double jitter, int n_draws, const double* eps, double* out, double* mean) {
  const long np = round_up(n, TILE), D = c->D;
  GP_TRY_RC(joint_alloc(c, np, true));
  const JointPlan& p = *c->joint;
  JointDraw& d = *p.draw;
  hipStream_t st = c->stream;
  // draws per group: the packed buffer [np][cols] stays near 64 MB
  const long group = std::max<long>(1, std::min<long>(n_draws, (64L << 20) / (8 * np) / D)), cols = round_up(group * D, TILE);
  GP_TRY_RC(d.eps.grow(c, (size_t)(np * cols), DA_RAW));
  GP_TRY_RC(d.out.grow(c, (size_t)(np * cols), DA_RAW));
  GP_TRY_RC(joint_rows(c, n, X));
  if (mean) GP_HIP(c, hipMemcpyAsync(mean, p.mean, (size_t)(n * D) * 8, hipMemcpyDeviceToHost, st));
  // cov_y + jitter sf2 I straight into the factorisation's matrix (zeros above the block diagonal), Lc in place
  GP_TRY_RC(launch_cov(c, n, np, ((flags & 1) ? 1.0 / c->beta : 0.0) + jitter * c->sf2, 1));
  GP_HIP(c, hipMemsetAsync(d.flags, 0, d.flags.bytes(), st));
  GP_TRY_RC(potrf_inverse_batched(c, st, (int)np, 1, p.cov, d.Linv, nullptr, d.Twork, d.flags, d.flags + 1, nullptr, 0, true));
  for (long s0 = 0; s0 < n_draws; s0 += group) {
    const long g = std::min<long>(group, n_draws - s0);
    GP_HIP(c, hipMemsetAsync(d.eps, 0, (size_t)(np * cols) * 8, st));
    for (long s = 0; s < g; ++s)
      GP_HIP(c, hipMemcpy2DAsync(d.eps + s * D, (size_t)cols * 8, eps + (s0 + s) * n * D, (size_t)D * 8, (size_t)D * 8, (size_t)n, hipMemcpyHostToDevice, st));
    GP_TRY_RC(pred_fill_mean(c, p.mean, n, np, cols, g * D, d.out));
    // out += Lc eps: Lc [i][k] K_CONTIG, eps [k][column] FREE_CONTIG
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)np, (int)cols, 1, gemm_of({p.cov, np}, {d.eps, cols}, {d.out, cols}, (int)np, 1.0, 1.0)));
    for (long s = 0; s < g; ++s)
      GP_HIP(c, hipMemcpy2DAsync(out + (s0 + s) * n * D, (size_t)D * 8, d.out + s * D, (size_t)cols * 8, (size_t)D * 8, (size_t)n, hipMemcpyDeviceToHost, st));
  }
  double h[2];
  GP_HIP(c, hipMemcpyAsync(h, d.flags, sizeof(h), hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  if (h[1] != 0.0)
    return fail(c, GP_ERR_NOT_PD, "gp_predict_sample: the joint covariance plus (noise + jitter sf2) I is not positive definite (Cholesky failed); raise jitter");
  return GP_OK;
}

}  // namespace gp
