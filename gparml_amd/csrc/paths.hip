// Pathwise posterior function draws (gp_paths_set, gp_paths_eval, gp_paths_clear), after a global step of this context: Matheron's rule on a
// random Fourier prior.
//
// The ARD-RBF prior in F frequency pairs: with the caller's frequencies omega (F, Q) and a centre c,
//   theta_f(x) = sum_q omega[f][q] (x_q - c_q)                 (difference first, q ascending, one fused multiply-add per term)
//   phi(x) = sqrt(sf2 / F) [cos theta_0 .. cos theta_{F-1}, sin theta_0 .. sin theta_{F-1}]
// and with a_i = Lk^-1 k(x_i), b_i = La^-1 k(x_i) (gp_predict's inverse-factor rows, pred_chunk_front) a draw s of the posterior function is
//   out[s][i][d] = mean[i][d] + phi(x_i) . w_s[:, d] - a_i . G_s[:, d] + b_i . eps_s[:, d],     G_s = Lk^-1 Phi_Z w_s  (once, in gp_paths_set)
// w (S, 2F, D) and eps_u (S, M, D) standard normals of the caller.  No n x n matrix: the work is linear in n.
//   paths_feature_kernel: one wave per 64 rows x 64 frequencies; lane = row holds its centred coordinates in registers, omega is read with
//     wave-uniform (scalar) loads, one FP64 sincos per (row, f) gives both features; 16 frequencies at a time leave through an LDS image so that
//     every row is written in runs of 128 bytes, k-contiguous, next to the chunk's [a | b]: one left operand [rows][Kf + 2 Mp], Kf = 2F rounded up
//     to 16 (the columns between are written as zeros).  The same kernel on the rows of Z gives Phi_Z: one definition of a feature.
//   gp_paths_set: the packed right-hand operand B = [Wt ; -G ; E], (Kf + 2 Mp) rows x (S D rounded up to 128) columns, column s D + d; padding rows
//     and columns are exact zeros.  G = Lk^-1 (Phi_Z Wt): two launch_gemm products.
//   gp_paths_eval, per chunk of rows: pred_chunk_front (mean, [a | b]), the features, then ONE product left operand x B with beta = 1 on a buffer
//     pre-filled with the mean; a transposing kernel puts it in the caller's [s][i][d] order and one strided copy per chunk takes it to the host.
//   gp_paths_grad, per chunk of points: the derivative of the same sum with respect to x_q, one row per (point, q).  The
//     left operand [dphi_q | a'_q | b'_q] (paths_dfeature_kernel from the features' own phase; a' = Lk^-1 dk_q, b' = La^-1 dk_q from grad.hip's dK
//     through pred_project) meets the SAME B with beta = 1 on a buffer pre-filled with the mean's Jacobian rows; paths_jac_point_kernel, one
//     workgroup per point, transposes to jac [s][i][d][q] and forms J_s^T J_s and the weighted column sums, d ascending.
// Coordinates: the library works in centred coordinates (gp_ctx::shift).  The features are formed from the centred inputs (x - shift, what
// pred_prep_kernel writes) and the centred centre (c - shift, formed on the host): the same phase, and the same arithmetic for X and for Z.
// Determinism: every product runs on the 128 x 128-tile GEMM kernel without split-k (on_big), whatever the launch size; an element of a product is
// a sum over k in a fixed order that does not depend on its place in the tile, and a feature depends on its row alone.  A point's outputs therefore
// depend on that point, the plan and the model only: the same bits alone, in any batch, in any row order and wherever a chunk boundary falls.  No
// floating-point atomics.  Every buffer belongs to the context's PathsPlan; the evaluation's buffers are only read.
#include "pred_chunk.h"
#include "lane_reduce.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int PF_ROWS = 64;          // rows per workgroup (one wave: lane = row)
constexpr int PF_FB = 64;            // frequencies per workgroup
constexpr int PF_FS = 16;            // frequencies per LDS image
constexpr int PF_LD = PF_FS + 1;     // row stride of the image: lane = row writes, and four rows x 16 columns read, without bank conflicts
constexpr long PATHS_CHUNK_BYTES = 64L << 20;   // left operand of a chunk

struct FeatArgs {
  const double* P;      // [rows][ldp] coordinates (centred inputs, or the centred Z)
  long ldp;
  const double* cen;    // [Q] the centre in the same coordinates
  const double* omega;  // [F][Q]
  int F, Q, Kf;
  long cnt;             // rows >= cnt get zero features
  double scale;         // sqrt(sf2 / F)
  double* out;          // [rows][ldo]: cos in columns [0, F), sin in [F, 2F), zeros in [2F, Kf)
  long ldo;
};

using ConstD = const __attribute__((address_space(4))) double*;

// The phase of a row, one definition for the features and for their derivatives (paths_dfeature_kernel).  QR: compile-time width of the
// coordinates kept in registers (16 or 64, zero-padded); QR = 0 reads them from memory (any Q).
// paths_centre: x_q - c_q of the row pr, the difference first
template <int QR>
__device__ __forceinline__ void paths_centre(const double* pr, const double* cen, int Q, double (&x)[QR > 0 ? QR : 1]) {
  if constexpr (QR > 0) {
#pragma unroll
    for (int q = 0; q < QR; ++q) x[q] = (q < Q) ? pr[q] - cen[q] : 0.0;
  }
}
// paths_phase: theta_f = sum_q omega[f][q] (x_q - c_q), q ascending, one fused multiply-add per term; om = omega[f] is wave-uniform
template <int QR>
__device__ __forceinline__ double paths_phase(const double* om, const double* pr, const double* cen, int Q, const double (&x)[QR > 0 ? QR : 1]) {
  double theta = 0.0;
  if constexpr (QR > 0) {
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q) theta = fma(om[q], x[q], theta);
  } else {
    // omega and the centre are never written while the kernel runs: read through the constant address space, the wave-uniform loads of
    // this run-time loop are scalar loads too (as plain global pointers the compiler gave them a vector offset)
    const ConstD omc = (ConstD)(uintptr_t)om, cenc = (ConstD)(uintptr_t)cen;
    for (int q = 0; q < Q; ++q) theta = fma(omc[q], pr[q] - cenc[q], theta);
  }
  return theta;
}

template <int QR>
__global__ void __launch_bounds__(PF_ROWS) paths_feature_kernel(FeatArgs a) {
  constexpr int QS = QR > 0 ? QR : 1;
  __shared__ double img[2][PF_ROWS * PF_LD];
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * PF_ROWS, row = row0 + lane;
  const bool live = row < a.cnt;
  const double* pr = a.P + (live ? row : 0) * a.ldp;
  double x[QS];
  paths_centre<QR>(pr, a.cen, a.Q, x);
  const int fb = blockIdx.y * PF_FB, fe = min(fb + PF_FB, a.F);
  for (int f0 = fb; f0 < fe; f0 += PF_FS) {
#pragma unroll 1
    for (int k = 0; k < PF_FS; ++k) {
      const int f = min(f0 + k, a.F - 1);                       // wave-uniform: omega comes through scalar loads
      const double theta = paths_phase<QR>(a.omega + (long)f * a.Q, pr, a.cen, a.Q, x);
      double sn, cs;
      sincos(theta, &sn, &cs);
      img[0][lane * PF_LD + k] = live ? a.scale * cs : 0.0;
      img[1][lane * PF_LD + k] = live ? a.scale * sn : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < PF_FS; ++j) {
      const int e = j * PF_ROWS + lane, r = e / PF_FS, k = e % PF_FS, f = f0 + k;
      if (f < a.F) {
        double* o = a.out + (row0 + r) * a.ldo;
        o[f] = img[0][r * PF_LD + k];
        o[a.F + f] = img[1][r * PF_LD + k];
      }
    }
    __syncthreads();
  }
  if (blockIdx.y == 0)
    for (int k = 2 * a.F; k < a.Kf; ++k) a.out[row * a.ldo + k] = 0.0;
}

// ---- the derivative features of gp_paths_grad: d phi / d x_q, one row per (point, q) ----
struct DFeatArgs {
  const double* P;      // [points][Q] centred inputs
  const double* cen;    // [Q] the centre in the same coordinates
  const double* omega;  // [F][Q]
  int F, Q, Kf;
  long cnt;             // points; the rows of a point i >= cnt are zeros
  long rows;            // rows of out, round_up(cnt Q, 128): every one is written in the columns [0, Kf)
  double scale;         // sqrt(sf2 / F)
  double* out;          // [rows][ldo], row i Q + q: -(scale sin theta_f) omega[f][q] in column f < F, (scale cos theta_f) omega[f][q] in F + f, zeros in [2F, Kf)
  long ldo;
};

// One wave per 64 points x 64 frequencies, lane = point for the phases: the same centred difference, the same fused multiply-adds and ONE sincos per
// (point, f) as paths_feature_kernel (paths_centre, paths_phase).  The image [2][64][17] of (scale cos, scale sin) then feeds the output phase, which
// walks (point, q, 16 frequencies): a store instruction covers four (point, q) rows x 16 columns, runs of 128 bytes, and each of the 2 Q values of a
// (point, f) is one rounding of the image's value times omega[f][q] (the sign flip is exact).  The omega tile [16][q] sits in LDS (row stride odd: the
// 16 frequencies of a run land on different banks); QR = 0 (any Q) passes it 64 columns at a time.
template <int QR>
__global__ void __launch_bounds__(PF_ROWS) paths_dfeature_kernel(DFeatArgs a) {
  constexpr int QS = QR > 0 ? QR : 1, OQ = QR > 0 ? QR : 64, OLD = OQ + 1;
  __shared__ double img[2][PF_ROWS * PF_LD];
  __shared__ double omt[PF_FS * OLD];
  const int lane = threadIdx.x, Q = a.Q, F = a.F;
  const long p0 = (long)blockIdx.x * PF_ROWS, pt = p0 + lane;
  const bool live = pt < a.cnt;
  const double* pr = a.P + (live ? pt : 0) * Q;
  double x[QS];
  paths_centre<QR>(pr, a.cen, Q, x);
  const int fb = blockIdx.y * PF_FB, fe = min(fb + PF_FB, F);
  for (int f0 = fb; f0 < fe; f0 += PF_FS) {
#pragma unroll 1
    for (int k = 0; k < PF_FS; ++k) {
      const int f = min(f0 + k, F - 1);                         // wave-uniform: omega comes through scalar loads
      const double theta = paths_phase<QR>(a.omega + (long)f * Q, pr, a.cen, Q, x);
      double sn, cs;
      sincos(theta, &sn, &cs);
      img[0][lane * PF_LD + k] = live ? a.scale * cs : 0.0;
      img[1][lane * PF_LD + k] = live ? a.scale * sn : 0.0;
    }
    for (int q0 = 0; q0 < Q; q0 += OQ) {
      const int nq = min(OQ, Q - q0);
      __syncthreads();                                          // the image is written; the previous omega tile has been consumed
      for (int e = lane; e < PF_FS * nq; e += PF_ROWS) {
        const int k = e / nq, ql = e - k * nq;
        omt[k * OLD + ql] = a.omega[(long)min(f0 + k, F - 1) * Q + q0 + ql];
      }
      __syncthreads();
      for (int e = lane; e < PF_ROWS * PF_FS * nq; e += PF_ROWS) {
        const int k = e % PF_FS, rq = e / PF_FS, r = rq / nq, ql = rq - r * nq, f = f0 + k;
        const long row = (p0 + r) * Q + q0 + ql;
        if (f < F && row < a.rows) {
          const bool on = p0 + r < a.cnt;
          const double w = omt[k * OLD + ql];
          double* o = a.out + row * a.ldo;
          o[f] = on ? -img[1][r * PF_LD + k] * w : 0.0;
          o[F + f] = on ? img[0][r * PF_LD + k] * w : 0.0;
        }
      }
    }
    __syncthreads();                                            // before the next image is written
  }
  const int nz = a.Kf - 2 * F;
  if (blockIdx.y == 0 && nz > 0)
    for (long e = lane; e < (long)PF_ROWS * Q * nz; e += PF_ROWS) {
      const long rq = e / nz, row = p0 * Q + rq;
      if (row < a.rows) a.out[row * a.ldo + 2 * F + (e - rq * nz)] = 0.0;
    }
}

// B rows [0, Kf): Wt[k][s D + d] = w[s][k][d]; rows [Kf + Mp, Kf + 2 Mp): E[m][s D + d] = eps_u[s][m][d]; zeros beyond 2F, M and S D
__global__ void __launch_bounds__(256) paths_pack_kernel(const double* __restrict__ w, const double* __restrict__ eps, int S, int F2, int Kf, int M, int Mp, int D,
                                                         long cols, double* __restrict__ B) {
  const long total = (long)(Kf + Mp) * cols, used = (long)S * D;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long r = e / cols, col = e - r * cols, s = col / D, d = col - s * D;
    if (r < Kf) {
      B[e] = (r < F2 && col < used) ? w[(s * F2 + r) * D + d] : 0.0;
    } else {
      const long m = r - Kf;
      B[(Kf + Mp + m) * cols + col] = (m < M && col < used) ? eps[(s * M + m) * D + d] : 0.0;
    }
  }
}

// T[s][i][d] = C[i][s D + d], i < cnt: the caller's order, one dense block per draw
__global__ void __launch_bounds__(256) paths_scatter_kernel(const double* __restrict__ C, long cnt, int S, int D, long cols, double* __restrict__ T) {
  const long per = cnt * D, total = per * S;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long s = e / per, r = e - s * per, i = r / D, d = r - i * D;
    T[e] = C[i * cols + s * D + d];
  }
}

// ---- gp_paths_grad's contraction: one workgroup per point ----
constexpr int PJ_CG = 64;            // columns d per group
constexpr int PJ_LD = PJ_CG + 1;     // row stride of the tile: the rows of one column, and the columns of one row, land on different banks

struct JacArgs {
  const double* C;      // [(i, q)][cols], column s D + d: d out[s][i][d] / d x_q
  long cols;
  const double* Jm;     // [(i, q)][ldj]: the mean's Jacobian rows, what C was pre-filled with
  long ldj;
  const double* W;      // the weights of grad: [D], or with per_row [S][cnt][D]
  int per_row, S, D, Q;
  long cnt;             // points of the chunk: the outputs are dense [s][cnt]..
  double* jac;          // [S][cnt][D][Q] or NULL
  double* grad;         // [S][cnt][Q] or NULL
  double* metric;       // [S][cnt][Q][Q] or NULL
  double* mean_jac;     // [cnt][D][Q] or NULL
};

// pair p of a symmetric Q x Q matrix, q <= r, row by row: p = r (r + 1) / 2 + q
__device__ __forceinline__ void paths_pair(int p, int& q, int& r) {
  r = 0;
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  q = p - r * (r + 1) / 2;
}

// Pass s = -1 (mean_jac) reads the point's Q rows of Jm, pass s >= 0 its Q rows of C in the columns of draw s; 64 columns d at a time, ascending, go
// through an LDS tile [Q][64] (stride 65).  jac leaves transposed to [d][q] (consecutive threads, consecutive addresses); a thread owns a pair q <= r
// of the Gram J_s^T J_s per 256 (1 for QW = 16, up to 9 for QW = 64) and thread q the weighted column sum of grad: each ONE chain of fused
// multiply-adds over d ascending, so the order is a function of (Q, D) alone.  The metric is mirrored from the same value through the tile.
template <int QW>
__global__ void __launch_bounds__(256) paths_jac_point_kernel(JacArgs a) {
  constexpr int IT = (QW * (QW + 1) / 2 + 255) / 256;
  __shared__ double tile[QW * PJ_LD];
  const int tid = threadIdx.x, Q = a.Q, D = a.D, np = Q * (Q + 1) / 2;
  const long i = blockIdx.x;
  int iq[IT], ir[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    iq[it] = ir[it] = -1;
    if (tid + 256 * it < np) paths_pair(tid + 256 * it, iq[it], ir[it]);
  }
  const bool draws = a.jac || a.grad || a.metric;
  for (int s = a.mean_jac ? -1 : 0; s < (draws ? a.S : 0); ++s) {
    const double* src = s < 0 ? a.Jm + i * Q * a.ldj : a.C + i * Q * a.cols + (long)s * D;
    const long ld = s < 0 ? a.ldj : a.cols, si = (long)s * a.cnt + i;
    double* jo = s < 0 ? a.mean_jac + i * D * Q : a.jac ? a.jac + si * D * Q : nullptr;
    const bool gram = s >= 0 && a.metric;
    const double* w = (s >= 0 && a.grad) ? (a.per_row ? a.W + si * D : a.W) : nullptr;
    double acc[IT], g = 0.0;
#pragma unroll
    for (int it = 0; it < IT; ++it) acc[it] = 0.0;
    for (int c0 = 0; c0 < D; c0 += PJ_CG) {
      const int nd = min(PJ_CG, D - c0);
      __syncthreads();                                           // the previous group (and the previous draw's metric image) has been consumed
      for (int e = tid; e < Q * PJ_CG; e += 256) {
        const int q = e / PJ_CG, c = e - q * PJ_CG;
        if (c < nd) tile[q * PJ_LD + c] = src[(long)q * ld + c0 + c];
      }
      __syncthreads();
      if (jo)
        for (int e = tid; e < nd * Q; e += 256) {
          const int dl = e / Q, q = e - dl * Q;
          jo[(long)c0 * Q + e] = tile[q * PJ_LD + dl];
        }
      if (gram) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
          if (iq[it] >= 0) {
            const double* x = tile + iq[it] * PJ_LD;
            const double* y = tile + ir[it] * PJ_LD;
            double t = acc[it];
            for (int j = 0; j < nd; ++j) t = fma(x[j], y[j], t);
            acc[it] = t;
          }
      }
      if (w && tid < Q) {
        const double* x = tile + tid * PJ_LD;
        for (int j = 0; j < nd; ++j) g = fma(w[c0 + j], x[j], g);
      }
    }
    if (gram) {
      __syncthreads();
#pragma unroll
      for (int it = 0; it < IT; ++it)
        if (iq[it] >= 0) {
          tile[iq[it] * PJ_LD + ir[it]] = acc[it];
          tile[ir[it] * PJ_LD + iq[it]] = acc[it];
        }
      __syncthreads();
      double* mo = a.metric + si * Q * Q;
      for (int e = tid; e < Q * Q; e += 256) {
        const int q = e / Q;
        mo[e] = tile[q * PJ_LD + e - q * Q];
      }
    }
    if (w && tid < Q) a.grad[si * Q + tid] = g;
  }
}

// any Q: jac through a [32 q][64 d] tile; a wave per pair (and per q of grad) reads the rows themselves, a column per lane and 64-column group, the
// lanes summed by a fixed butterfly (grad_point_kernel<0>'s plain path)
template <>
__global__ void __launch_bounds__(256) paths_jac_point_kernel<0>(JacArgs a) {
  __shared__ double tile[32 * PJ_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Q = a.Q, D = a.D, np = Q * (Q + 1) / 2;
  const long i = blockIdx.x;
  const bool draws = a.jac || a.grad || a.metric;
  for (int s = a.mean_jac ? -1 : 0; s < (draws ? a.S : 0); ++s) {
    const double* src = s < 0 ? a.Jm + i * Q * a.ldj : a.C + i * Q * a.cols + (long)s * D;
    const long ld = s < 0 ? a.ldj : a.cols, si = (long)s * a.cnt + i;
    double* jo = s < 0 ? a.mean_jac + i * D * Q : a.jac ? a.jac + si * D * Q : nullptr;
    if (jo)
      for (int q0 = 0; q0 < Q; q0 += 32)
        for (int d0 = 0; d0 < D; d0 += PJ_CG) {
          __syncthreads();
          for (int e = tid; e < 32 * PJ_CG; e += 256) {
            const int ql = e >> 6, dl = e & 63;
            if (q0 + ql < Q && d0 + dl < D) tile[ql * PJ_LD + dl] = src[(long)(q0 + ql) * ld + d0 + dl];
          }
          __syncthreads();
          for (int e = tid; e < 32 * PJ_CG; e += 256) {
            const int dl = e >> 5, ql = e & 31;
            if (q0 + ql < Q && d0 + dl < D) jo[(long)(d0 + dl) * Q + q0 + ql] = tile[ql * PJ_LD + dl];
          }
        }
    if (s < 0) continue;
    if (a.metric) {
      double* mo = a.metric + si * Q * Q;
      for (int p = wave; p < np; p += 4) {
        int q, r;
        paths_pair(p, q, r);
        const double* x = src + (long)q * ld;
        const double* y = src + (long)r * ld;
        double t = 0.0;
        for (int c = lane; c < D; c += 64) t = fma(x[c], y[c], t);
        t = wave_sum(t);
        if (lane == 0) { mo[q * Q + r] = t; mo[r * Q + q] = t; }
      }
    }
    if (a.grad) {
      const double* w = a.per_row ? a.W + si * D : a.W;
      for (int q = wave; q < Q; q += 4) {
        const double* x = src + (long)q * ld;
        double t = 0.0;
        for (int c = lane; c < D; c += 64) t = fma(w[c], x[c], t);
        t = wave_sum(t);
        if (lane == 0) a.grad[si * Q + q] = t;
      }
    }
  }
}

// test hook (gp_debug_set_option "paths_rows"): rows per chunk of gp_paths_eval (any k >= 1: the buffers are padded to 128 rows, a chunk is not);
// 0 = the default below
std::atomic<int> g_opt_paths_rows{0};

// the chunk buffers of gp_paths_eval, cap rows (a multiple of 128): replaced whole when the chunk size grows
struct PathsChunk {
  long cap = 0;
  DevBuf<double> L;           // [cap][Kf + 2 Mp] left operand [phi | a | b]
  DevBuf<double> X;           // [cap][Q] centred inputs
  DevBuf<double> mean;        // [cap][D]
  DevBuf<double> C;           // [cap][cols] mean + the three terms, column s D + d
  DevBuf<double> T;           // [S][cnt][D] the same in the caller's order
};

// the chunk buffers of gp_paths_grad, pts points (rows = round_up(pts Q, 128) rows (point, q)): replaced whole when the chunk size grows
struct PathsGradChunk {
  long pts = 0;
  DevBuf<double> X;           // [round_up(pts, 128)][Q] centred inputs
  DevBuf<double> dK;          // [rows][Mp] d k / d x_q
  DevBuf<double> Jm;          // [rows][Dp] the mean's Jacobian rows
  DevBuf<double> L;           // [rows][Kf + 2 Mp] left operand [dphi_q | a'_q | b'_q]
  DevBuf<double> C;           // [rows][cols] Jm + the three terms, column s D + d
  DevBuf<double> W;           // [D] or [S][cnt][D] the weights of grad
  DevBuf<double> jac;         // [S][cnt][D][Q]
  DevBuf<double> grad;        // [S][cnt][Q]
  DevBuf<double> metric;      // [S][cnt][Q][Q]
  DevBuf<double> mjac;        // [cnt][D][Q]
};

struct PathsPlan {
  int S = 0, F = 0, Kf = 0;
  long cols = 0;              // S D rounded up to 128
  long serial = 0;            // Lifecycle::model_serial() of the global step G was formed from
  DevBuf<double> omega;       // [F][Q]
  DevBuf<double> centre;      // [Q] the centre in centred coordinates (c - shift)
  DevBuf<double> B;           // [Kf + 2 Mp][cols] the packed operand [Wt ; -G ; E]
  std::unique_ptr<PathsChunk> chunk;
  std::unique_ptr<PathsGradChunk> gchunk;
};
void PathsPlanDelete::operator()(PathsPlan* p) const { delete p; }

static int paths_Kf(int F) { return (int)round_up(2L * F, KC); }

long paths_operand_bytes(const gp_ctx* c, int n_draws, int F) {
  return 8L * (paths_Kf(F) + 2L * c->Mp) * round_up((long)n_draws * c->D, TILE);
}

static int launch_features(gp_ctx* c, const double* P, long ldp, const PathsPlan& p, long cnt, long rows, double* out, long ldo) {
  FeatArgs a;
  a.P = P; a.ldp = ldp; a.cen = p.centre; a.omega = p.omega; a.F = p.F; a.Q = c->Q; a.Kf = p.Kf; a.cnt = cnt;
  a.scale = std::sqrt(c->sf2 / p.F); a.out = out; a.ldo = ldo;
  const dim3 grid((unsigned)(rows / PF_ROWS), (unsigned)((p.F + PF_FB - 1) / PF_FB));
  // the latent width the kernel keeps in registers: 16, 64, or (0) a run-time Q beyond
  return for_width<16, 64, 0>(c, "feature kernel", c->Q <= 16 ? 16 : c->Q <= 64 ? 64 : 0,
                              [&](auto W) -> int { GP_LAUNCH(c, c->stream, paths_feature_kernel<W()>, grid, dim3(PF_ROWS), 0, a); return GP_OK; });
}

// The earlier plan is dropped FIRST, so that its operand (up to 2 GiB) is not held next to the new one; the new plan is then built aside and
// published only when complete: a call that fails part way (an allocation, a launch) leaves the context without a plan, never with half of one.
// Every element of the plan's buffers is written before it is read (DA_RAW): Wt and E by paths_pack_kernel, -G by its product, both over the
// padding too.
int run_paths_set(gp_ctx* c, int n_draws, int F, const double* omega, const double* centre, const double* w, const double* eps_u) {
  const long Mp = c->Mp, M = c->M, Q = c->Q, D = c->D, S = n_draws;
  hipStream_t st = c->stream;
  c->paths.reset();
  std::unique_ptr<PathsPlan, PathsPlanDelete> p(new PathsPlan());
  p->S = n_draws; p->F = F; p->Kf = paths_Kf(F); p->cols = round_up(S * D, TILE); p->serial = c->life.model_serial();
  const long Kf = p->Kf, cols = p->cols;
  std::vector<double> cen(Q);
  for (long q = 0; q < Q; ++q) cen[q] = (centre ? centre[q] : 0.0) - c->h_shift[q];
  DevBuf<double> dw, de, PhiZ, T;                      // the caller's normals, Phi_Z [Mp][Kf] and Phi_Z Wt [Mp][cols]: this call's only
  GP_TRY_RC(p->omega.alloc(c, (size_t)(F * Q), DA_RAW)); GP_TRY_RC(p->centre.alloc(c, (size_t)Q, DA_RAW));
  GP_TRY_RC(p->B.alloc(c, (size_t)((Kf + 2 * Mp) * cols), DA_RAW));
  GP_TRY_RC(dw.alloc(c, (size_t)(S * 2 * F * D), DA_RAW)); GP_TRY_RC(de.alloc(c, (size_t)(S * M * D), DA_RAW));
  GP_TRY_RC(PhiZ.alloc(c, (size_t)(Mp * Kf), DA_RAW)); GP_TRY_RC(T.alloc(c, (size_t)(Mp * cols), DA_RAW));
  GP_HIP(c, hipMemcpyAsync(p->omega, omega, p->omega.bytes(), hipMemcpyHostToDevice, st));
  GP_HIP(c, hipMemcpyAsync(p->centre, cen.data(), p->centre.bytes(), hipMemcpyHostToDevice, st));
  GP_HIP(c, hipMemcpyAsync(dw, w, dw.bytes(), hipMemcpyHostToDevice, st));
  GP_HIP(c, hipMemcpyAsync(de, eps_u, de.bytes(), hipMemcpyHostToDevice, st));
  GP_LAUNCH(c, st, paths_pack_kernel, dim3((unsigned)blocks_for((Kf + Mp) * cols)), dim3(256), 0, dw, de, (int)S, 2 * F, (int)Kf, (int)M, (int)Mp, (int)D, cols, p->B);
  GP_TRY_RC(launch_features(c, c->Z, Q, *p, M, Mp, PhiZ, Kf));
  // T = Phi_Z Wt, then -G = -Lk^-1 T into its rows of B: Phi_Z, Lk^-1 [i][k] K_CONTIG, Wt, T [k][column] FREE_CONTIG
  GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)Mp, (int)cols, 1, gemm_of({PhiZ, Kf}, {p->B, cols}, {T, cols}, (int)Kf).on_big(1)));
  GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)Mp, (int)cols, 1,
                        gemm_of({c->gstep.Linv, Mp}, {T, cols}, {p->B + Kf * cols, cols}, (int)Mp, -1.0).on_big(1)));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  c->paths = std::move(p);
  return GP_OK;
}

bool paths_plan_current(gp_ctx* c) {
  if (c->paths && !(c->life.model_current() && c->paths->serial == c->life.model_serial())) c->paths.reset();
  return c->paths != nullptr;
}

int paths_plan_draws(const gp_ctx* c) { return c->paths->S; }

static long paths_rows_for(const gp_ctx* c, const PathsPlan& p, long pred_rows) {
  const int opt = g_opt_paths_rows.load();
  const long dflt = std::max<long>(TILE, PATHS_CHUNK_BYTES / (8L * (p.Kf + 2L * c->Mp)) / TILE * TILE);
  return std::min<long>(opt > 0 ? opt : dflt, pred_rows);       // a chunk goes through gp_predict's chunk buffers
}

int run_paths_eval(gp_ctx* c, long n, const double* X, double* out, double* mean) {
  PathsPlan& p = *c->paths;
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Q = c->Q, D = c->D, S = p.S, Kf = p.Kf, cols = p.cols, ldl = Kf + 2 * Mp;
  PredChunk pc;
  GP_TRY_RC(pred_chunk_open(c, false, &pc));
  const long R = std::min(paths_rows_for(c, p, pc.rows), n), cap = round_up(R, TILE);
  if (!p.chunk || p.chunk->cap < cap) {
    p.chunk.reset();
    auto k = std::make_unique<PathsChunk>();
    auto A = [c](DevBuf<double>& b, long cnt) { return b.alloc(c, (size_t)cnt, DA_RAW); };
    GP_TRY_RC(A(k->L, cap * ldl)); GP_TRY_RC(A(k->X, cap * Q)); GP_TRY_RC(A(k->mean, cap * D)); GP_TRY_RC(A(k->C, cap * cols)); GP_TRY_RC(A(k->T, S * cap * D));
    k->cap = cap;
    p.chunk = std::move(k);
  }
  const PathsChunk& k = *p.chunk;
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0), rows = round_up(cnt, TILE);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), n0, cnt, pred_into(k.X).factors(k.L + Kf, ldl).on_big()));
    GP_TRY_RC(pred_chunk_mean(c, cnt, k.mean));
    GP_TRY_RC(launch_features(c, k.X, Q, p, cnt, rows, k.L, ldl));
    GP_TRY_RC(pred_fill_mean(c, k.mean, cnt, rows, cols, S * D, k.C));
    // C += [phi | a | b] [Wt ; -G ; E]: the left operand [i][k] K_CONTIG, B [k][column] FREE_CONTIG
    GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)rows, (int)cols, 1, gemm_of({k.L, ldl}, {p.B, cols}, {k.C, cols}, (int)ldl, 1.0, 1.0).on_big(1)));
    GP_LAUNCH(c, st, paths_scatter_kernel, dim3((unsigned)blocks_for(S * cnt * D)), dim3(256), 0, k.C, cnt, (int)S, (int)D, cols, k.T);
    GP_HIP(c, hipMemcpy2DAsync(out + n0 * D, (size_t)(n * D) * 8, k.T, (size_t)(cnt * D) * 8, (size_t)(cnt * D) * 8, (size_t)S, hipMemcpyDeviceToHost, st));
    if (mean) GP_HIP(c, hipMemcpyAsync(mean + n0 * D, k.mean, (size_t)(cnt * D) * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

static int launch_dfeatures(gp_ctx* c, const double* P, const PathsPlan& p, long cnt, long rows, double* out, long ldo) {
  DFeatArgs a;
  a.P = P; a.cen = p.centre; a.omega = p.omega; a.F = p.F; a.Q = c->Q; a.Kf = p.Kf; a.cnt = cnt; a.rows = rows;
  a.scale = std::sqrt(c->sf2 / p.F); a.out = out; a.ldo = ldo;
  // the points whose rows reach the last of the padded rows: those beyond cnt write the zeros
  const long cover = (rows + c->Q - 1) / c->Q;
  const dim3 grid((unsigned)((cover + PF_ROWS - 1) / PF_ROWS), (unsigned)((p.F + PF_FB - 1) / PF_FB));
  return for_width<16, 64, 0>(c, "derivative feature kernel", c->Q <= 16 ? 16 : c->Q <= 64 ? 64 : 0,
                              [&](auto W) -> int { GP_LAUNCH(c, c->stream, paths_dfeature_kernel<W()>, grid, dim3(PF_ROWS), 0, a); return GP_OK; });
}

// Derivatives of the draws with respect to the input: the left operand [dphi_q | a'_q | b'_q], one row per (point, q),
// against the plan's B on a buffer pre-filled with the mean's Jacobian rows; paths_jac_point_kernel then forms the requested outputs per point.
// weights: [D], or [S][n][D] with GP_PATHS_WEIGHTS_PER_ROW (flags bit 0).  A call for mean_jac alone runs neither the features nor the product.
int run_paths_grad(gp_ctx* c, long n, const double* X, int flags, const double* weights, double* jac, double* grad, double* metric, double* mean_jac) {
  PathsPlan& p = *c->paths;
  hipStream_t st = c->stream;
  const long Mp = c->Mp, Q = c->Q, D = c->D, Dp = c->Dp, S = p.S, Kf = p.Kf, cols = p.cols, ldl = Kf + 2 * Mp;
  const bool draws = jac || grad || metric, per_row = (flags & 1) != 0;
  PredChunk pc;
  GP_TRY_RC(pred_chunk_open(c, false, &pc));
  const long pts = std::min(std::max<long>(1, paths_rows_for(c, p, pc.rows) / Q), n), cap = round_up(pts * Q, TILE);
  if (!p.gchunk || p.gchunk->pts < pts) {
    p.gchunk.reset();
    auto k = std::make_unique<PathsGradChunk>();
    auto A = [c](DevBuf<double>& b, long cnt) { return b.alloc(c, (size_t)cnt, DA_RAW); };
    GP_TRY_RC(A(k->X, round_up(pts, TILE) * Q)); GP_TRY_RC(A(k->dK, cap * Mp)); GP_TRY_RC(A(k->Jm, cap * Dp)); GP_TRY_RC(A(k->L, cap * ldl));
    GP_TRY_RC(A(k->C, cap * cols)); GP_TRY_RC(A(k->W, std::max(D, S * pts * D))); GP_TRY_RC(A(k->jac, S * pts * D * Q)); GP_TRY_RC(A(k->grad, S * pts * Q));
    GP_TRY_RC(A(k->metric, S * pts * Q * Q)); GP_TRY_RC(A(k->mjac, pts * D * Q));
    k->pts = pts;
    p.gchunk = std::move(k);
  }
  const PathsGradChunk& k = *p.gchunk;
  if (grad && !per_row) GP_HIP(c, hipMemcpyAsync(k.W, weights, (size_t)D * 8, hipMemcpyHostToDevice, st));
  for (long n0 = 0; n0 < n; n0 += pts) {
    const long cnt = std::min(pts, n - n0), rows = round_up(cnt * Q, TILE);
    // the front for the centred inputs and Psi1*: its [a | b] product is not formed (no destination)
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), n0, cnt, pred_into(k.X).on_big()));
    GP_TRY_RC(grad_launch_dk(c, pc.psi1, k.X, cnt, rows, k.dK));
    GP_TRY_RC(pred_project(c, k.dK, rows, {k.Jm, Dp}, {draws ? k.L + Kf : nullptr, ldl}, GEMM_BIG));
    if (draws) {
      GP_TRY_RC(launch_dfeatures(c, k.X, p, cnt, rows, k.L, ldl));
      GP_TRY_RC(pred_fill_rows(c, k.Jm, Dp, cnt * Q, rows, cols, S * D, k.C));
      // C += [dphi_q | a'_q | b'_q] [Wt ; -G ; E]: the left operand [(i, q)][k] K_CONTIG, B [k][column] FREE_CONTIG
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)rows, (int)cols, 1, gemm_of({k.L, ldl}, {p.B, cols}, {k.C, cols}, (int)ldl, 1.0, 1.0).on_big(1)));
      if (grad && per_row)
        GP_HIP(c, hipMemcpy2DAsync(k.W, (size_t)(cnt * D) * 8, weights + n0 * D, (size_t)(n * D) * 8, (size_t)(cnt * D) * 8, (size_t)S, hipMemcpyHostToDevice, st));
    }
    JacArgs a;
    a.C = k.C; a.cols = cols; a.Jm = k.Jm; a.ldj = Dp; a.W = k.W; a.per_row = per_row ? 1 : 0; a.S = (int)S; a.D = (int)D; a.Q = (int)Q; a.cnt = cnt;
    a.jac = jac ? k.jac.get() : nullptr; a.grad = grad ? k.grad.get() : nullptr; a.metric = metric ? k.metric.get() : nullptr;
    a.mean_jac = mean_jac ? k.mjac.get() : nullptr;
    // the rows the contraction's tile holds: 16, 64, or (0) the plain path of any Q
    GP_TRY_RC((for_width<16, 64, 0>(c, "path gradient kernel", Q <= 16 ? 16 : Q <= 64 ? 64 : 0,
                                    [&](auto W) -> int { GP_LAUNCH(c, st, paths_jac_point_kernel<W()>, dim3((unsigned)cnt), dim3(256), 0, a); return GP_OK; })));
    auto down = [&](double* dst, const double* src, long per) {      // [s][cnt][per] of the chunk into [s][n][per] of the caller: S runs
      return hipMemcpy2DAsync(dst + n0 * per, (size_t)(n * per) * 8, src, (size_t)(cnt * per) * 8, (size_t)(cnt * per) * 8, (size_t)S, hipMemcpyDeviceToHost, st);
    };
    if (jac) GP_HIP(c, down(jac, k.jac, D * Q));
    if (grad) GP_HIP(c, down(grad, k.grad, Q));
    if (metric) GP_HIP(c, down(metric, k.metric, Q * Q));
    if (mean_jac) GP_HIP(c, hipMemcpyAsync(mean_jac + n0 * D * Q, k.mjac, (size_t)(cnt * D * Q) * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
