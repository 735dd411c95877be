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
// Coordinates: the library works in centred coordinates (gp_ctx::shift).  The features are formed from the centred inputs (x - shift, what
// pred_prep_kernel writes) and the centred centre (c - shift, formed on the host): the same phase, and the same arithmetic for X and for Z.
// Determinism: every product runs on the 128 x 128-tile GEMM kernel without split-k (on_big), whatever the launch size; an element of a product is
// a sum over k in a fixed order that does not depend on its place in the tile, and a feature depends on its row alone.  A point's outputs therefore
// depend on that point, the plan and the model only: the same bits alone, in any batch, in any row order and wherever a chunk boundary falls.  No
// floating-point atomics.  Every buffer belongs to the context's PathsPlan; the evaluation's buffers are only read.
#include "pred_chunk.h"
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

// QR: compile-time width of the coordinates kept in registers (16 or 64, zero-padded); QR = 0 reads them from memory (any Q)
template <int QR>
__global__ void __launch_bounds__(PF_ROWS) paths_feature_kernel(FeatArgs a) {
  constexpr int QS = QR > 0 ? QR : 1;
  __shared__ double img[2][PF_ROWS * PF_LD];
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * PF_ROWS, row = row0 + lane;
  const bool live = row < a.cnt;
  const double* pr = a.P + (live ? row : 0) * a.ldp;
  double x[QS];
  if constexpr (QR > 0) {
#pragma unroll
    for (int q = 0; q < QR; ++q) x[q] = (q < a.Q) ? pr[q] - a.cen[q] : 0.0;
  }
  const int fb = blockIdx.y * PF_FB, fe = min(fb + PF_FB, a.F);
  for (int f0 = fb; f0 < fe; f0 += PF_FS) {
#pragma unroll 1
    for (int k = 0; k < PF_FS; ++k) {
      const int f = min(f0 + k, a.F - 1);                       // wave-uniform: omega comes through scalar loads
      const double* om = a.omega + (long)f * a.Q;
      double theta = 0.0;
      if constexpr (QR > 0) {
#pragma unroll
        for (int q = 0; q < QR; ++q)
          if (q < a.Q) theta = fma(om[q], x[q], theta);
      } else {
        // omega and the centre are never written while the kernel runs: read through the constant address space, the wave-uniform loads of
        // this run-time loop are scalar loads too (as plain global pointers the compiler gave them a vector offset)
        const ConstD omc = (ConstD)(uintptr_t)om, cenc = (ConstD)(uintptr_t)a.cen;
        for (int q = 0; q < a.Q; ++q) theta = fma(omc[q], pr[q] - cenc[q], theta);
      }
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

struct PathsPlan {
  int S = 0, F = 0, Kf = 0;
  long cols = 0;              // S D rounded up to 128
  long serial = 0;            // Lifecycle::model_serial() of the global step G was formed from
  DevBuf<double> omega;       // [F][Q]
  DevBuf<double> centre;      // [Q] the centre in centred coordinates (c - shift)
  DevBuf<double> B;           // [Kf + 2 Mp][cols] the packed operand [Wt ; -G ; E]
  std::unique_ptr<PathsChunk> chunk;
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

}  // namespace gp
