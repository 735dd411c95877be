// Derivatives of the posterior predictive with respect to a new deterministic input (gp_predict_grad), after a global step of this context.
//
// With W = beta E, k_m = psi1_m(x), a = Lk^-1 k, b = La^-1 k (predict.hip) and dk_mq = d k_m / d x_q = -alpha_q (x_q - z_mq) k_m (the difference first,
// on the centred coordinates):
//   jac[d][q]    = sum_m dk_mq W_md                                                        d mean_d / d x_q
//   dvar[q]      = -2 (a . a'_q - b . b'_q),   a'_q = Lk^-1 dk_q,  b'_q = La^-1 dk_q       d var_f / d x_q
//   metric[q][r] = sum_d jac_dq jac_dr + D (sf2 alpha_q [q == r] - a'_q . a'_r + b'_q . b'_r)   E[J^T J] = E[J]^T E[J] + D Cov(J)
//   logdet       = ln det metric                                                           (magnification = exp(logdet / 2))
// Cov(J)_qr is the mixed second derivative of joint.hip's cov_f(x, x') at x = x'; dvar and Cov(J) are in the signed inverse-factor form of DESIGN.md
// sections 11 and 14 (no quadratic form in Ki - P).  The noise enters none of them.
// Per chunk of points:
//   pred_chunk_front (predict.hip, as gp_predict runs it): the centred inputs, Psi1* and the rows [a | b];
//   grad_dk_kernel: the operand dK [(point, q)][Mp], point-major, zero in the columns >= M and in the rows beyond the chunk's last point;
//   two launch_gemm products, T [(point, q)][Dp + 2 Mp] = dK [beta E | Linv^T] = [jac rows | a' | b'];
//   grad_point_kernel: one workgroup per point.  Its Q rows of T and, as one more row, [0 | a | b] form a (Q + 1)-row matrix whose signed Gram (q <= r,
//     the pairs with r == Q being dvar's dot products) is summed 64 columns at a time from an LDS tile (stride 65), a thread per (pair, slice of the 64
//     columns); the slices are added in ascending order.  The jac section leaves transposed through the same tile.  Q <= 64: the metric is
//     factorised in LDS (right-looking Cholesky), logdet = 2 sum ln L_qq in ascending order.  QW = 16, 64: rows the tile holds; QW = 0 (any Q): a wave
//     per pair reads T itself, 128 columns at a time, and sums over its lanes with a fixed butterfly.
// No floating-point atomics, fixed summation order that depends on Q alone: a point's bits do not depend on the batch.  Every buffer belongs to the
// context's GradPlan; the evaluation's and gp_predict's buffers are only read.
// Not covered: uncertain inputs, second derivatives, generating dK inside the GEMM's staging, pinned or pipelined host copies.
#include "pred_chunk.h"
#include "lane_reduce.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int GR_CG = 64;            // columns per group of the staged contraction
constexpr int GR_LD = GR_CG + 1;     // row stride of the tile: the rows of one column, and the columns of one row, land on different banks
constexpr int GR_PG = 128;           // columns per group of the plain path (two per lane)

// dK[(i, q)][m] = -(alpha_q (x_iq - z_mq)) k_im, two columns per thread (16-byte loads and stores)
__global__ void __launch_bounds__(256) grad_dk_kernel(const double* __restrict__ P1, const double* __restrict__ X, const double* __restrict__ Zt,
                                                      const double* __restrict__ alpha, long pts, long rows, int M, int Mp, int Q, double* __restrict__ dK) {
  const long half = Mp / 2, total = rows * half;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long row = e / half;
    const int m = 2 * (int)(e - row * half);
    const long i = row / Q;
    const int q = (int)(row - i * Q);
    double2 v = make_double2(0.0, 0.0);
    if (i < pts && m < M) {
      const double x = X[i * Q + q], aq = alpha[q];
      const double2 k = *reinterpret_cast<const double2*>(P1 + i * Mp + m);
      const double2 z = *reinterpret_cast<const double2*>(Zt + (long)q * Mp + m);
      v.x = -(aq * (x - z.x)) * k.x;
      if (m + 1 < M) v.y = -(aq * (x - z.y)) * k.y;
    }
    *reinterpret_cast<double2*>(dK + row * Mp + m) = v;
  }
}

// the launch of gp_predict_grad and of gp_paths_grad (paths.hip): pts points of X against P1 = Psi1*, rows = round_up(pts Q, 128) rows of dK
int grad_launch_dk(gp_ctx* c, const double* P1, const double* X, long pts, long rows, double* dK) {
  GP_LAUNCH(c, c->stream, grad_dk_kernel, dim3((unsigned)blocks_for(rows * c->Mp / 2)), dim3(256), 0, P1, X, c->Zt, c->alpha, pts, rows, c->M, c->Mp, c->Q, dK);
  return GP_OK;
}

struct GradArgs {
  const double* T;      // [rows][ldt] = [jac rows (Dp) | a' (Mp) | b' (Mp)]
  const double* R;      // [points][2 Mp] rows [a | b]
  const double* alpha;  // [Q]
  long ldt;
  int M, Mp, D, Dp, Q;
  double sf2;
  int need_e, need_l;   // the jac section / the factor sections are present in T
  double* jac;          // [points][D][Q] or NULL
  double* dvar;         // [points][Q] or NULL
  double* metric;       // [points][Q][Q] or NULL
  double* logdet;       // [points] or NULL
  int* fail;            // [points]: 1 where the metric did not factorise (written with logdet)
};

// pair p of the (Q + 1)-row matrix, q <= r, row by row: p = r (r + 1) / 2 + q
__device__ __forceinline__ void grad_pair(int p, int& q, int& r) {
  r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > p) --r;
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  q = p - r * (r + 1) / 2;
}

// slices of a column group for Q: the (pair, slice) items fill the workgroup's IT x 256 slots
__host__ __device__ inline int grad_slices(int Q, int IT) {
  const int np = Q * (Q + 1) / 2 + Q;
  int ns = 8;
  while (ns > 1 && np * ns > 256 * IT) ns >>= 1;
  return ns;
}

template <int QW>
__global__ void __launch_bounds__(256) grad_point_kernel(GradArgs a) {
  constexpr int IT = (QW * (QW + 1) / 2 + QW + 255) / 256;       // items per thread: 1 (QW 16), 9 (QW 64)
  constexpr int TILE_D = (QW + 1) * GR_LD;                        // the tile; later the metric's image [Q][GR_LD]
  __shared__ double sh[TILE_D + 256 * IT];
  double* tile = sh;
  double* red = sh + TILE_D;
  const int tid = threadIdx.x;
  const long i = blockIdx.x;
  const int Q = a.Q, D = a.D, M = a.M;
  const double* Ti = a.T + i * Q * a.ldt;
  const double* Ri = a.R + i * 2L * a.Mp;
  const int np = Q * (Q + 1) / 2 + Q, ns = grad_slices(Q, IT), cs = GR_CG / ns;
  int iq[IT], ir[IT], isl[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int e = tid + 256 * it;
    isl[it] = e / np;
    grad_pair(e - isl[it] * np, iq[it], ir[it]);
    if (e >= np * ns) isl[it] = -1;
  }
  double vj[IT], va[IT], v[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) vj[it] = va[it] = v[it] = 0.0;

  // the three sections of T's columns: jac rows (weight 1), a' (-D), b' (+D); row Q of the tile is 0, a, b
  for (int sec = a.need_e ? 0 : 1; sec < (a.need_l ? 3 : 1); ++sec) {
    const int base = sec == 0 ? 0 : sec == 1 ? a.Dp : a.Dp + a.Mp, len = sec == 0 ? D : M;
    const double* rsec = sec == 0 ? nullptr : Ri + (sec - 1) * a.Mp;
    double s[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) s[it] = 0.0;
    for (int c0 = 0; c0 < len; c0 += GR_CG) {
      __syncthreads();                                           // the previous group has been consumed
      for (int e = tid; e < (Q + 1) * (GR_CG / 2); e += 256) {
        const int r = e / (GR_CG / 2), c = 2 * (e - r * (GR_CG / 2));
        double2 t = make_double2(0.0, 0.0);
        if (c0 + c < len) {
          if (r < Q) t = *reinterpret_cast<const double2*>(Ti + (long)r * a.ldt + base + c0 + c);
          else if (rsec) t = *reinterpret_cast<const double2*>(rsec + c0 + c);
          if (c0 + c + 1 >= len) t.y = 0.0;
        }
        tile[r * GR_LD + c] = t.x;
        tile[r * GR_LD + c + 1] = t.y;
      }
      __syncthreads();
      if (sec == 0 && a.jac) {
        // jac[i][d][q] = T[(i, q)][d]: consecutive threads write consecutive addresses
        const int nd = min(GR_CG, D - c0);
        for (int e = tid; e < nd * Q; e += 256) {
          const int dl = e / Q, q = e - dl * Q;
          a.jac[(i * D + c0) * Q + e] = tile[q * GR_LD + dl];
        }
      }
      if (a.need_l) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          if (isl[it] >= 0) {
            const double* x = tile + iq[it] * GR_LD + isl[it] * cs;
            const double* y = tile + ir[it] * GR_LD + isl[it] * cs;
            double t = s[it];
#pragma unroll 2
            for (int j = 0; j < cs; ++j) t = fma(x[j], y[j], t);
            s[it] = t;
          }
        }
      }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      if (sec == 0) vj[it] = s[it];
      else if (sec == 1) va[it] = s[it];
      else v[it] = s[it] - va[it];
    }
  }
  if (!a.need_l) return;                                         // jac alone (workgroup-uniform)

  // a slice's share of the pair: the metric's S_jac + D (S_b - S_a), dvar's 2 (S_b - S_a); the slices in ascending order
  __syncthreads();
#pragma unroll
  for (int it = 0; it < IT; ++it)
    if (isl[it] >= 0) red[tid + 256 * it] = ir[it] < Q ? fma((double)D, v[it], vj[it]) : 2.0 * v[it];
  __syncthreads();
  double* img = tile;                                            // [Q][GR_LD]: the tile is free
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    if (isl[it] == 0) {
      const int p = tid + 256 * it, q = iq[it], r = ir[it];
      double t = red[p];
      for (int sl = 1; sl < ns; ++sl) t += red[p + sl * np];
      if (r < Q) {
        if (q == r) t += (double)D * (a.sf2 * a.alpha[q]);
        img[q * GR_LD + r] = t;
        img[r * GR_LD + q] = t;
      } else if (a.dvar) {
        a.dvar[i * Q + q] = t;
      }
    }
  }
  __syncthreads();
  if (a.metric)
    for (int e = tid; e < Q * Q; e += 256) {
      const int q = e / Q;
      a.metric[i * Q * Q + e] = img[q * GR_LD + e - q * Q];
    }
  if (!a.logdet) return;
  // right-looking Cholesky of the image's lower triangle; the pivots' logarithms are added in ascending order by thread 0
  double ld = 0.0;
  bool bad = false;
  for (int j = 0; j < Q; ++j) {
    __syncthreads();
    const double d = img[j * GR_LD + j];
    if (!(d > 0.0) || !(d < INFINITY)) { bad = true; break; }   // workgroup-uniform: every thread reads the same pivot
    const double l = sqrt(d);
    ld += log(l);
    for (int r = j + 1 + tid; r < Q; r += 256) img[r * GR_LD + j] /= l;
    __syncthreads();
    const int w = Q - 1 - j;
    for (int e = tid; e < w * w; e += 256) {
      const int r = j + 1 + e / w, c = j + 1 + e % w;
      if (c <= r) img[r * GR_LD + c] = fma(-img[r * GR_LD + j], img[c * GR_LD + j], img[r * GR_LD + c]);
    }
  }
  if (tid == 0) {
    a.logdet[i] = bad ? NAN : 2.0 * ld;
    a.fail[i] = bad ? 1 : 0;
  }
}

// any Q: a wave per pair, two columns per lane and 128-column group, the lanes summed by a fixed butterfly; no factorisation
template <>
__global__ void __launch_bounds__(256) grad_point_kernel<0>(GradArgs a) {
  __shared__ double tile[32 * GR_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long i = blockIdx.x;
  const int Q = a.Q, D = a.D, M = a.M;
  const double* Ti = a.T + i * Q * a.ldt;
  const double* Ri = a.R + i * 2L * a.Mp;
  if (a.jac) {
    // jac[i][d][q] = T[(i, q)][d] through a [32 q][64 d] tile: rows of T read along the columns, runs of 32 q written
    for (int q0 = 0; q0 < Q; q0 += 32)
      for (int d0 = 0; d0 < D; d0 += GR_CG) {
        __syncthreads();
        for (int e = tid; e < 32 * GR_CG; e += 256) {
          const int ql = e >> 6, dl = e & 63;
          if (q0 + ql < Q && d0 + dl < D) tile[ql * GR_LD + dl] = Ti[(long)(q0 + ql) * a.ldt + d0 + dl];
        }
        __syncthreads();
        for (int e = tid; e < 32 * GR_CG; e += 256) {
          const int dl = e >> 5, ql = e & 31;
          if (q0 + ql < Q && d0 + dl < D) a.jac[(i * D + d0 + dl) * Q + q0 + ql] = tile[ql * GR_LD + dl];
        }
      }
  }
  if (!a.need_l) return;
  const int np = Q * (Q + 1) / 2 + Q;
  for (int p = wave; p < np; p += 4) {
    int q, r;
    grad_pair(p, q, r);
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int sec = 0; sec < 3; ++sec) {
      if (sec == 0 && (!a.need_e || r == Q)) continue;
      const int base = sec == 0 ? 0 : sec == 1 ? a.Dp : a.Dp + a.Mp, len = sec == 0 ? D : M;
      const double* x = Ti + (long)q * a.ldt + base;
      const double* y = r < Q ? Ti + (long)r * a.ldt + base : Ri + (sec - 1) * a.Mp;
      double t = 0.0;
      for (int c = 2 * lane; c < len; c += GR_PG) {
        const double2 u = *reinterpret_cast<const double2*>(x + c), w = *reinterpret_cast<const double2*>(y + c);
        t = fma(u.x, w.x, t);
        if (c + 1 < len) t = fma(u.y, w.y, t);
      }
      s[sec] = wave_sum(t);
    }
    if (lane == 0) {
      const double u = s[2] - s[1];
      if (r < Q) {
        double t = fma((double)D, u, s[0]);
        if (q == r) t += (double)D * (a.sf2 * a.alpha[q]);
        if (a.metric) { a.metric[(i * Q + q) * Q + r] = t; a.metric[(i * Q + r) * Q + q] = t; }
      } else if (a.dvar) {
        a.dvar[i * Q + q] = 2.0 * u;
      }
    }
  }
}

// the chunk buffers: pts points per chunk, replaced whole when the chunk size changes
struct GradPlan {
  long pts = 0;
  DevBuf<double> X;           // [round_up(pts, 128)][Q] centred inputs
  DevBuf<double> R;           // [round_up(pts, 128)][2 Mp] [Lk^-1 k | La^-1 k]
  DevBuf<double> dK;          // [rows][Mp], rows = round_up(pts Q, 128)
  DevBuf<double> T;           // [rows][Dp + 2 Mp]
  DevBuf<double> jac;         // [pts][D][Q]
  DevBuf<double> small;       // [pts][Q + Q Q + 1] dvar | metric | logdet
  DevBuf<int> fail;           // [pts]
};
void GradPlanDelete::operator()(GradPlan* p) const { delete p; }

// Built aside and published whole.  Every element is written before it is read (DA_RAW).
static int grad_alloc(gp_ctx* c, long pts) {
  if (c->grad && c->grad->pts == pts) return GP_OK;
  c->grad.reset();
  const long Q = c->Q, Mp = c->Mp, prow = round_up(pts, TILE), rows = round_up(pts * Q, TILE);
  auto A = [c](DevBuf<double>& b, long n) { return b.alloc(c, (size_t)n, DA_RAW); };
  std::unique_ptr<GradPlan, GradPlanDelete> p(new GradPlan());
  GP_TRY_RC(A(p->X, prow * Q)); GP_TRY_RC(A(p->R, prow * 2 * Mp)); GP_TRY_RC(A(p->dK, rows * Mp)); GP_TRY_RC(A(p->T, rows * (c->Dp + 2 * Mp)));
  GP_TRY_RC(A(p->jac, pts * c->D * Q)); GP_TRY_RC(A(p->small, pts * (Q + Q * Q + 1))); GP_TRY_RC(p->fail.alloc(c, (size_t)pts, DA_RAW));
  p->pts = pts;
  c->grad = std::move(p);
  return GP_OK;
}

int run_predict_grad(gp_ctx* c, long n, const double* X, double* jac, double* dvar, double* metric, double* logdet) {
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  const long Q = c->Q, D = c->D, Mp = c->Mp, Dp = c->Dp, ldt = Dp + 2 * Mp;
  const long pts = std::max<long>(1, k.rows / Q);    // <= k.rows: a chunk of points fits gp_predict's chunk; its T has round_up(pts Q, 128) rows
  GP_TRY_RC(grad_alloc(c, pts));
  const GradPlan& p = *c->grad;
  hipStream_t st = c->stream;
  const int need_e = jac || metric || logdet, need_l = dvar || metric || logdet;
  double* o_dvar = p.small;
  double* o_metric = p.small + pts * Q;
  double* o_logdet = p.small + pts * (Q + Q * Q);
  std::vector<int> h_fail(logdet ? (size_t)n : 0);
  for (long n0 = 0; n0 < n; n0 += pts) {
    const long cnt = std::min(pts, n - n0), rows = round_up(cnt * Q, TILE);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), n0, cnt, pred_into(p.X).factors(need_l ? p.R.get() : nullptr, 2 * Mp)));
    GP_TRY_RC(grad_launch_dk(c, k.psi1, p.X, cnt, rows, p.dK));
    GP_TRY_RC(pred_project(c, p.dK, rows, {need_e ? p.T.get() : nullptr, ldt}, {need_l ? p.T + Dp : nullptr, ldt}, GEMM_BY_SIZE));
    GradArgs a;
    a.T = p.T; a.R = p.R; a.alpha = c->alpha; a.ldt = ldt; a.M = c->M; a.Mp = (int)Mp; a.D = (int)D; a.Dp = (int)Dp; a.Q = (int)Q; a.sf2 = c->sf2;
    a.need_e = need_e; a.need_l = need_l;
    a.jac = jac ? p.jac.get() : nullptr; a.dvar = dvar ? o_dvar : nullptr; a.metric = metric ? o_metric : nullptr; a.logdet = logdet ? o_logdet : nullptr;
    a.fail = p.fail;
    // the rows the contraction's tile holds: 16, 64, or (0) the plain path of any Q
    GP_TRY_RC((for_width<16, 64, 0>(c, "predictive gradient kernel", Q <= 16 ? 16 : Q <= 64 ? 64 : 0,
                                    [&](auto W) -> int { GP_LAUNCH(c, st, grad_point_kernel<W()>, dim3((unsigned)cnt), dim3(256), 0, a); return GP_OK; })));
    if (jac) GP_HIP(c, hipMemcpyAsync(jac + n0 * D * Q, p.jac, (size_t)(cnt * D * Q) * 8, hipMemcpyDeviceToHost, st));
    if (dvar) GP_HIP(c, hipMemcpyAsync(dvar + n0 * Q, o_dvar, (size_t)(cnt * Q) * 8, hipMemcpyDeviceToHost, st));
    if (metric) GP_HIP(c, hipMemcpyAsync(metric + n0 * Q * Q, o_metric, (size_t)(cnt * Q * Q) * 8, hipMemcpyDeviceToHost, st));
    if (logdet) {
      GP_HIP(c, hipMemcpyAsync(logdet + n0, o_logdet, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
      GP_HIP(c, hipMemcpyAsync(h_fail.data() + n0, p.fail, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, st));
    }
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  for (size_t k = 0; k < h_fail.size(); ++k)
    if (h_fail[k])
      return fail(c, GP_ERR_NOT_PD, "gp_predict_grad: the metric tensor of point %zu is not positive definite (Cholesky failed); its logdet is NaN", k);
  return GP_OK;
}

}  // namespace gp
