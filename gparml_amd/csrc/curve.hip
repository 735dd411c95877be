// Expected energy of discrete curves through latent space under the posterior of f, and its gradient (gp_curve_energy), after a global step of this
// context.  Deterministic inputs only.
//
// A curve is T >= 2 points x_0 .. x_{T-1}; segment s joins x_s and x_{s+1}.  With k_s = psi1(x_s), dk_s = k_{s+1} - k_s, dx_s = x_{s+1} - x_s,
// kappa_s = k(x_s, x_{s+1}), W = beta E and [dmu | da | db] = [dk^T W | Lk^-1 dk | La^-1 dk] (predict.hip's products on the differences):
//   seg[s]  = E|f(x_{s+1}) - f(x_s)|^2 = |dmu_s|^2 + D (|db_s|^2 - |da_s|^2) + 2 D (sf2 - kappa_s)
//   energy  = 1/2 (T - 1) sum_s seg[s]                          (1/2 int |c'|^2 dt on [0, 1] with step 1 / (T - 1))
//   g_s     = W dmu_s - D (Lk^-T da_s - La^-T db_s)             (M; g_{-1} = g_{T-1} = 0)
//   grad[t][q] = (T - 1) [ (g_{t-1} - g_t) . dk_t,q + D alpha_q (kappa_{t-1} dx_{t-1,q} - kappa_t dx_{t,q}) ],  dk_t,q = -alpha_q (x_tq - z_q) o k_t
// joint.hip's covariance differenced twice, in the signed inverse-factor form of DESIGN.md sections 11 and 14 (nothing forms Ki - P).  The two
// differences that would cancel on a fine curve are never formed as differences of exponentials:
//   dk_sm          = k_base,m expm1(-1/2 sum_q alpha_q dx_sq ((x_sq - z_mq) + (x_{s+1,q} - z_mq)))   base = the endpoint with the larger k_m (argument <= 0)
//   sf2 - kappa_s  = -sf2 expm1(-1/2 sum_q alpha_q dx_sq^2)
// and dx is the difference of the inputs as given (the centred coordinates of DESIGN.md section 13 serve x - z only), so a repeated point gives
// seg = 0 exactly.
// Per chunk of whole curves:
//   pred_chunk_front (predict.hip, as gp_predict runs it) over the chunk's points: the centred inputs and Psi1*;
//   curve_dk_kernel: dK [segment][Mp], zero in the columns >= M and in the rows beyond the chunk's last segment, and [sf2 - kappa | kappa] per segment;
//   two launch_gemm products, Tm [segment][Dp + 2 Mp] = dK [beta E | Linv^T] = [dmu | da | db];
//   curve_seg_kernel: a wave per segment, the three sections summed separately (fixed butterfly), the prior term added last;
//   curve_sum_kernel: a thread per curve, the segments in ascending order;
//   the gradient only: three launch_gemm products G [segment][Mp] = beta dmu E^T - D da Lk^-1 + D db La^-1, then curve_grad_kernel, a wave per point:
//     sum_m (g_{t-1} - g_t)_m k_tm (x_tq - z_mq) over its lanes by a fixed butterfly, QW latent dimensions at a time in registers (QW = 16, 64; 0: one
//     at a time, any Q), the kappa terms added last.
// Every product runs on the 128 x 128-tile GEMM kernel without split-k whatever the launch size (on_big, as paths.hip), so a curve's bits are the same
// alone, in any batch and on either side of a chunk boundary.  No floating-point atomics; the summation order depends on (M, Q, D, T) alone.  Every
// buffer belongs to the context's CurvePlan; the evaluation's and gp_predict's buffers are only read.
// Not covered: uncertain inputs, second derivatives, generating dK inside the GEMM's staging, results kept on the device.
#include "pred_chunk.h"
#include "lane_reduce.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int CV_PG = 128;           // columns per group of the row kernels (two per lane)

// dK[s][m] in the expm1 form, two columns per thread (16-byte loads and stores); the thread of column 0 also writes kap[s] = [sf2 - kappa | kappa]
__global__ void __launch_bounds__(256) curve_dk_kernel(const double* __restrict__ P1, const double* __restrict__ Xc, const double* __restrict__ Xr,
                                                       const double* __restrict__ Zt, const double* __restrict__ alpha, long nseg, long rows, int T, int M, int Mp,
                                                       int Q, double sf2, double* __restrict__ dK, double* __restrict__ kap) {
  const long half = Mp / 2, total = rows * half;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long row = e / half;
    const int m = 2 * (int)(e - row * half);
    double2 v = make_double2(0.0, 0.0);
    if (row < nseg) {
      const long i = row + row / (T - 1);                        // the segment's first point: curve * T + s
      const double* x0 = Xc + i * Q;
      const double* r0 = Xr + i * Q;
      if (m < M) {
        double ux = 0.0, uy = 0.0;
        for (int q = 0; q < Q; ++q) {
          const double w = alpha[q] * (r0[Q + q] - r0[q]);
          const double2 z = *reinterpret_cast<const double2*>(Zt + (long)q * Mp + m);
          ux = fma(w, (x0[q] - z.x) + (x0[Q + q] - z.x), ux);
          uy = fma(w, (x0[q] - z.y) + (x0[Q + q] - z.y), uy);
        }
        const double2 k0 = *reinterpret_cast<const double2*>(P1 + i * Mp + m);
        const double2 k1 = *reinterpret_cast<const double2*>(P1 + (i + 1) * Mp + m);
        // k_{s+1} / k_s = exp(-u / 2): u >= 0 the first point is the base, else the second and the result changes sign
        const double ex = (ux >= 0.0 ? k0.x : k1.x) * expm1(-0.5 * fabs(ux));
        const double ey = (uy >= 0.0 ? k0.y : k1.y) * expm1(-0.5 * fabs(uy));
        v.x = ux >= 0.0 ? ex : -ex;
        if (m + 1 < M) v.y = uy >= 0.0 ? ey : -ey;
      }
      if (m == 0) {
        double u = 0.0;
        for (int q = 0; q < Q; ++q) {
          const double d = r0[Q + q] - r0[q];
          u = fma(alpha[q] * d, d, u);
        }
        *reinterpret_cast<double2*>(kap + 2 * row) = make_double2(-(sf2 * expm1(-0.5 * u)), sf2 * exp(-0.5 * u));
      }
    }
    *reinterpret_cast<double2*>(dK + row * Mp + m) = v;
  }
}

// sum of squares of x[0 .. len) over the wave: two columns per lane and 128-column group, then the butterfly
__device__ __forceinline__ double curve_sumsq(const double* __restrict__ x, int len, int lane) {
  double t = 0.0;
  for (int c = 2 * lane; c < len; c += CV_PG) {
    const double2 u = *reinterpret_cast<const double2*>(x + c);
    t = fma(u.x, u.x, t);
    if (c + 1 < len) t = fma(u.y, u.y, t);
  }
  return wave_sum(t);
}

// seg[s] = |dmu|^2 + D (|db|^2 - |da|^2) + 2 D (sf2 - kappa): one wave per row of Tm
__global__ void __launch_bounds__(256) curve_seg_kernel(const double* __restrict__ Tm, long ldt, const double* __restrict__ kap, long nseg, int M, int Mp, int D,
                                                        int Dp, double* __restrict__ seg) {
  const int lane = threadIdx.x & 63;
  const long s = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (s >= nseg) return;
  const double* t = Tm + s * ldt;
  const double smu = curve_sumsq(t, D, lane), sa = curve_sumsq(t + Dp, M, lane), sb = curve_sumsq(t + Dp + Mp, M, lane);
  if (lane == 0) seg[s] = fma((double)D, sb - sa, smu) + 2.0 * D * kap[2 * s];
}

// energy[c] = 1/2 (T - 1) sum_s seg[c][s], s ascending
__global__ void __launch_bounds__(256) curve_sum_kernel(const double* __restrict__ seg, long curves, int T, double* __restrict__ energy) {
  const long c = blockIdx.x * 256L + threadIdx.x;
  if (c >= curves) return;
  const double* s = seg + c * (T - 1);
  double t = 0.0;
  for (int j = 0; j < T - 1; ++j) t += s[j];
  energy[c] = 0.5 * (T - 1) * t;
}

struct CurveGradArgs {
  const double* G;      // [segments][Mp]
  const double* P1;     // [points][Mp]
  const double* Xc;     // [points][Q] centred inputs
  const double* Xr;     // [points][Q] inputs as given
  const double* Zt;     // [Q][Mp]
  const double* alpha;  // [Q]
  const double* kap;    // [segments][2]
  long pts;
  int T, M, Mp, Q, D;
  double* grad;         // [points][Q]
};

// one wave per point; QW latent dimensions at a time in registers (0: one)
template <int QW>
__global__ void __launch_bounds__(256) curve_grad_kernel(CurveGradArgs a) {
  constexpr int QB = QW > 0 ? QW : 1;
  const int lane = threadIdx.x & 63;
  const long i = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (i >= a.pts) return;                                        // wave-uniform
  const int T = a.T, M = a.M, Mp = a.Mp, Q = a.Q;
  const long cu = i / T, s = i - cu;                             // s: the segment that starts at this point (the one before it ends here)
  const int t = (int)(i - cu * T);
  const double* gm = t > 0 ? a.G + (s - 1) * Mp : nullptr;
  const double* gp = t < T - 1 ? a.G + s * Mp : nullptr;
  const double* k = a.P1 + i * Mp;
  const double* x = a.Xc + i * Q;
  const double* r = a.Xr + i * Q;
  for (int q0 = 0; q0 < Q; q0 += QB) {
    double acc[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) acc[j] = 0.0;
    for (int c = 2 * lane; c < M; c += CV_PG) {
      double2 h = make_double2(0.0, 0.0);
      if (gm) h = *reinterpret_cast<const double2*>(gm + c);
      if (gp) {
        const double2 g = *reinterpret_cast<const double2*>(gp + c);
        h.x -= g.x;
        h.y -= g.y;
      }
      const double2 kk = *reinterpret_cast<const double2*>(k + c);
      const double hx = h.x * kk.x, hy = c + 1 < M ? h.y * kk.y : 0.0;
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        if (QW == 0 || q0 + j < Q) {
          const double2 z = *reinterpret_cast<const double2*>(a.Zt + (long)(q0 + j) * Mp + c);
          const double xq = x[q0 + j];
          acc[j] = fma(hy, xq - z.y, fma(hx, xq - z.x, acc[j]));
        }
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      const double w = wave_sum(acc[j]);
      if (lane == j) mine = w;
    }
    const int q = q0 + lane;
    if (lane < QB && q < Q) {
      const double aq = a.alpha[q];
      double kt = 0.0;                                           // kappa_{t-1} dx_{t-1,q} - kappa_t dx_{t,q}
      if (t > 0) kt = a.kap[2 * (s - 1) + 1] * (r[q] - r[q - Q]);
      if (t < T - 1) kt -= a.kap[2 * s + 1] * (r[Q + q] - r[q]);
      a.grad[i * Q + q] = (double)(T - 1) * (-(aq * mine) + (double)a.D * aq * kt);
    }
  }
}

// test hook (gp_debug_set_option "curve_curves"): at most this many curves per chunk; 0 = the default, what gp_predict's chunk holds
std::atomic<int> g_opt_curve_curves{0};

// the chunk buffers: curves curves of T points per chunk, replaced whole when either changes
struct CurvePlan {
  long curves = 0;
  int T = 0;
  DevBuf<double> X;           // [round_up(points, 128)][Q] centred inputs
  DevBuf<double> dK;          // [rows][Mp], rows = round_up(curves (T - 1), 128)
  DevBuf<double> Tm;          // [rows][Dp + 2 Mp]
  DevBuf<double> G;           // [rows][Mp]
  DevBuf<double> kap;         // [rows][2] sf2 - kappa | kappa
  DevBuf<double> seg;         // [curves (T - 1)]
  DevBuf<double> energy;      // [curves]
  DevBuf<double> grad;        // [points][Q]
};
void CurvePlanDelete::operator()(CurvePlan* p) const { delete p; }

// Built aside and published whole.  Every element is written before it is read (DA_RAW).
static int curve_alloc(gp_ctx* c, long curves, int T) {
  if (c->curve && c->curve->curves == curves && c->curve->T == T) return GP_OK;
  c->curve.reset();
  const long Q = c->Q, Mp = c->Mp, pts = curves * T, rows = round_up(curves * (T - 1), TILE);
  auto A = [c](DevBuf<double>& b, long n) { return b.alloc(c, (size_t)n, DA_RAW); };
  std::unique_ptr<CurvePlan, CurvePlanDelete> p(new CurvePlan());
  GP_TRY_RC(A(p->X, round_up(pts, TILE) * Q)); GP_TRY_RC(A(p->dK, rows * Mp)); GP_TRY_RC(A(p->Tm, rows * (c->Dp + 2 * Mp))); GP_TRY_RC(A(p->G, rows * Mp));
  GP_TRY_RC(A(p->kap, rows * 2)); GP_TRY_RC(A(p->seg, curves * (T - 1))); GP_TRY_RC(A(p->energy, curves)); GP_TRY_RC(A(p->grad, pts * Q));
  p->curves = curves;
  p->T = T;
  c->curve = std::move(p);
  return GP_OK;
}

int run_curve_energy(gp_ctx* c, long n, int T, const double* X, double* energy, double* seg, double* grad) {
  PredChunk k;
  GP_TRY_RC(pred_chunk_open(c, false, &k));
  if (T > k.rows)
    return fail(c, GP_ERR_UNSUPPORTED, "gp_curve_energy: a curve of T = %d points exceeds the %ld points of one chunk (chunks hold whole curves): split the curve", T, k.rows);
  const int opt = g_opt_curve_curves.load();
  long per = std::max<long>(1, k.rows / T);           // per T <= k.rows: a chunk of curves fits gp_predict's chunk
  if (opt > 0) per = std::min<long>(per, opt);
  GP_TRY_RC(curve_alloc(c, per, T));
  const CurvePlan& p = *c->curve;
  hipStream_t st = c->stream;
  const long Q = c->Q, Mp = c->Mp, Dp = c->Dp, ldt = Dp + 2 * Mp;
  const double D = c->D;
  for (long c0 = 0; c0 < n; c0 += per) {
    const long nc = std::min(per, n - c0), cnt = nc * T, nseg = nc * (T - 1), rows = round_up(nseg, TILE);
    GP_TRY_RC(pred_chunk_front(c, pred_at(X), c0 * T, cnt, pred_into(p.X).on_big()));
    GP_LAUNCH(c, st, curve_dk_kernel, dim3((unsigned)blocks_for(rows * Mp / 2)), dim3(256), 0, k.psi1, p.X, k.inputs, c->Zt, c->alpha, nseg, rows,
              T, c->M, (int)Mp, (int)Q, c->sf2, p.dK, p.kap);
    GP_TRY_RC(pred_project(c, p.dK, rows, {p.Tm, ldt}, {p.Tm + Dp, ldt}, GEMM_BIG));
    if (energy || seg)
      GP_LAUNCH(c, st, curve_seg_kernel, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, p.Tm, ldt, p.kap, nseg, c->M, (int)Mp, c->D, (int)Dp, p.seg);
    if (energy) GP_LAUNCH(c, st, curve_sum_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, p.seg, nc, T, p.energy);
    if (grad) {
      // g = W dmu - D Lk^-T da + D La^-T db: the transposed operands of the forward products, the factor terms with their signs
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, K_CONTIG, (int)rows, (int)Mp, 1, gemm_of({p.Tm, ldt}, {c->gstep.E, Dp}, {p.G, Mp}, (int)Dp, c->beta).on_big(1)));
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)rows, (int)Mp, 1, gemm_of({p.Tm + Dp, ldt}, {c->gstep.Linv, Mp}, {p.G, Mp}, (int)Mp, -D, 1.0).on_big(1)));
      GP_TRY_RC(launch_gemm(c, st, K_CONTIG, FREE_CONTIG, (int)rows, (int)Mp, 1,
                            gemm_of({p.Tm + Dp + Mp, ldt}, {c->gstep.Linv + Mp * Mp, Mp}, {p.G, Mp}, (int)Mp, D, 1.0).on_big(1)));
      CurveGradArgs a;
      a.G = p.G; a.P1 = k.psi1; a.Xc = p.X; a.Xr = k.inputs; a.Zt = c->Zt; a.alpha = c->alpha; a.kap = p.kap; a.pts = cnt;
      a.T = T; a.M = c->M; a.Mp = (int)Mp; a.Q = (int)Q; a.D = c->D; a.grad = p.grad;
      // the latent dimensions a wave keeps in registers: 16, 64, or (0) one at a time for any Q
      GP_TRY_RC((for_width<16, 64, 0>(c, "curve gradient kernel", Q <= 16 ? 16 : Q <= 64 ? 64 : 0, [&](auto W) -> int {
        GP_LAUNCH(c, st, curve_grad_kernel<W()>, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, a);
        return GP_OK;
      })));
      GP_HIP(c, hipMemcpyAsync(grad + c0 * T * Q, p.grad, (size_t)(cnt * Q) * 8, hipMemcpyDeviceToHost, st));
    }
    if (energy) GP_HIP(c, hipMemcpyAsync(energy + c0, p.energy, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
    if (seg) GP_HIP(c, hipMemcpyAsync(seg + c0 * (T - 1), p.seg, (size_t)nseg * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
