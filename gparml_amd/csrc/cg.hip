// The resident CG / GD vectors (gp_cg_*): grad_latest, grad_new, grad_old and the search direction stay in HBM next to the embeddings they move
// (scg_adapted_local_MapReduce.py:29-243, gd_local_MapReduce.py:38-61).  gp_phase2 with embedding gradients writes grad_latest (api.hip).
#include "gp_common.h"
#include "lane_reduce.h"
#include "varpoint.h"
#include <cmath>

using namespace gp;

int gp::CgState::alloc(gp_ctx* c) {
  for (DevBuf<double>* b : {&g_latest, &g_new, &g_old}) GP_TRY_RC(b->alloc(c, (size_t)2 * c->N * c->Q));
  return GP_OK;
}

int gp::resident_ready(gp_ctx* c, const char* who, const char* what) {
  if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "%s: no shard data", who);
  if (!c->xs_raw) return fail(c, GP_ERR_STATE, "%s: the %s only for free embeddings (raw variances)", who, what);
  return GP_OK;
}
static int cg_ready(gp_ctx* c, const char* who) { return resident_ready(c, who, "resident CG vectors exist"); }

// which: 0 d = -g_new (reset_d :160-173) | 1 d = a*d - g_new (update_d :175-189) | 2 X += a*d (update_X :191-214)
//        3 g_old = g_new (:216-229) | 4 g_new = g_latest (:231-243) | 5 set_grads: g_new = g_old = g_latest, d = -g_latest (:29-55)
__global__ void cg_update_kernel(int which, double a, long nq, double* __restrict__ d, double* __restrict__ gnew, double* __restrict__ gold,
                                 const double* __restrict__ glatest, double* __restrict__ Xmu, double* __restrict__ Xs) {
  const long n2 = 2 * nq;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n2; i += (long)gridDim.x * 256L) {
    switch (which) {
      case 0: d[i] = -gnew[i]; break;
      case 1: d[i] = mul_then_add(a, d[i], -gnew[i]); break;
      case 2: if (i < nq) Xmu[i] = mul_then_add(a, d[i], Xmu[i]); else Xs[i - nq] = mul_then_add(a, d[i], Xs[i - nq]); break;
      case 3: gold[i] = gnew[i]; break;
      case 4: gnew[i] = glatest[i]; break;
      default: { const double g = glatest[i]; gnew[i] = g; gold[i] = g; d[i] = -g; } break;
    }
  }
}
// out[0..4] += (g_new.d, d.d, d.(g_latest - g_new), g_new.g_new, g_new.g_old); out[5] = max(out[5], max |d|)
// The five sums are COMPENSATED (Ogita, Rump, Oishi: Dot2): every product's and every addition's rounding error is kept in a second accumulator,
// through the thread's loop and the block fold alike, and added once at the end.  The order of the additions is unchanged (a thread's terms in
// ascending order, block_fold<256>, the blocks in ascending order on the host); the result is the sum as if formed in twice the precision, so the
// optimiser's alpha and Gamma, which cancel, do not depend on that order beyond the last bits.
struct TwoSum { double s, e; };
__host__ __device__ __forceinline__ TwoSum two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double t = a + b, z = t - a;
  return TwoSum{t, (a - (t - z)) + (b - z)};
}
__device__ __forceinline__ void dot2_step(double x, double y, double& s, double& c) {
#pragma clang fp contract(off)
  const double p = x * y;
  const double pe = __builtin_fma(x, y, -p);
  const TwoSum t = two_sum(s, p);
  s = t.s;
  c += pe + t.e;
}
__global__ void __launch_bounds__(256) cg_dots_kernel(long n2, const double* __restrict__ d, const double* __restrict__ gnew,
                                                      const double* __restrict__ gold, const double* __restrict__ glatest, double* part) {
  __shared__ double red[6][256];
  __shared__ double cmp[5][256];
  double s[6] = {0, 0, 0, 0, 0, 0}, c[5] = {0, 0, 0, 0, 0};
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n2; i += (long)gridDim.x * 256L) {
    const double di = d[i], gn = gnew[i];
    dot2_step(gn, di, s[0], c[0]); dot2_step(di, di, s[1], c[1]); dot2_step(di, glatest[i] - gn, s[2], c[2]);
    dot2_step(gn, gn, s[3], c[3]); dot2_step(gn, gold[i], s[4], c[4]);
    s[5] = fmax(s[5], fabs(di));
  }
  for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = s[k];
  for (int k = 0; k < 5; ++k) cmp[k][threadIdx.x] = c[k];
  __syncthreads();
  block_fold<256>([&](int i, int j) {
    for (int k = 0; k < 5; ++k) {
      const TwoSum t = two_sum(red[k][i], red[k][j]);
      red[k][i] = t.s;
      cmp[k][i] += cmp[k][j] + t.e;
    }
    red[5][i] = fmax(red[5][i], red[5][j]);
  });
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0] + (threadIdx.x < 5 ? cmp[threadIdx.x][0] : 0.0);
}
// out[0] += sum |g_new| ; out[1] = max |g_new|   (gd_local_MapReduce.py:38-61)
__global__ void __launch_bounds__(256) cg_abs_kernel(long n2, const double* __restrict__ gnew, double* part) {
  __shared__ double red[2][256];
  double s = 0.0, m = 0.0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n2; i += (long)gridDim.x * 256L) { const double a = fabs(gnew[i]); s += a; m = fmax(m, a); }
  red[0][threadIdx.x] = s; red[1][threadIdx.x] = m;
  __syncthreads();
  block_fold<256>([&](int i, int j) { red[0][i] += red[0][j]; red[1][i] = fmax(red[1][i], red[1][j]); });
  if (threadIdx.x < 2) part[blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0];
}

extern "C" int gp_cg_update(gp_ctx* c, int which, double a) {
  if (!c) return GP_ERR_BAD_ARG;
  if (which < 0 || which > 5) return fail(c, GP_ERR_BAD_ARG, "gp_cg_update: which must be 0..5");
  GP_TRY_RC(cg_ready(c, "gp_cg_update"));
  if ((which == 4 || which == 5) && !c->life.has_grad_latest()) return fail(c, GP_ERR_STATE, "gp_cg_update: no grad_latest yet (gp_phase2(ctx, 1) first)");
  GP_HIP(c, hipSetDevice(c->device));
  const long nq = (long)c->N * c->Q;
  GP_LAUNCH(c, c->stream, cg_update_kernel, dim3(blocks_for(2 * nq)), dim3(256), 0, which, a, nq, c->dir, c->cg.g_new, c->cg.g_old, c->cg.g_latest,
            c->Xmu, c->Xs);
  if (which == 0 || which == 1 || which == 5) c->life.direction_rewritten();
  if (which == 2) c->life.embeddings_changed();
  return GP_OK;
}

extern "C" int gp_cg_set_grads(gp_ctx* c) { return gp_cg_update(c, 5, 0.0); }

// The host half of both reductions over the 2 N Q elements: cg_dots_kernel (width 6) or cg_abs_kernel (width 2) writes a row of partials per block
// into c->red; h receives them [blocks][width] once the stream has been synchronised, for the caller's fold in ascending block order
static int cg_partials(gp_ctx* c, int width, std::vector<double>& h) {
  const long n2 = 2L * c->N * c->Q;
  const int nb = std::min(blocks_for(n2), 1024);
  if (width == 6) GP_LAUNCH(c, c->stream, cg_dots_kernel, dim3(nb), dim3(256), 0, n2, c->dir, c->cg.g_new, c->cg.g_old, c->cg.g_latest, c->red);
  else GP_LAUNCH(c, c->stream, cg_abs_kernel, dim3(nb), dim3(256), 0, n2, c->cg.g_new, c->red);
  h.resize((size_t)nb * width);
  GP_HIP(c, hipMemcpyAsync(h.data(), c->red, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  return GP_OK;
}

static int cg_reduce(gp_ctx* c, double* out6) {
  std::vector<double> h;
  GP_TRY_RC(cg_partials(c, 6, h));
  double comp[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 6; ++k) out6[k] = 0.0;
  for (size_t b = 0; b < h.size(); b += 6) {
    for (int k = 0; k < 5; ++k) { const TwoSum t = two_sum(out6[k], h[b + k]); out6[k] = t.s; comp[k] += t.e; }
    out6[5] = std::max(out6[5], h[b + 5]);
  }
  for (int k = 0; k < 5; ++k) out6[k] += comp[k];
  return GP_OK;
}

extern "C" int gp_cg_dots(gp_ctx* c, double* out6) {
  if (!c || !out6) return GP_ERR_BAD_ARG;
  GP_TRY_RC(cg_ready(c, "gp_cg_dots"));
  if (!c->life.has_direction()) return fail(c, GP_ERR_STATE, "gp_cg_dots: no search direction (gp_cg_set_grads first)");
  GP_HIP(c, hipSetDevice(c->device));
  return cg_reduce(c, out6);
}

extern "C" int gp_cg_abs(gp_ctx* c, double* out2) {
  if (!c || !out2) return GP_ERR_BAD_ARG;
  GP_TRY_RC(cg_ready(c, "gp_cg_abs"));
  if (!c->life.has_direction()) return fail(c, GP_ERR_STATE, "gp_cg_abs: no gradient vectors (gp_cg_set_grads first)");
  GP_HIP(c, hipSetDevice(c->device));
  std::vector<double> h;
  GP_TRY_RC(cg_partials(c, 2, h));
  out2[0] = 0.0; out2[1] = 0.0;
  for (size_t b = 0; b < h.size(); b += 2) { out2[0] += h[b]; out2[1] = std::max(out2[1], h[b + 1]); }
  return GP_OK;
}

extern "C" int gp_cg_max_d(gp_ctx* c, double alpha, double* out) {
  if (!c || !out) return GP_ERR_BAD_ARG;
  GP_TRY_RC(cg_ready(c, "gp_cg_max_d"));
  if (!c->life.has_direction()) return fail(c, GP_ERR_STATE, "gp_cg_max_d: no search direction (gp_cg_set_grads first)");
  GP_HIP(c, hipSetDevice(c->device));
  double o[6];
  GP_TRY_RC(cg_reduce(c, o));
  *out = std::fabs(alpha) * o[5];
  return GP_OK;
}
