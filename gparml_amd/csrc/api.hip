// extern "C" entry points of libgparml_hip.so (see include/gparml_hip.h).
#include "gp_common.h"
#include "lane_reduce.h"
#include "varpoint.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <limits>

namespace gp {
thread_local std::string g_create_error;

int fail(gp_ctx* ctx, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf; else g_create_error = buf;
  return code;
}

hipStream_t ctx_stream(const gp_ctx* c) { return c ? c->stream : nullptr; }

std::atomic<int> g_opt_poison{env_flag("GPARML_POISON", false)};
std::atomic<int> g_alloc_fail_after{0};
#define GP_TRY(x) do { int rc__ = (x); if (rc__ != GP_OK) return rc__; } while (0)

__global__ void sumsq_kernel(const double* __restrict__ x, long n, double* part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) s += x[i] * x[i];
  const double tot = block_sum<256>(red, s);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// gather a padded device matrix [rows_p][ld] into a dense host-shaped [rows][cols] staging buffer
__global__ void gather2d_kernel(const double* __restrict__ src, long ld, long rows, long cols, double* __restrict__ dst) {
  const long total = rows * cols;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const long r = i / cols, c = i - r * cols;
    dst[i] = src[r * ld + c];
  }
}
__global__ void scatter2d_kernel(const double* __restrict__ src, long rows, long cols, double* __restrict__ dst, long ld, long rows_p, long cols_p) {
  const long total = rows_p * cols_p;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const long r = i / cols_p, c = i - r * cols_p;
    dst[r * ld + c] = (r < rows && c < cols) ? src[r * cols + c] : 0.0;
  }
}
__global__ void scale_kernel(double* x, long n, double f) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) x[i] *= f;
}
// Zaug[m] = [1, z_m, z_m^2] (rows >= M zero), Z padded copy
// Zin / alpha_in are read straight from the pinned host slot of gp_set_globals (mapped memory: M Q + Q doubles over the bus, no copy commands)
__global__ void __launch_bounds__(256) zaug_kernel(const double* __restrict__ Zin, const double* __restrict__ alpha_in, int M, int Mp, int Q, int CZp,
                                                   double* __restrict__ Z, double* __restrict__ Zaug, double* __restrict__ alpha, double* __restrict__ Zt) {
  // one element of Zaug per thread (r05): every read of the mapped host slot is its own bus round trip, and the first form -- one thread per inducing point
  // walking its Q coordinates -- made them one after the other (8.8 us at M = 128, Q = 10; 28 us at M = 1024, Q = 50)
  const long total = (long)Mp * CZp;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int m = (int)(e / CZp), c = (int)(e - (long)m * CZp);
    if (e < Q) alpha[e] = alpha_in[e];
    double v = 0.0;
    if (c == 0) v = (m < M) ? 1.0 : 0.0;
    else if (c <= 2 * Q) {
      const int q = (c <= Q) ? c - 1 : c - 1 - Q;
      const double z = (m < M) ? Zin[(long)m * Q + q] : 0.0;
      if (c <= Q) { Z[(long)m * Q + q] = z; Zt[(long)q * Mp + m] = z; v = z; }
      else v = z * z;
    }
    Zaug[e] = v;
  }
}

static int download_matrix(gp_ctx* c, const double* src, long ld, long rows, long cols, double* dst, int64_t n) {
  if (n != rows * cols) return fail(c, GP_ERR_BAD_ARG, "gp_download: expected %ld doubles, got %ld", rows * cols, (long)n);
  DevBuf<double> tmp;
  GP_TRY(tmp.alloc(c, rows * cols, DA_RAW));
  GP_LAUNCH(c, c->stream, gather2d_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, src, ld, rows, cols, tmp);
  hipError_t e = hipMemcpyAsync(dst, tmp, rows * cols * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, GP_ERR_HIP, "download failed: %s", hipGetErrorString(e));
  return GP_OK;
}

// The shared workspace's capacity, a function of the shape alone: the split-k partial tiles of the tile form of phase 1 in either regime, and at
// least the 1024 partial tiles of p1v2
static size_t workspace_capacity(const gp_ctx* c) {
  const int mt = c->Mp / TILE, dt = c->Dp / TILE, n_tiles = c->p1t.n_tiles;
  const int total_chunks = (int)(c->Np / KC);
  const int S = std::max(1, std::min(512 / std::max(1, std::min(n_tiles, mt * dt > 0 ? n_tiles : 1)), total_chunks));
  // worst case slices x tiles (regime B uses fewer tiles, hence possibly more slices)
  const int Tb = mt * dt;
  const int Sb = std::max(1, std::min(512 / std::max(1, Tb), total_chunks));
  // ... and at least the 1024 partial tiles of p1v2
  return std::max((size_t)std::max((long)(S + 16) * n_tiles, (long)(Sb + 16) * Tb) * TILE * TILE, (size_t)1100 * TILE * TILE);
}
int Workspace::alloc(gp_ctx* c) {
  capacity = workspace_capacity(c);
  return buf.alloc(c, capacity);
}
}  // namespace gp

using namespace gp;

// ---- argument checks the entry points share (`who` names the entry in the message).  all_finite works blockwise and finds no index ----
static bool all_finite(const double* x, size_t n) {
  for (size_t i0 = 0; i0 < n; i0 += 4096) {
    int ok = 1;        // no short circuit inside a block: the loop vectorises, and is then no slower than a scan that stops at the first bad element
    for (size_t i = i0, e = std::min(n, i0 + 4096); i < e; ++i) ok &= (int)std::isfinite(x[i]);
    if (!ok) return false;
  }
  return true;
}
static int finite_check(gp_ctx* c, const char* who, const char* name, const double* x, size_t n) {
  return all_finite(x, n) ? GP_OK : fail(c, GP_ERR_BAD_ARG, "%s: %s is not finite", who, name);
}
// Inputs at n new rows as the pair X_mu, X_S (NULL: deterministic): finite, and the variances >= 0 unless raw -- or, positive, > 0 in the form the
// model takes (the infer entries).  Element by element through both arrays: the first bad element decides which of the two is named.
static int inputs_check(gp_ctx* c, const char* who, int64_t n, const double* X_mu, const double* X_S, int raw, bool positive) {
  const size_t nq = (size_t)n * c->Q;
  if (!X_S) return finite_check(c, who, "X_mu", X_mu, nq);
  for (size_t i = 0; i < nq; ++i) {
    if (!std::isfinite(X_mu[i])) return fail(c, GP_ERR_BAD_ARG, "%s: X_mu is not finite", who);
    const double v = positive && raw ? std::log(1.0 + std::exp(X_S[i])) : X_S[i];
    if (!std::isfinite(X_S[i]) || (positive ? !std::isfinite(v) || !(v > 0.0) : !raw && v < 0.0))
      return fail(c, GP_ERR_BAD_ARG, positive ? "%s: X_S must be finite and > 0" : "%s: X_S must be finite and >= 0", who);
  }
  return GP_OK;
}
// A NULL array that stands for the resident rows (`what` says so in the entry's words): they have been uploaded, and n is their count
static int resident_rows_check(gp_ctx* c, const char* who, const char* what, int64_t n) {
  if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "%s: %s before gp_upload_shard", who, what);
  if (n != c->N) return fail(c, GP_ERR_BAD_ARG, "%s: %s: n must be N_s = %ld, got %ld", who, what, (long)c->N, (long)n);
  return GP_OK;
}
// Y (n, D) is finite wherever it is observed (a hidden entry is never read).  The column-list form: the same columns in every row, NULL = all D.
static int observed_cols_check(gp_ctx* c, const char* who, int64_t n, const double* Y, const int* cols, int n_cols) {
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < (cols ? n_cols : c->D); ++j)
      if (!std::isfinite(Y[i * c->D + (cols ? cols[j] : j)])) return fail(c, GP_ERR_BAD_ARG, "%s: Y is not finite in an observed column", who);
  return GP_OK;
}
// The per-row mask form (observed (n, D), nonzero = observed; NULL: every entry).  need_one: a row that observes nothing is an error too.
static int observed_mask_check(gp_ctx* c, const char* who, int64_t n, const double* Y, const uint8_t* observed, bool need_one) {
  for (int64_t i = 0; i < n; ++i) {
    int seen = 0;
    for (int j = 0; j < c->D; ++j) {
      if (observed && !observed[i * c->D + j]) continue;
      ++seen;
      if (!std::isfinite(Y[i * c->D + j])) return fail(c, GP_ERR_BAD_ARG, "%s: Y is not finite in an observed entry (row %ld, column %d)", who, (long)i, j);
    }
    if (need_one && !seen) return fail(c, GP_ERR_BAD_ARG, "%s: row %ld has no observed column", who, (long)i);
  }
  return GP_OK;
}

extern "C" const char* gp_last_error(const gp_ctx* ctx) { return ctx ? ctx->err.c_str() : gp::g_create_error.c_str(); }
extern "C" const char* gp_version(void) { return "gparml_hip 0.1 (gfx950, fp64 4x4x4-mfma)"; }

extern "C" int gp_create(gp_ctx** out, int device, int64_t N_s, int D, int M, int Q) {
  if (!out) return fail(nullptr, GP_ERR_BAD_ARG, "gp_create: out is NULL");
  *out = nullptr;
  if (N_s <= 0 || D <= 0 || M <= 0 || Q <= 0) return fail(nullptr, GP_ERR_BAD_ARG, "gp_create: N_s, D, M, Q must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, GP_ERR_HIP, "gp_create: no HIP device available");
  if (device < 0 || device >= ndev) return fail(nullptr, GP_ERR_BAD_ARG, "gp_create: device %d out of range (%d devices)", device, ndev);
  gp_ctx* c = new gp_ctx();
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) { delete c; return fail(nullptr, GP_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e)); }
  c->N = N_s; c->D = D; c->M = M; c->Q = Q;
  c->Np = round_up(N_s, TILE);
  c->Mp = (int)round_up(M, TILE);
  c->Dp = (int)round_up(D, TILE);
  c->LDK = c->Mp + c->Dp;
  c->CX = 2 * Q + 1; c->CXp = (int)round_up(c->CX, 4);
  c->CZ = 2 * Q + 1; c->CZp = (int)round_up(c->CZ, 4);
  const long Mp = c->Mp, Np = c->Np;
  int rc = GP_OK;
  auto A = [&](auto& b, size_t n, int mode = DA_INIT) { if (rc == GP_OK) rc = b.alloc(c, n, mode); };
  A(c->Kaug, (size_t)Np * c->LDK);
  A(c->Xmu, (size_t)N_s * Q); A(c->Xs, (size_t)N_s * Q); A(c->dir, (size_t)2 * N_s * Q);
  A(c->mu, (size_t)Np * Q); A(c->S, (size_t)Np * Q); A(c->U, (size_t)Np * Q);
  A(c->PU, (size_t)Np * (2 * std::max(psi1_qp(Q), 2) + 2), DA_ZERO);   // zero contract: the records' columns Q .. QP - 1 (u = 0: no guards in psi1_kernel's q loop) are never written
  A(c->lnc1, (size_t)Np); A(c->Xa, (size_t)Np * c->CXp);
  A(c->Z, (size_t)Mp * Q); A(c->shift, (size_t)Q, DA_ZERO); A(c->alpha, (size_t)Q); A(c->Zaug, (size_t)Mp * c->CZp + 8); A(c->Zt, (size_t)Mp * Q);   // + 8: p2_gen8_kernel stages feature columns in groups of eight
  A(c->stats, (size_t)stats_doubles(c));
  A(c->grads, (size_t)grads_doubles(c));
  A(c->gXmu, (size_t)N_s * Q); A(c->gXs, (size_t)N_s * Q);
  A(c->red, 8192);
  // the stages (eager: an evaluation allocates nothing of theirs); the workspace's capacity needs the tile table
  if (rc == GP_OK) rc = c->p1t.alloc(c);
  if (rc == GP_OK) rc = c->ws.alloc(c);
  if (rc == GP_OK) rc = c->gstep.alloc(c);
  if (rc == GP_OK) rc = c->p2.alloc(c);
  if (rc == GP_OK) rc = c->cg.alloc(c);
  for (int i = 0; i < 14 && rc == GP_OK; ++i) if (hipEventCreate(&c->ev[i]) != hipSuccess) rc = fail(c, GP_ERR_HIP, "hipEventCreate failed");
  if (rc == GP_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(c, GP_ERR_HIP, "device sync failed after allocation");
  if (rc != GP_OK) { gp::g_create_error = c->err; gp_destroy(c); return rc; }
  *out = c;
  return GP_OK;
}

extern "C" int gp_destroy(gp_ctx* c) {
  if (!c) return GP_OK;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  gp::comm_free(c);
  for (hipEvent_t e : c->ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->glob.glob_ev) if (e) (void)hipEventDestroy(e);
  delete c;     // the buffers are its DevBuf members
  return GP_OK;
}

extern "C" int gp_memory_info(gp_ctx* c, int64_t* free_bytes, int64_t* total_bytes) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  size_t f = 0, t = 0;
  GP_HIP(c, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return GP_OK;
}

extern "C" int gp_i8_status(gp_ctx* c, int* state, double* rel_psi2, double* rel_c, double* cond_lower_bound, int64_t* checks) {
  if (!c) return GP_ERR_BAD_ARG;
  if (state) *state = !p1i8_applicable_static(c) ? -1 : c->i8.guard;
  if (rel_psi2) *rel_psi2 = c->i8.rel_psi2;
  if (rel_c) *rel_c = c->i8.rel_c;
  if (cond_lower_bound) *cond_lower_bound = c->i8.cond_lb;
  if (checks) *checks = c->i8.checks;
  return GP_OK;
}

extern "C" int gp_set_timing(gp_ctx* c, int level) {
  if (!c) return GP_ERR_BAD_ARG;
  if (level < 0 || level > 2) return fail(c, GP_ERR_BAD_ARG, "gp_set_timing: level must be 0 (no events), 1 (total only) or 2 (every phase and kernel)");
  c->timing = level;
  return GP_OK;
}

extern "C" int gp_set_stream(gp_ctx* c, void* s) {
  if (!c) return GP_ERR_BAD_ARG;
  c->stream = (hipStream_t)s;
  return GP_OK;
}

static int upload_embeddings(gp_ctx* c, const double* X_mu, const double* X_S, int xs_is_raw) {
  const size_t nq = (size_t)c->N * c->Q;
  bool all_zero = true, any_neg = false, finite = true;
  for (size_t i = 0; i < nq; ++i) {
    const double s = X_S[i];
    if (s != 0.0) all_zero = false;
    if (s < 0.0) any_neg = true;
    if (!std::isfinite(s) || !std::isfinite(X_mu[i])) finite = false;
  }
  if (!finite) return fail(c, GP_ERR_NON_FINITE, "embeddings contain non-finite values");
  if (!xs_is_raw && any_neg) return fail(c, GP_ERR_BAD_ARG, "X_S must be >= 0 (kernel_exp.py:30 assertion)");
  if (!xs_is_raw && !all_zero) {
    for (size_t i = 0; i < nq; ++i) if (X_S[i] == 0.0) return fail(c, GP_ERR_NON_FINITE, "X_S mixes zero and non-zero variances: log(0) in the KL term (partial_terms.py:85)");
  }
  c->xs_raw = xs_is_raw != 0;
  c->regime_A = (!xs_is_raw) && all_zero;
  c->life.embeddings_changed();
  GP_HIP(c, hipMemcpyAsync(c->Xmu, X_mu, nq * 8, hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipMemcpyAsync(c->Xs, X_S, nq * 8, hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  return GP_OK;
}

// sum_YYT (partial_terms.py:40) of the dense rows dY [n]: 1024 block sums of sumsq_kernel, folded here in ascending order.  The one place the
// statistic is summed -- gp_upload_shard and gp_gather_shard (gather.hip) both come here, so the same rows give the same bits.  *out is set even
// when the sum is not finite.
int gp::sum_yyt(gp_ctx* c, const double* dY, long n, double* out) {
  const int nb = 1024;
  double* part = c->red;
  GP_LAUNCH(c, c->stream, sumsq_kernel, dim3(nb), dim3(256), 0, dY, n, part);
  std::vector<double> h(nb);
  hipError_t e = hipMemcpyAsync(h.data(), part, nb * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, GP_ERR_HIP, "sum_YYT failed: %s", hipGetErrorString(e));
  double s = 0.0;
  for (double v : h) s += v;
  *out = s;
  return std::isfinite(s) ? GP_OK : fail(c, GP_ERR_NON_FINITE, "Y contains non-finite values");
}

extern "C" int gp_upload_shard(gp_ctx* c, const double* Y, const double* X_mu, const double* X_S, int xs_is_raw) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!Y || !X_mu || !X_S) return fail(c, GP_ERR_BAD_ARG, "gp_upload_shard: NULL array");
  GP_HIP(c, hipSetDevice(c->device));
  const size_t nd = (size_t)c->N * c->D;
  DevBuf<double> dY;
  GP_TRY(dY.alloc(c, nd, DA_RAW));
  hipError_t e = hipMemcpyAsync(dY, Y, nd * 8, hipMemcpyHostToDevice, c->stream);
  int rc = GP_OK;
  if (e != hipSuccess) rc = fail(c, GP_ERR_HIP, "Y upload failed: %s", hipGetErrorString(e));
  if (rc == GP_OK) rc = run_upload_y(c, dY);
  if (rc == GP_OK) rc = sum_yyt(c, dY, (long)nd, &c->sumYY);      // once per upload
  if (rc != GP_OK) return rc;
  GP_TRY(upload_embeddings(c, X_mu, X_S, xs_is_raw));
  c->life.data_uploaded();
  c->i8.reset();      // new data: Y's digits are stale and the int8 path is measured again (p1i8.hip, guard)
  return GP_OK;
}

extern "C" int gp_upload_embeddings(gp_ctx* c, const double* X_mu, const double* X_S, int xs_is_raw) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "gp_upload_embeddings before gp_upload_shard");
  if (!X_mu || !X_S) return fail(c, GP_ERR_BAD_ARG, "gp_upload_embeddings: NULL array");
  GP_HIP(c, hipSetDevice(c->device));
  return upload_embeddings(c, X_mu, X_S, xs_is_raw);
}

extern "C" int gp_set_direction(gp_ctx* c, const double* d) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  if (!d) { c->life.direction_set(false); return GP_OK; }
  GP_HIP(c, hipMemcpyAsync(c->dir, d, (size_t)2 * c->N * c->Q * 8, hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  c->life.direction_set(true);
  return GP_OK;
}

// Test mode (gp_common.h, g_opt_poison): everything an evaluation is supposed to (re)write before it reads is refilled with NaN bytes when a new
// evaluation starts -- scratch and partial sums, the statistics, the global step's matrices, the gradients, Psi1 (not Y), the regime-B tables.
// Not refilled: the shard's data and what the prep kernels derive from it alone (they are skipped from the second evaluation on for fixed
// embeddings), the CG vectors, Linv (its upper blocks are a zero contract), tables and plans.
static int poison_scratch(gp_ctx* c) {
  for (const DevBuf<double>* b : {&c->ws.buf, &c->stats, &c->grads, &c->gXmu, &c->gXs}) GP_HIP(c, poison_fill(c, *b));
  GP_HIP(c, hipMemset2DAsync(c->Kaug, (size_t)c->LDK * 8, 0xFF, (size_t)c->Mp * 8, c->Np, c->stream));      // the Psi1 columns of [Psi1 | Y]
  GP_TRY(c->p2.poison(c));
  GP_TRY(c->gstep.poison(c));
  return b_poison(c);
}

// The origin of the centred coordinates (gp_ctx::shift): the column mean of Z.  It is kept from call to call while it stays inside the cloud of inducing
// points -- no further from their mean, in any dimension, than the farthest of them plus one length scale -- so that an optimiser's small steps of Z do not
// move it: a new origin means new centred means, and fixed embeddings would pay the prep kernels in every evaluation (Lifecycle::origin_moved).  With that bound
// every centred coordinate stays within about twice the spread of the points.
static int choose_origin(gp_ctx* c, const double* Z, const double* alpha) {
  const int M = c->M, Q = c->Q;
  std::vector<double> mean(Q, 0.0), spread(Q, 0.0);
  for (int m = 0; m < M; ++m) for (int q = 0; q < Q; ++q) mean[q] += Z[(long)m * Q + q] / M;
  for (int m = 0; m < M; ++m) for (int q = 0; q < Q; ++q) spread[q] = std::max(spread[q], std::fabs(Z[(long)m * Q + q] - mean[q]));
  bool keep = !c->h_shift.empty();
  for (int q = 0; keep && q < Q; ++q) {
    const double scale = alpha[q] > 0.0 ? 1.0 / std::sqrt(alpha[q]) : 0.0;
    keep = std::fabs(mean[q] - c->h_shift[q]) <= spread[q] + scale;
  }
  if (keep) return GP_OK;
  c->h_shift = mean;
  // a blocking copy from pageable memory (rare: see above); stream-ordered after whatever still reads the old origin
  GP_HIP(c, hipMemcpyAsync(c->shift, c->h_shift.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->life.origin_moved();
  return GP_OK;
}

extern "C" int gp_set_globals(gp_ctx* c, const double* Z, double sf2, const double* alpha, double beta, int64_t N_global, double step) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!Z || !alpha) return fail(c, GP_ERR_BAD_ARG, "gp_set_globals: NULL array");
  if (!(sf2 > 0.0)) return fail(c, GP_ERR_BAD_ARG, "sf2 must be > 0 (kernels.py:62 assert sf > 0)");
  if (!(beta > 0.0) || !std::isfinite(beta)) return fail(c, GP_ERR_BAD_ARG, "beta must be finite and > 0");
  for (int q = 0; q < c->Q; ++q) {
    if (!(alpha[q] >= 0.0)) return fail(c, GP_ERR_BAD_ARG, "alpha must be >= 0 (kernel_exp.py:31 assertion)");
    if (!std::isfinite(alpha[q])) return fail(c, GP_ERR_NON_FINITE, "alpha is not finite");
  }
  for (long i = 0; i < (long)c->M * c->Q; ++i) if (!std::isfinite(Z[i])) return fail(c, GP_ERR_NON_FINITE, "Z is not finite");
  if (N_global < c->N) return fail(c, GP_ERR_BAD_ARG, "N_global (%ld) smaller than the local shard (%ld)", (long)N_global, (long)c->N);
  GP_HIP(c, hipSetDevice(c->device));
  if (g_opt_poison.load()) GP_TRY(poison_scratch(c));
  // stage through pinned memory: hipMemcpyAsync from pageable memory blocks the host until the copy has been staged AND used to be followed by a
  // stream synchronisation here (r03: every evaluation of an optimiser paid it).  r05: no copy command at all -- zaug_kernel reads the pinned
  // (mapped) slot itself; two copy commands cost ~25 us of stream time at configs[1]'s size (blit dispatches with idle gaps around them,
  // profiles/r05_config1_timeline.txt) for 10 KB.  The evaluation's only host synchronisation is the read-back in gp_finish
  const size_t nz = (size_t)c->M * c->Q, nq = (size_t)c->Q;
  const int slot = c->glob.glob_slot;
  if (!c->glob.h_glob[slot]) {
    GP_TRY(c->glob.h_glob[slot].alloc(c, nz + nq));
  } else if (c->glob.glob_epoch[slot] >= c->sync_epoch) {
    // the kernel that read this slot two calls ago may still be queued: no stream synchronisation has been seen since (never the case in an
    // optimiser's sequence -- every evaluation ends in gp_finish's synchronisation -- so no event is recorded per call: that was one more signal
    // packet on the stream)
    GP_HIP(c, hipStreamSynchronize(c->stream));
    ++c->sync_epoch;
  }
  GP_TRY(choose_origin(c, Z, alpha));
  for (size_t i = 0; i < nz; ++i) c->glob.h_glob[slot][i] = Z[i] - c->h_shift[i % nq];      // centred: exact when Z and the origin are within a factor of two
  std::memcpy(c->glob.h_glob[slot] + nz, alpha, nq * sizeof(double));
  double* dslot = nullptr;
  GP_HIP(c, hipHostGetDevicePointer((void**)&dslot, c->glob.h_glob[slot], 0));
  GP_LAUNCH(c, c->stream, zaug_kernel, dim3((int)std::min<long>(((long)c->Mp * c->CZp + 255) / 256, 1024)), dim3(256), 0, dslot, dslot + nz, c->M, c->Mp, c->Q, c->CZp, c->Z,
            c->Zaug, c->alpha, c->Zt);
  c->glob.glob_epoch[slot] = c->sync_epoch;                      // the slot may be rewritten once a later stream synchronisation has passed
  c->glob.glob_slot = slot ^ 1;
  c->sf2 = sf2; c->beta = beta; c->N_global = N_global; c->step = step;
  c->life.globals_set();
  return GP_OK;
}

extern "C" int gp_phase1(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.can_phase1()) return fail(c, GP_ERR_STATE, "gp_phase1 needs gp_upload_shard and gp_set_globals first");
  GP_HIP(c, hipSetDevice(c->device));
  GP_EV(c, 0);
  GP_TRY(run_prep_and_generate(c));
  if (!c->regime_A) GP_TRY(run_generate_b(c));
  GP_EV(c, 1);
  GP_TRY(run_phase1(c));
  if (!c->regime_A) GP_TRY(run_phase1_b(c));
  GP_EV(c, 2);
  c->life.phase1_ran();
  return GP_OK;
}

extern "C" int gp_stats_buffer(gp_ctx* c, void** dev_ptr, int64_t* n) {
  if (!c) return GP_ERR_BAD_ARG;
  if (dev_ptr) *dev_ptr = c->stats;
  if (n) *n = stats_doubles(c);
  return GP_OK;
}

// ---- packed statistics for the all-reduce across processes: Psi2 upper triangle (row-major) | C [M][D] | scalars
// element e of the packed payload <-> its place in the padded statistics buffer (second index: the mirrored Psi2 element, or -1)
__device__ __forceinline__ bool spack_map(long e, int M, int Mp, int D, int Dp, long* k, long* s0, long* s1) {
  const long tri = (long)M * (M + 1) / 2, md = (long)M * D;
  *s1 = -1;
  if (e < (long)M * M) {
    const int i = (int)(e / M), j = (int)(e - (long)i * M);
    if (j < i) return false;
    *k = (long)i * M - (long)i * (i - 1) / 2 + (j - i);
    *s0 = (long)i * Mp + j; *s1 = (long)j * Mp + i;
  } else if (e < (long)M * M + md) {
    const long r = e - (long)M * M;
    const int i = (int)(r / D), d = (int)(r - (long)i * D);
    *k = tri + r; *s0 = (long)Mp * Mp + (long)i * Dp + d;
  } else {
    const long r = e - (long)M * M - md;
    *k = tri + md + r; *s0 = (long)Mp * Mp + (long)Mp * Dp + r;
  }
  return true;
}
__global__ void __launch_bounds__(256) stats_pack_kernel(const double* __restrict__ stats, double* __restrict__ pk, int M, int Mp, int D, int Dp) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < (long)M * M + (long)M * D + SC_COUNT; e += (long)gridDim.x * 256L) {
    long k, s0, s1;
    if (spack_map(e, M, Mp, D, Dp, &k, &s0, &s1)) pk[k] = stats[s0];
  }
}
__global__ void __launch_bounds__(256) stats_unpack_kernel(const double* __restrict__ pk, double* __restrict__ stats, int M, int Mp, int D, int Dp) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < (long)M * M + (long)M * D + SC_COUNT; e += (long)gridDim.x * 256L) {
    long k, s0, s1;
    if (spack_map(e, M, Mp, D, Dp, &k, &s0, &s1)) { const double v = pk[k]; stats[s0] = v; if (s1 >= 0) stats[s1] = v; }
  }
}
static int ensure_spack(gp_ctx* c) {
  if (!c->spack) GP_TRY(c->spack.alloc(c, spack_doubles(c), DA_ZERO));   // zero contract: gp_stats_packed_buffer hands it out before any pack
  return GP_OK;
}
extern "C" int gp_stats_packed_buffer(gp_ctx* c, void** dev_ptr, int64_t* n) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  GP_TRY(ensure_spack(c));
  if (dev_ptr) *dev_ptr = c->spack;
  if (n) *n = spack_doubles(c);
  return GP_OK;
}
static int stats_pack(gp_ctx* c, int unpack_) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.has_stats()) return fail(c, GP_ERR_STATE, "gp_stats_pack / gp_stats_unpack before gp_phase1");
  GP_HIP(c, hipSetDevice(c->device));
  GP_TRY(ensure_spack(c));
  const long n = (long)c->M * c->M + (long)c->M * c->D + SC_COUNT;
  if (unpack_) {
    c->life.stats_unpacked();
    // the packed buffer only holds statistics after a pack (it is zero from its allocation): unpacking first would silently wipe phase 1's sums
    if (!c->life.packed_is_current()) return fail(c, GP_ERR_STATE, "gp_stats_unpack before gp_stats_pack");
    GP_LAUNCH(c, c->stream, stats_unpack_kernel, dim3(blocks_for(n)), dim3(256), 0, (const double*)c->spack, c->stats, c->M, c->Mp, c->D, c->Dp);
  } else {
    GP_LAUNCH(c, c->stream, stats_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, (const double*)c->stats, c->spack, c->M, c->Mp, c->D, c->Dp);
    c->life.stats_packed();
  }
  return GP_OK;
}
extern "C" int gp_stats_pack(gp_ctx* c) { return stats_pack(c, 0); }
extern "C" int gp_stats_unpack(gp_ctx* c) { return stats_pack(c, 1); }

extern "C" int gp_grads_buffer(gp_ctx* c, void** dev_ptr, int64_t* n) {
  if (!c) return GP_ERR_BAD_ARG;
  if (dev_ptr) *dev_ptr = c->grads;
  if (n) *n = grads_doubles(c);
  return GP_OK;
}

__global__ void combine_kernel(double* dst, const double* src, long n, int op) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) dst[i] = (op == 0 ? dst[i] : 0.0) + src[i];
}
__global__ void grad_latest_kernel(const double* __restrict__ gmu, const double* __restrict__ gS, const double* __restrict__ Xs,
                                   const double* __restrict__ dir, long N, int Q, double step, int raw, int have_dir, double* __restrict__ out) {
  const long nq = N * Q;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nq; i += (long)gridDim.x * 256L) {
    out[i] = -gmu[i];
    double g = gS[i];
    if (raw) {
      double x = Xs[i];
      if (have_dir && step != 0.0) x = mul_then_add(step, dir[nq + i], x);      // the trial point's own raw variance, bit for bit (prep_elem_kernel)
      g *= softplus_slope(x);      // transformVar_grad, supporting_functions.py:165-168
    }
    out[nq + i] = -g;
  }
}

extern "C" int gp_buffer_combine(gp_ctx* dst, const gp_ctx* src, int which, int op) {
  if (!dst || !src) return GP_ERR_BAD_ARG;
  if (dst->M != src->M || dst->Q != src->Q || dst->D != src->D) return fail(dst, GP_ERR_BAD_ARG, "gp_buffer_combine: shape mismatch");
  const long n = which == 0 ? stats_doubles(dst) : grads_doubles(dst);
  const double* from = which == 0 ? src->stats : src->grads;
  // the source context's work must have finished before its buffer is read from another stream / device
  if (src->stream != dst->stream || src->device != dst->device) {
    GP_HIP(dst, hipSetDevice(src->device));
    GP_HIP(dst, hipStreamSynchronize(src->stream));
  }
  GP_HIP(dst, hipSetDevice(dst->device));
  if (src->device != dst->device || g_force_staging) {
    // shards on different GPUs of one process (options['devices']): peer copy into a staging buffer on the destination
    // device, then the same combine kernel -- the device-side form of statistics_reducer (local_MapReduce.py:250-277)
    GP_TRY(dst->staging.grow(dst, n, DA_RAW));
    GP_HIP(dst, hipMemcpyPeerAsync(dst->staging, dst->device, from, src->device, (size_t)n * 8, dst->stream));
    from = dst->staging;
  }
  GP_LAUNCH(dst, dst->stream, combine_kernel, dim3(blocks_for(n)), dim3(256), 0, which == 0 ? dst->stats : dst->grads, from, n, op);
  if (which == 0) dst->life.stats_combined();
  return GP_OK;
}

extern "C" int gp_scale_buffer(gp_ctx* c, int which, double f) {
  if (!c) return GP_ERR_BAD_ARG;
  if (which != 0 && which != 1) return fail(c, GP_ERR_BAD_ARG, "gp_scale_buffer: which must be 0 (statistics) or 1 (gradient sums)");
  if (which == 0 && !c->life.has_stats()) return fail(c, GP_ERR_STATE, "gp_scale_buffer(statistics) before gp_phase1");
  if (which == 1 && !c->life.phase2_done()) return fail(c, GP_ERR_STATE, "gp_scale_buffer(gradient sums) before gp_phase2");
  GP_HIP(c, hipSetDevice(c->device));
  const long n = which == 0 ? stats_doubles(c) : grads_doubles(c);
  if (which == 0) c->life.stats_scaled();   // a later unpack needs a new pack
  if (f == 0.0) {
    // a dropped shard: the reference never loads its files (local_MapReduce.py:119-129) -- a memset, so that non-finite values in
    // the dropped shard's sums (0 * inf = nan) cannot reach the reduction
    GP_HIP(c, hipMemsetAsync(which == 0 ? c->stats : c->grads, 0, (size_t)n * sizeof(double), c->stream));
    return GP_OK;
  }
  GP_LAUNCH(c, c->stream, scale_kernel, dim3(blocks_for(n)), dim3(256), 0, which == 0 ? c->stats : c->grads, n, f);
  return GP_OK;
}

extern "C" int gp_scale_stats(gp_ctx* c, double f) { return gp_scale_buffer(c, 0, f); }

extern "C" int gp_global_step_jitter(gp_ctx* c, int jitter_mask) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.has_stats()) return fail(c, GP_ERR_STATE, "gp_global_step before gp_phase1 / gp_set_local_statistics");
  if (jitter_mask < 0 || jitter_mask > 3) return fail(c, GP_ERR_BAD_ARG, "gp_global_step_jitter: mask must be 0..3");
  GP_HIP(c, hipSetDevice(c->device));
  c->gstep.jitter_mask = jitter_mask;
  c->gstep.svi_step = false;
  c->life.step_started();
  GP_EV(c, 3);
  const int rc_gs = run_global_step(c);
  GP_EV(c, 4);
  if (rc_gs != GP_OK) return rc_gs;
  c->life.step_enqueued();           // scalars and failure flags are read back at the next host synchronisation point (check_global)
  return GP_OK;
}

extern "C" int gp_global_step(gp_ctx* c) { return gp_global_step_jitter(c, 0); }

// The int8 guard's decision (p1i8.hip) for an evaluation that ran both phase-1 paths.  It needs P = (K_mm + beta Psi2)^-1 of a global step that SUCCEEDED:
// a step that failed or asks for the jitter retry leaves P non-finite and would reject the int8 path for a reason that has nothing to do with its
// accuracy -- the check then stays pending (guard 0: the next evaluation runs both paths again).  Called wherever an evaluation's global step is
// known to be over: gp_finish, gp_global_status, gp_download of a global-step array.
static int resolve_i8_check(gp_ctx* c) {
  if (!c->i8.check_pending || !c->life.step_done()) return GP_OK;
  if (c->gstep.svi_step) return GP_OK;            // gp_svi_step wrote no P: the check stays pending for the next collapsed step
  if (check_global(c) != GP_OK) return GP_OK;     // the caller reports that status itself
  return p1i8_check_finish(c);
}

extern "C" int gp_global_status(gp_ctx* c, int* retry_mask) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.step_done()) return fail(c, GP_ERR_STATE, "gp_global_status before gp_global_step");
  GP_HIP(c, hipSetDevice(c->device));
  GP_TRY(resolve_i8_check(c));
  const int rc = check_global(c);
  if (retry_mask) *retry_mask = (rc == GP_RETRY_JITTER) ? c->gstep.retry_mask : 0;
  return rc;
}

extern "C" int gp_phase2(gp_ctx* c, int want_embedding_grads) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.step_done()) return fail(c, GP_ERR_STATE, "gp_phase2 before gp_global_step");
  if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "gp_phase2 without shard data");
  GP_HIP(c, hipSetDevice(c->device));
  GP_EV(c, 5);
  if ((want_embedding_grads != 0) != c->life.embedding_mode()) {
    // the per-point feature matrix depends on the mode: rebuild the trial point
    c->life.phase2_mode(want_embedding_grads != 0);
    GP_TRY(run_prep_and_generate(c));
  }
  GP_TRY(run_phase2(c));
  if (!c->regime_A) GP_TRY(run_phase2_b(c));
  if (c->life.embedding_mode() && c->xs_raw) {
    // the .grad_latest vector of this evaluation, resident for the optimiser's dot products
    const long nq = (long)c->N * c->Q;
    GP_LAUNCH(c, c->stream, grad_latest_kernel, dim3(blocks_for(nq)), dim3(256), 0, c->gXmu, c->gXs, c->Xs, c->dir, (long)c->N, c->Q, c->step,
              1, c->life.has_direction() ? 1 : 0, c->cg.g_latest);
    c->life.grad_latest_written();
  }
  GP_EV(c, 6);
  c->life.phase2_ran();
  return GP_OK;
}

extern "C" int gp_last_timings(gp_ctx* c, double* out8) {
  double* out5 = out8;
  if (!c || !out8) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 8; ++i) out8[i] = 0.0;
  float ms;
  ++c->sync_epoch;
  if (c->timing == 1) {       // only the evaluation's first and last event were recorded
    if (c->life.phase2_timed() && hipEventElapsedTime(&ms, c->ev[0], c->ev[6]) == hipSuccess) out5[4] = ms;
    return GP_OK;
  }
  if (c->timing == 0) return GP_OK;
  if (c->life.phase1_timed() && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) out5[0] = ms;
  if (c->life.phase1_timed() && hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) out5[1] = ms;
  if (c->life.step_timed() && hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) out5[2] = ms;
  if (c->life.phase2_timed() && hipEventElapsedTime(&ms, c->ev[5], c->ev[6]) == hipSuccess) out5[3] = ms;
  out5[4] = out5[0] + out5[1] + out5[2] + out5[3];
  if (c->life.phase1_timed() && hipEventElapsedTime(&ms, c->ev[8], c->ev[9]) == hipSuccess) out8[5] = ms;
  if (c->life.phase1_timed() && hipEventElapsedTime(&ms, c->ev[10], c->ev[11]) == hipSuccess) out8[6] = ms;
  if (c->life.phase2_timed() && hipEventElapsedTime(&ms, c->ev[12], c->ev[13]) == hipSuccess) out8[7] = ms;
  return GP_OK;
}

extern "C" int gp_download(gp_ctx* c, int which, double* dst, int64_t n) {
  if (!c || !dst) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  const long M = c->M, Mp = c->Mp, D = c->D, Dp = c->Dp, N = c->N, Q = c->Q;
  if (c->life.step_done() && (which == GP_ARR_KMM_INV || which == GP_ARR_KMM_PLUS_OP_INV || which == GP_ARR_DF_DKMM || which == GP_ARR_DF_DPSI1TY ||
                        which == GP_ARR_DF_DPSI2 || which == GP_ARR_SCALARS)) {
    GP_TRY(resolve_i8_check(c));
    GP_TRY(check_global(c));
  }
  switch (which) {
    case GP_ARR_PSI1: return download_matrix(c, c->Kaug, c->LDK, N, M, dst, n);
    case GP_ARR_PSI2_SUM: return download_matrix(c, c->stats, Mp, M, M, dst, n);
    case GP_ARR_PSI1TY: return download_matrix(c, c->stats + Mp * Mp, Dp, M, D, dst, n);
    case GP_ARR_KMM: return download_matrix(c, c->gstep.KmmKeep, Mp, M, M, dst, n);
    case GP_ARR_KMM_INV: return download_matrix(c, c->gstep.Inv, Mp, M, M, dst, n);
    case GP_ARR_KMM_PLUS_OP_INV: return download_matrix(c, c->gstep.Inv + Mp * Mp, Mp, M, M, dst, n);
    case GP_ARR_DF_DKMM: return download_matrix(c, c->gstep.dFdK, Mp, M, M, dst, n);
    case GP_ARR_DF_DPSI1TY: return download_matrix(c, c->gstep.Abar, Dp, M, D, dst, n);
    case GP_ARR_DF_DPSI2: return download_matrix(c, c->gstep.Bbar, Mp, M, M, dst, n);
    case GP_ARR_GRAD_X_MU: return download_matrix(c, c->gXmu, Q, N, Q, dst, n);
    case GP_ARR_GRAD_X_S: return download_matrix(c, c->gXs, Q, N, Q, dst, n);
    case GP_ARR_X_MU_TRIAL: {
      GP_TRY(download_matrix(c, c->mu, Q, N, Q, dst, n));
      for (long i = 0; i < N * Q && !c->h_shift.empty(); ++i) dst[i] += c->h_shift[i % Q];     // the resident trial means are centred (gp_ctx::shift)
      return GP_OK;
    }
    case GP_ARR_X_S_TRIAL: return download_matrix(c, c->S, Q, N, Q, dst, n);
    case GP_ARR_X_MU:
      if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "GP_ARR_X_MU before gp_upload_shard");
      return download_matrix(c, c->Xmu, Q, N, Q, dst, n);
    case GP_ARR_GRAD_LATEST: {
      if (!c->life.grad_latest_ready()) return fail(c, GP_ERR_STATE, "GP_ARR_GRAD_LATEST needs gp_phase2(ctx, 1) first");
      if (n != 2 * N * Q) return fail(c, GP_ERR_BAD_ARG, "GP_ARR_GRAD_LATEST wants %ld doubles", 2 * N * Q);
      if (c->regime_A) return fail(c, GP_ERR_NON_FINITE, "grad_X_S with X_S == 0 (1/S, partial_terms.py:417)");
      DevBuf<double> tmp;
      GP_TRY(tmp.alloc(c, 2 * N * Q, DA_RAW));
      GP_LAUNCH(c, c->stream, grad_latest_kernel, dim3(blocks_for(N * Q)), dim3(256), 0, c->gXmu, c->gXs, c->Xs, c->dir, N, (int)Q, c->step,
                c->xs_raw ? 1 : 0, c->life.has_direction() ? 1 : 0, tmp);
      hipError_t e = hipMemcpyAsync(dst, tmp, 2 * N * Q * 8, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) return fail(c, GP_ERR_HIP, "download failed: %s", hipGetErrorString(e));
      return GP_OK;
    }
    case GP_ARR_SCALARS: {
      if (n != 8) return fail(c, GP_ERR_BAD_ARG, "GP_ARR_SCALARS wants 8 doubles");
      double sc[SC_COUNT];
      GP_HIP(c, hipMemcpyAsync(sc, c->stats + Mp * Mp + Mp * Dp, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
      GP_HIP(c, hipStreamSynchronize(c->stream));
      dst[0] = sc[SC_SUM_YYT]; dst[1] = sc[SC_PSI0]; dst[2] = sc[SC_KL];
      dst[3] = c->gstep.h_gs[GS_LOGDET_K]; dst[4] = c->gstep.h_gs[GS_LOGDET_A]; dst[5] = c->gstep.h_gs[GS_F]; dst[6] = c->gstep.h_gs[GS_GRAD_BETA]; dst[7] = c->gstep.h_gs[GS_GRAD_SF2];
      return GP_OK;
    }
    case GP_ARR_PSI2_POINTS: case GP_ARR_DKMM_DZ: case GP_ARR_DPSI1TY_DZ: case GP_ARR_DPSI2_DZ: case GP_ARR_DKMM_DALPHA:
    case GP_ARR_DPSI1TY_DALPHA: case GP_ARR_DPSI2_DALPHA: {
      DevBuf<double> buf;
      GP_TRY(compat_build(c, which, buf));
      const long cnt = (long)buf.size();
      if (cnt != n) return fail(c, GP_ERR_BAD_ARG, "gp_download: expected %ld doubles, got %ld", cnt, (long)n);
      hipError_t e = hipMemcpyAsync(dst, buf, cnt * 8, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) return fail(c, GP_ERR_HIP, "download failed: %s", hipGetErrorString(e));
      return GP_OK;
    }
    default: return fail(c, GP_ERR_UNSUPPORTED, "gp_download: array %d not available", which);
  }
}

extern "C" int gp_set_local_statistics(gp_ctx* c, double sum_YYT, const double* Psi2, const double* C, double sum_exp_K_ii, double KL) {
  if (!c || !Psi2 || !C) return GP_ERR_BAD_ARG;
  if (!c->life.has_globals()) return fail(c, GP_ERR_STATE, "gp_set_local_statistics before gp_set_globals");
  GP_HIP(c, hipSetDevice(c->device));
  const long M = c->M, Mp = c->Mp, D = c->D, Dp = c->Dp;
  double* tmp = c->gstep.T2;
  GP_HIP(c, hipMemcpyAsync(tmp, Psi2, M * M * 8, hipMemcpyHostToDevice, c->stream));
  GP_LAUNCH(c, c->stream, scatter2d_kernel, dim3(blocks_for(Mp * Mp)), dim3(256), 0, tmp, M, M, c->stats, Mp, Mp, Mp);
  GP_HIP(c, hipStreamSynchronize(c->stream));
  GP_HIP(c, hipMemcpyAsync(tmp, C, M * D * 8, hipMemcpyHostToDevice, c->stream));
  GP_LAUNCH(c, c->stream, scatter2d_kernel, dim3(blocks_for(Mp * Dp)), dim3(256), 0, tmp, M, D, c->stats + Mp * Mp, Dp, Mp, Dp);
  double sc[SC_COUNT] = {0};
  sc[SC_SUM_YYT] = sum_YYT; sc[SC_PSI0] = sum_exp_K_ii; sc[SC_KL] = KL; sc[SC_NLOCAL] = sum_exp_K_ii / c->sf2;
  GP_HIP(c, hipMemcpyAsync(c->stats + Mp * Mp + Mp * Dp, sc, sizeof(sc), hipMemcpyHostToDevice, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  c->life.stats_injected();    // the packed payload of an earlier evaluation no longer describes these statistics
  return GP_OK;
}

// gp_predict / gp_infer_*: the model of a global step that saw the statistics and globals as they are now, and succeeded
static int model_ready(gp_ctx* c, const char* who) {
  if (!c->life.model_current())
    return fail(c, GP_ERR_STATE, "%s needs a global step on the statistics and globals as they are now (none since the last phase 1, "
                "gp_set_globals, gp_set_local_statistics, gp_buffer_combine, gp_scale_buffer or gp_stats_unpack)", who);
  GP_HIP(c, hipSetDevice(c->device));
  GP_TRY(resolve_i8_check(c));
  if (check_global(c) != GP_OK) return fail(c, GP_ERR_STATE, "%s: the last global step did not succeed (%s)", who, c->gstep.gs_msg.c_str());
  return GP_OK;
}

extern "C" int gp_predict(gp_ctx* c, int64_t n, const double* X_mu, const double* X_S, int xs_is_raw, int flags, double* mean, double* var) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_predict: n must be >= 0");
  if (flags & ~1) return fail(c, GP_ERR_BAD_ARG, "gp_predict: unknown flags %d", flags);
  GP_TRY(model_ready(c, "gp_predict"));
  if (n == 0) return GP_OK;
  if (!X_mu) return fail(c, GP_ERR_BAD_ARG, "gp_predict: X_mu is NULL");
  GP_TRY(inputs_check(c, "gp_predict", n, X_mu, X_S, xs_is_raw, false));
  if (!mean && !var) return GP_OK;
  return run_predict(c, (long)n, X_mu, X_S, xs_is_raw, flags, mean, var);
}

// ---- held-out scoring (score.hip): gp_predict's state rule and input checks, then the outputs' own ----
extern "C" int gp_predict_score(gp_ctx* c, int64_t n, const double* X_mu, const double* X_S, int xs_is_raw, const double* Y, const uint8_t* observed,
                                int flags, double* row_logp, double* row_sse, double* row_chi2, double* cols) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_predict_score: n must be >= 0");
  if (flags & ~3) return fail(c, GP_ERR_BAD_ARG, "gp_predict_score: unknown flags %d", flags);
  if ((flags & 2) && X_mu) return fail(c, GP_ERR_BAD_ARG, "gp_predict_score: flags bit 1 (the resident variances) needs X_mu == NULL (the resident rows)");
  GP_TRY(model_ready(c, "gp_predict_score"));
  const size_t D = (size_t)c->D;
  const bool resident = X_mu == nullptr;
  if (resident) {      // the resident rows' own rules come first: they hold for every n, n = 0 included
    GP_TRY(resident_rows_check(c, "gp_predict_score", "X_mu is NULL (the resident rows)", n));
    if (X_S || xs_is_raw) return fail(c, GP_ERR_BAD_ARG, "gp_predict_score: X_mu is NULL (the resident rows): X_S must be NULL and xs_is_raw 0 (flags bit 1 takes the resident variances)");
  }
  if (n == 0) {
    if (cols) std::fill(cols, cols + 5 * D, 0.0);
    return GP_OK;
  }
  if (!resident) {
    if (!Y) return fail(c, GP_ERR_BAD_ARG, "gp_predict_score: Y is NULL with host inputs");
    GP_TRY(inputs_check(c, "gp_predict_score", n, X_mu, X_S, xs_is_raw, false));
  }
  if (Y) GP_TRY(observed_mask_check(c, "gp_predict_score", n, Y, observed, false));
  if (!row_logp && !row_sse && !row_chi2 && !cols) return GP_OK;
  return run_predict_score(c, (long)n, X_mu, X_S, xs_is_raw ? 1 : 0, resident, (flags & 2) != 0, Y, observed, flags, row_logp, row_sse, row_chi2, cols);
}

// ---- leave-one-out / leave-block-out scoring of the resident rows (loo.hip): the argument errors first, then gp_predict_score's state rule ----
extern "C" int gp_loo_score(gp_ctx* c, int block, const uint8_t* observed, int flags, double* row_logp, double* row_sse, double* row_chi2, double* lev,
                            double* var_loo, double* cols) {
  if (!c) return GP_ERR_BAD_ARG;
  if (block < 1 || block > 128) return fail(c, GP_ERR_BAD_ARG, "gp_loo_score: block must be 1 .. 128, got %d", block);
  if (flags & ~1) return fail(c, GP_ERR_BAD_ARG, "gp_loo_score: unknown flags %d", flags);
  GP_TRY(model_ready(c, "gp_loo_score"));
  if (!c->life.has_data()) return fail(c, GP_ERR_STATE, "gp_loo_score: the resident rows before gp_upload_shard");
  if (!c->regime_A)
    return fail(c, GP_ERR_UNSUPPORTED, "gp_loo_score: the shard has embeddings of non-zero variance: such a row contributes a full-rank psi2 to "
                "Kmm + beta Psi2, and leaving it out is not a rank-one downdate (fixed embeddings only)");
  if (!row_logp && !row_sse && !row_chi2 && !lev && !var_loo && !cols) return GP_OK;
  return run_loo_score(c, block, observed, flags, row_logp, row_sse, row_chi2, lev, var_loo, cols);
}

// gp_predict_joint / gp_predict_sample: gp_predict's preconditions and argument errors for deterministic inputs, then the size limit
static int joint_check(gp_ctx* c, const char* who, int64_t n, const double* X, int flags, int64_t n_max, bool* nothing) {
  *nothing = true;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "%s: n must be >= 0", who);
  if (flags & ~1) return fail(c, GP_ERR_BAD_ARG, "%s: unknown flags %d", who, flags);
  GP_TRY(model_ready(c, who));
  if (n == 0) return GP_OK;
  if (!X) return fail(c, GP_ERR_BAD_ARG, "%s: X is NULL", who);
  if (n > n_max) return fail(c, GP_ERR_UNSUPPORTED, "%s: n = %ld is beyond the limit of %ld points of one call (the n x n matrix is held on the device)", who, (long)n, (long)n_max);
  GP_TRY(finite_check(c, who, "X", X, (size_t)n * c->Q));
  *nothing = false;
  return GP_OK;
}

extern "C" int gp_predict_joint(gp_ctx* c, int64_t n, const double* X, int flags, double* mean, double* cov) {
  if (!c) return GP_ERR_BAD_ARG;
  bool nothing;
  GP_TRY(joint_check(c, "gp_predict_joint", n, X, flags, 16384, &nothing));
  if (nothing || (!mean && !cov)) return GP_OK;
  return run_predict_joint(c, (long)n, X, flags, mean, cov);
}

extern "C" int gp_predict_sample(gp_ctx* c, int64_t n, const double* X, int flags, double jitter, int n_draws, const double* eps, double* out, double* mean) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(c, GP_ERR_BAD_ARG, "gp_predict_sample: jitter must be finite and >= 0");
  if (n_draws < 0) return fail(c, GP_ERR_BAD_ARG, "gp_predict_sample: n_draws must be >= 0");
  if (n_draws > 0 && (!eps || !out)) return fail(c, GP_ERR_BAD_ARG, "gp_predict_sample: eps or out is NULL");
  bool nothing;
  GP_TRY(joint_check(c, "gp_predict_sample", n, X, flags, 8192, &nothing));
  if (nothing || n_draws == 0) return GP_OK;
  GP_TRY(finite_check(c, "gp_predict_sample", "eps", eps, (size_t)n_draws * n * c->D));
  return run_predict_sample(c, (long)n, X, flags, jitter, n_draws, eps, out, mean);
}

extern "C" int gp_predict_grad(gp_ctx* c, int64_t n, const double* X, int flags, double* jac, double* dvar, double* metric, double* logdet) {
  if (!c) return GP_ERR_BAD_ARG;
  if (flags != 0) return fail(c, GP_ERR_BAD_ARG, "gp_predict_grad: flags is reserved and must be 0 (got %d)", flags);
  bool nothing;
  GP_TRY(joint_check(c, "gp_predict_grad", n, X, 0, INT64_MAX, &nothing));
  if (nothing || (!jac && !dvar && !metric && !logdet)) return GP_OK;
  if (logdet && c->Q > 64)
    return fail(c, GP_ERR_UNSUPPORTED, "gp_predict_grad: logdet is computed on the device for Q <= 64 only (Q = %d): pass NULL and take slogdet of the metric", c->Q);
  return run_predict_grad(c, (long)n, X, jac, dvar, metric, logdet);
}

// ---- curve energy (curve.hip) ----
extern "C" int gp_curve_energy(gp_ctx* c, int64_t n_curves, int T, const double* X, int flags, double* energy, double* seg, double* grad) {
  if (!c) return GP_ERR_BAD_ARG;
  if (flags != 0) return fail(c, GP_ERR_BAD_ARG, "gp_curve_energy: flags is reserved and must be 0 (got %d)", flags);
  if (T < 2) return fail(c, GP_ERR_BAD_ARG, "gp_curve_energy: a curve has at least two points (T = %d)", T);
  if (n_curves > INT64_MAX / ((int64_t)T * c->Q)) return fail(c, GP_ERR_BAD_ARG, "gp_curve_energy: n_curves T Q overflows");
  bool nothing;
  GP_TRY(joint_check(c, "gp_curve_energy", n_curves * T, X, 0, INT64_MAX, &nothing));
  if (nothing || (!energy && !seg && !grad)) return GP_OK;
  return run_curve_energy(c, (long)n_curves, T, X, energy, seg, grad);
}

// ---- pathwise posterior draws (paths.hip) ----
extern "C" int gp_paths_set(gp_ctx* c, int n_draws, int F, const double* omega, const double* centre, const double* w, const double* eps_u) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n_draws < 1 || F < 1) return fail(c, GP_ERR_BAD_ARG, "gp_paths_set: n_draws and F must be >= 1 (got %d, %d)", n_draws, F);
  if (!omega || !w || !eps_u) return fail(c, GP_ERR_BAD_ARG, "gp_paths_set: omega, w or eps_u is NULL");
  GP_TRY(model_ready(c, "gp_paths_set"));
  const long bytes = paths_operand_bytes(c, n_draws, F);
  if ((double)n_draws * c->D > 1e9 || (double)F > 1e8 || bytes > (2L << 30))
    return fail(c, GP_ERR_UNSUPPORTED, "gp_paths_set: the packed operand of %d draws at F = %d would exceed the limit of 2 GiB: set fewer draws at a time", n_draws, F);
  const size_t D = (size_t)c->D;
  if (!all_finite(omega, (size_t)F * c->Q) || (centre && !all_finite(centre, (size_t)c->Q)) || !all_finite(w, (size_t)n_draws * 2 * F * D) ||
      !all_finite(eps_u, (size_t)n_draws * c->M * D))
    return fail(c, GP_ERR_BAD_ARG, "gp_paths_set: omega, centre, w or eps_u is not finite");
  return run_paths_set(c, n_draws, F, omega, centre, w, eps_u);
}

extern "C" int gp_paths_eval(gp_ctx* c, int64_t n, const double* X, int flags, double* out, double* mean) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_paths_eval: n must be >= 0");
  if (flags != 0) return fail(c, GP_ERR_BAD_ARG, "gp_paths_eval: flags is reserved and must be 0 (got %d)", flags);
  if (const int rc = model_ready(c, "gp_paths_eval"); rc != GP_OK) {
    c->paths.reset();            // the draws were of a model that is gone
    return rc;
  }
  if (!paths_plan_current(c))
    return fail(c, GP_ERR_STATE, "gp_paths_eval needs gp_paths_set on the model as it is now (none yet, or a global step, new statistics or new globals since)");
  if (n == 0) return GP_OK;
  if (!X || !out) return fail(c, GP_ERR_BAD_ARG, "gp_paths_eval: X or out is NULL");
  GP_TRY(finite_check(c, "gp_paths_eval", "X", X, (size_t)n * c->Q));
  return run_paths_eval(c, (long)n, X, out, mean);
}

// the argument errors that need nothing of the model first, then gp_paths_eval's state rule (a model, a current plan), then the arrays
extern "C" int gp_paths_grad(gp_ctx* c, int64_t n, const double* X, int flags, const double* weights, double* jac, double* grad, double* metric,
                             double* mean_jac) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 1) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: n must be >= 1 (got %ld)", (long)n);
  if (flags & ~GP_PATHS_WEIGHTS_PER_ROW) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: unknown flags %d", flags);
  if (!jac && !grad && !metric && !mean_jac) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: jac, grad, metric and mean_jac are all NULL");
  if ((grad != nullptr) != (weights != nullptr)) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: weights go with grad (both, or neither)");
  if (!X) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: X is NULL");
  if (const int rc = model_ready(c, "gp_paths_grad"); rc != GP_OK) {
    c->paths.reset();            // the draws were of a model that is gone
    return rc;
  }
  if (!paths_plan_current(c))
    return fail(c, GP_ERR_STATE, "gp_paths_grad needs gp_paths_set on the model as it is now (none yet, or a global step, new statistics or new globals since)");
  const int64_t S = paths_plan_draws(c);
  if (n > INT64_MAX / (S * c->D * std::max(c->Q, 1) * c->Q)) return fail(c, GP_ERR_BAD_ARG, "gp_paths_grad: n_draws n D Q overflows");
  GP_TRY(finite_check(c, "gp_paths_grad", "X", X, (size_t)n * c->Q));
  if (weights)
    GP_TRY(finite_check(c, "gp_paths_grad", "weights", weights, (flags & GP_PATHS_WEIGHTS_PER_ROW) ? (size_t)S * n * c->D : (size_t)c->D));
  return run_paths_grad(c, (long)n, X, flags, weights, jac, grad, metric, mean_jac);
}

extern "C" int gp_paths_clear(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  c->paths.reset();
  return GP_OK;
}

// ---- the posterior conditioned on extra observed rows (condition.hip): the order of the checks is gp_paths_set's / gp_paths_eval's ----
extern "C" int gp_condition_set(gp_ctx* c, int64_t m, const double* Xc, const double* Yc) {
  if (!c) return GP_ERR_BAD_ARG;
  if (m < 1) return fail(c, GP_ERR_BAD_ARG, "gp_condition_set: m must be >= 1 (got %ld)", (long)m);
  if (!Xc || !Yc) return fail(c, GP_ERR_BAD_ARG, "gp_condition_set: Xc or Yc is NULL");
  GP_TRY(model_ready(c, "gp_condition_set"));
  if (m > 1024)
    return fail(c, GP_ERR_UNSUPPORTED, "gp_condition_set: m = %ld is beyond the limit of 1024 conditioning rows (the m x m factorisation is held on the device): "
                "refit with the rows in the statistics", (long)m);
  GP_TRY(finite_check(c, "gp_condition_set", "Xc", Xc, (size_t)m * c->Q));
  GP_TRY(finite_check(c, "gp_condition_set", "Yc", Yc, (size_t)m * c->D));
  return run_condition_set(c, (long)m, Xc, Yc);
}

extern "C" int gp_condition_predict(gp_ctx* c, int64_t n, const double* X, int flags, double* mean, double* var, double* reduction) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_condition_predict: n must be >= 0");
  if (flags & ~1) return fail(c, GP_ERR_BAD_ARG, "gp_condition_predict: unknown flags %d", flags);
  if (const int rc = model_ready(c, "gp_condition_predict"); rc != GP_OK) {
    c->cond.reset();             // the rows were conditioned on a model that is gone
    return rc;
  }
  if (!cond_plan_current(c))
    return fail(c, GP_ERR_STATE, "gp_condition_predict needs gp_condition_set on the model as it is now (none yet, or a global step, new statistics or new globals since)");
  if (n == 0) return GP_OK;
  if (!X) return fail(c, GP_ERR_BAD_ARG, "gp_condition_predict: X is NULL");
  GP_TRY(finite_check(c, "gp_condition_predict", "X", X, (size_t)n * c->Q));
  if (!mean && !var && !reduction) return GP_OK;
  return run_condition_predict(c, (long)n, X, flags, mean, var, reduction);
}

extern "C" int gp_condition_clear(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  c->cond.reset();
  return GP_OK;
}

// gp_infer_objective / gp_infer_latent and their _rows forms: gp_predict's preconditions, then the arguments of the new rows.  masked: the observed
// set of every row (observed) in place of the one column list (cols, n_cols)
static int infer_check(gp_ctx* c, const char* who, int64_t n, const double* Y, const int* cols, int n_cols, bool masked, const uint8_t* observed,
                       const double* X_mu, const double* X_S, int raw, bool* nothing) {
  *nothing = true;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "%s: n must be >= 0", who);
  if (!masked) {
    if (cols ? (n_cols < 1 || n_cols > c->D) : n_cols != 0)
      return fail(c, GP_ERR_BAD_ARG, "%s: n_cols must be 1 .. D with a column list and 0 without one", who);
    for (int j = 0; cols && j < n_cols; ++j)
      if (cols[j] < 0 || cols[j] >= c->D || (j && cols[j] <= cols[j - 1]))
        return fail(c, GP_ERR_BAD_ARG, "%s: cols must be strictly increasing in 0 .. D - 1", who);
  }
  GP_TRY(model_ready(c, who));
  if (n == 0) return GP_OK;
  if (!Y || (masked && !observed) || !X_mu || !X_S) return fail(c, GP_ERR_BAD_ARG, masked ? "%s: Y, observed, X_mu or X_S is NULL" : "%s: Y, X_mu or X_S is NULL", who);
  GP_TRY(inputs_check(c, who, n, X_mu, X_S, raw, true));
  GP_TRY(masked ? observed_mask_check(c, who, n, Y, observed, true) : observed_cols_check(c, who, n, Y, cols, n_cols));
  *nothing = false;
  return GP_OK;
}

extern "C" int gp_infer_objective(gp_ctx* c, int64_t n, const double* Y, const int* cols, int n_cols, const double* X_mu, const double* X_S, int xs_is_raw,
                                  double* L, double* grad_mu, double* grad_S) {
  if (!c) return GP_ERR_BAD_ARG;
  bool nothing;
  GP_TRY(infer_check(c, "gp_infer_objective", n, Y, cols, n_cols, false, nullptr, X_mu, X_S, xs_is_raw, &nothing));
  if (nothing || (!L && !grad_mu && !grad_S)) return GP_OK;
  return run_infer(c, 0, (long)n, Y, cols, n_cols, const_cast<double*>(X_mu), const_cast<double*>(X_S), xs_is_raw ? 1 : 0, 0, 0.0, L, grad_mu, grad_S, nullptr);
}

extern "C" int gp_infer_latent(gp_ctx* c, int64_t n, const double* Y, const int* cols, int n_cols, double* X_mu, double* X_S, int xs_is_raw, int max_iters,
                               double gtol, double* L, int32_t* iters) {
  if (!c) return GP_ERR_BAD_ARG;
  if (max_iters < 0 || !(gtol >= 0.0)) return fail(c, GP_ERR_BAD_ARG, "gp_infer_latent: max_iters and gtol must be >= 0");
  bool nothing;
  GP_TRY(infer_check(c, "gp_infer_latent", n, Y, cols, n_cols, false, nullptr, X_mu, X_S, xs_is_raw, &nothing));
  if (nothing) return GP_OK;
  return run_infer(c, 1, (long)n, Y, cols, n_cols, X_mu, X_S, xs_is_raw ? 1 : 0, max_iters, gtol, L, nullptr, nullptr, iters);
}

extern "C" int gp_infer_objective_rows(gp_ctx* c, int64_t n, const double* Y, const uint8_t* observed, const double* X_mu, const double* X_S, int xs_is_raw,
                                       double* L, double* grad_mu, double* grad_S) {
  if (!c) return GP_ERR_BAD_ARG;
  bool nothing;
  GP_TRY(infer_check(c, "gp_infer_objective_rows", n, Y, nullptr, 0, true, observed, X_mu, X_S, xs_is_raw, &nothing));
  if (nothing || (!L && !grad_mu && !grad_S)) return GP_OK;
  return run_infer_rows(c, 0, (long)n, Y, observed, const_cast<double*>(X_mu), const_cast<double*>(X_S), xs_is_raw ? 1 : 0, 0, 0.0, L, grad_mu, grad_S, nullptr);
}

extern "C" int gp_infer_latent_rows(gp_ctx* c, int64_t n, const double* Y, const uint8_t* observed, double* X_mu, double* X_S, int xs_is_raw, int max_iters,
                                    double gtol, double* L, int32_t* iters) {
  if (!c) return GP_ERR_BAD_ARG;
  if (max_iters < 0 || !(gtol >= 0.0)) return fail(c, GP_ERR_BAD_ARG, "gp_infer_latent_rows: max_iters and gtol must be >= 0");
  bool nothing;
  GP_TRY(infer_check(c, "gp_infer_latent_rows", n, Y, nullptr, 0, true, observed, X_mu, X_S, xs_is_raw, &nothing));
  if (nothing) return GP_OK;
  return run_infer_rows(c, 1, (long)n, Y, observed, X_mu, X_S, xs_is_raw ? 1 : 0, max_iters, gtol, L, nullptr, nullptr, iters);
}

// One Lloyd assignment pass (csrc/kmeans.hip).  Nothing of the evaluation is read or written: only the resident X_mu (X == NULL) and the plan's buffers.
extern "C" int gp_kmeans_accumulate(gp_ctx* c, int64_t n, const double* X, int K, const double* centres, double* sums, int64_t* counts, double* dist2,
                                    int32_t* labels) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_kmeans_accumulate: n must be >= 0");
  if (K < 1) return fail(c, GP_ERR_BAD_ARG, "gp_kmeans_accumulate: K must be >= 1");
  if (!centres) return fail(c, GP_ERR_BAD_ARG, "gp_kmeans_accumulate: centres is NULL");
  if (!X) GP_TRY(resident_rows_check(c, "gp_kmeans_accumulate", "X is NULL (the resident X_mu)", n));
  const size_t kq = (size_t)K * c->Q;
  GP_TRY(finite_check(c, "gp_kmeans_accumulate", "centres", centres, kq));
  if (X) GP_TRY(finite_check(c, "gp_kmeans_accumulate", "X", X, (size_t)n * c->Q));
  if (n == 0) {
    if (sums) std::fill(sums, sums + kq, 0.0);
    if (counts) std::fill(counts, counts + K, (int64_t)0);
    if (dist2) dist2[0] = dist2[1] = 0.0;
    return GP_OK;
  }
  if (!sums && !counts && !dist2 && !labels) return GP_OK;
  GP_HIP(c, hipSetDevice(c->device));
  return run_kmeans(c, (long)n, X, K, centres, sums, counts, dist2, labels);
}

// The two passes of the PCA initialisation (csrc/pca.hip).  Nothing of the evaluation is read or written: only the Y columns of Kaug (Y == NULL) and
// the plan's buffers.
static int pca_rows_check(gp_ctx* c, const char* who, int64_t n, const double* Y) {
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "%s: n must be >= 0", who);
  return Y ? finite_check(c, who, "Y", Y, (size_t)n * c->D) : resident_rows_check(c, who, "Y is NULL (the resident Y)", n);
}

extern "C" int gp_scatter_accumulate(gp_ctx* c, int64_t n, const double* Y, const double* centre, double* sum, double* gram) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!centre) return fail(c, GP_ERR_BAD_ARG, "gp_scatter_accumulate: centre is NULL");
  GP_TRY(pca_rows_check(c, "gp_scatter_accumulate", n, Y));
  GP_TRY(finite_check(c, "gp_scatter_accumulate", "centre", centre, (size_t)c->D));
  if (n == 0) {
    if (sum) std::fill(sum, sum + c->D, 0.0);
    if (gram) std::fill(gram, gram + (size_t)c->D * c->D, 0.0);
    return GP_OK;
  }
  if (!sum && !gram) return GP_OK;
  GP_HIP(c, hipSetDevice(c->device));
  return run_scatter(c, (long)n, Y, centre, sum, gram);
}

extern "C" int gp_project_rows(gp_ctx* c, int64_t n, const double* Y, const double* mean, const double* P, int Q_out, double* X) {
  if (!c) return GP_ERR_BAD_ARG;
  if (Q_out < 1) return fail(c, GP_ERR_BAD_ARG, "gp_project_rows: Q_out must be >= 1");
  if (!mean || !P) return fail(c, GP_ERR_BAD_ARG, "gp_project_rows: mean or P is NULL");
  GP_TRY(pca_rows_check(c, "gp_project_rows", n, Y));
  if (!all_finite(mean, (size_t)c->D) || !all_finite(P, (size_t)c->D * Q_out)) return fail(c, GP_ERR_BAD_ARG, "gp_project_rows: mean or P is not finite");
  if (n == 0) return GP_OK;
  if (!X) return fail(c, GP_ERR_BAD_ARG, "gp_project_rows: X is NULL");
  GP_HIP(c, hipSetDevice(c->device));
  return run_project(c, (long)n, Y, mean, P, Q_out, X);
}

// ---- greedy conditional-variance selection of the inducing points (csrc/select.hip) ----
// Nothing of the evaluation is read or written: only the resident X_mu (X == NULL) and the plan's buffers.
static int select_plan(gp_ctx* c, const char* who) {
  if (!c->sel) return fail(c, GP_ERR_STATE, "%s before gp_select_begin (or after gp_select_end)", who);
  GP_HIP(c, hipSetDevice(c->device));
  return GP_OK;
}

extern "C" int gp_select_begin(gp_ctx* c, int64_t n, const double* X, int K, double sf2, const double* alpha, double tol) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: n must be >= 0");
  if (K < 1) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: K must be >= 1");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: tol must be finite and >= 0");
  if (!(sf2 > 0.0) || !std::isfinite(sf2)) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: sf2 must be finite and > 0");
  if (!alpha) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: alpha is NULL");
  for (int q = 0; q < c->Q; ++q)
    if (!(alpha[q] >= 0.0) || !std::isfinite(alpha[q])) return fail(c, GP_ERR_BAD_ARG, "gp_select_begin: alpha must be finite and >= 0");
  GP_TRY(X ? finite_check(c, "gp_select_begin", "X", X, (size_t)n * c->Q) : resident_rows_check(c, "gp_select_begin", "X is NULL (the resident X_mu)", n));
  GP_HIP(c, hipSetDevice(c->device));
  c->sel.reset();                    // an earlier plan goes first: its memory counts as free
  size_t free_b = 0, total_b = 0;
  GP_HIP(c, hipMemGetInfo(&free_b, &total_b));
  const double need = 8.0 * (double)K * (double)std::max<int64_t>(n, 1);      // the factor alone, before any rounding: no overflow
  if (need > (double)free_b || (double)select_bytes(c, (long)n, K, X != nullptr) > (double)free_b)
    return fail(c, GP_ERR_UNSUPPORTED, "gp_select_begin: the factor of n = %ld rows and K = %d columns takes %.3g bytes, %.3g are free on the device: "
                "select over fewer rows per shard, or fewer points", (long)n, K, need, (double)free_b);
  return run_select_begin(c, (long)n, X, K, sf2, alpha, tol);
}

extern "C" int gp_select_run(gp_ctx* c, int steps, int32_t* n_done, int64_t* rows, double* trace) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_TRY(select_plan(c, "gp_select_run"));
  if (steps < 0) return fail(c, GP_ERR_BAD_ARG, "gp_select_run: steps must be >= 0");
  if (!n_done || (steps > 0 && !rows)) return fail(c, GP_ERR_BAD_ARG, "gp_select_run: n_done or rows is NULL");
  return run_select_run(c, steps, n_done, rows, trace);
}

extern "C" int gp_select_candidate(gp_ctx* c, double* d, int64_t* row, double* x, double* l) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_TRY(select_plan(c, "gp_select_candidate"));
  if (!d || !row) return fail(c, GP_ERR_BAD_ARG, "gp_select_candidate: d or row is NULL");
  return run_select_candidate(c, d, row, x, l);
}

extern "C" int gp_select_apply(gp_ctx* c, const double* x_p, const double* l_p, double d_p, int64_t own_row, double* trace) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_TRY(select_plan(c, "gp_select_apply"));
  long n; int K, j;
  select_info(c, &n, &K, &j);
  if (j >= K) return fail(c, GP_ERR_STATE, "gp_select_apply: all K = %d steps of this selection are done", K);
  if (!x_p || (j > 0 && !l_p)) return fail(c, GP_ERR_BAD_ARG, "gp_select_apply: x_p or l_p is NULL");
  if (!(d_p > 0.0) || !std::isfinite(d_p)) return fail(c, GP_ERR_BAD_ARG, "gp_select_apply: d_p must be finite and > 0");
  if (own_row < -1 || own_row >= n) return fail(c, GP_ERR_BAD_ARG, "gp_select_apply: own_row = %ld is outside -1 .. n - 1 = %ld", (long)own_row, n - 1);
  if (!all_finite(x_p, (size_t)c->Q) || !all_finite(l_p, (size_t)j)) return fail(c, GP_ERR_BAD_ARG, "gp_select_apply: x_p or l_p is not finite");
  return run_select_apply(c, x_p, l_p, d_p, own_row, trace);
}

extern "C" int gp_select_end(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  GP_TRY(select_plan(c, "gp_select_end"));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  ++c->sync_epoch;
  c->sel.reset();
  return GP_OK;
}

// Per new row the nearest training row (csrc/nearest.hip).  Nothing of the evaluation is read or written: only the Y columns of Kaug and the resident
// X_mu (Y_train == NULL) and the plan's buffers.  One body for both entries (fn names the entry in the messages): masked = every new row has its
// own observed set (observed (n,D), nonzero = observed), else the one column list cols for all of them.
static int nearest_entry(gp_ctx* c, const char* fn, int64_t n_train, const double* Y_train, int64_t n, const double* Y_test, const int32_t* cols,
                         int n_cols, bool masked, const uint8_t* observed, double* dist2, int64_t* index, double* x_near) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "%s: n must be >= 0", fn);
  if (cols && n_cols < 1) return fail(c, GP_ERR_BAD_ARG, "%s: n_cols must be >= 1 with a column list (got %d)", fn, n_cols);
  for (int j = 0; cols && j < n_cols; ++j)
    if (cols[j] < 0 || cols[j] >= c->D) return fail(c, GP_ERR_BAD_ARG, "%s: cols[%d] = %d is outside 0 .. D - 1 = %d", fn, j, cols[j], c->D - 1);
  if (Y_train && x_near) return fail(c, GP_ERR_BAD_ARG, "%s: x_near is the base mean of a resident row: it cannot be asked for with host rows (Y_train)", fn);
  if (!Y_train) {
    n_train = c->N;       // the resident rows are all of them: only their presence is left to check
    GP_TRY(resident_rows_check(c, fn, "Y_train is NULL (the resident rows)", n_train));
  } else if (n_train < 0) {
    return fail(c, GP_ERR_BAD_ARG, "%s: n_train must be >= 0", fn);
  }
  if (n == 0) return GP_OK;
  if (!Y_test) return fail(c, GP_ERR_BAD_ARG, "%s: Y_test is NULL", fn);
  if (masked && !observed) return fail(c, GP_ERR_BAD_ARG, "%s: observed is NULL", fn);
  const int nc = cols ? n_cols : c->D;
  for (int64_t i = 0; i < n; ++i) {
    bool ok = true;
    int seen = 0;
    for (int j = 0; j < nc; ++j) {
      const int64_t e = i * c->D + (cols ? cols[j] : j);
      if (masked && !observed[e]) continue;               // an unobserved element is never read: it may be NaN
      ++seen;
      ok = ok && std::isfinite(Y_test[e]);
    }
    if (!seen) return fail(c, GP_ERR_BAD_ARG, "%s: row %lld of Y_test has no observed column", fn, (long long)i);
    if (!ok) return fail(c, GP_ERR_BAD_ARG, "%s: Y_test is not finite in an observed column", fn);
  }
  if (Y_train) GP_TRY(finite_check(c, fn, "Y_train", Y_train, (size_t)n_train * c->D));
  if (!dist2 && !index && !x_near) return GP_OK;
  if (n_train == 0) {
    if (dist2) std::fill(dist2, dist2 + n, std::numeric_limits<double>::infinity());
    if (index) std::fill(index, index + n, (int64_t)-1);
    return GP_OK;
  }
  GP_HIP(c, hipSetDevice(c->device));
  return run_nearest(c, (long)n_train, Y_train, (long)n, Y_test, cols, n_cols, masked ? observed : nullptr, dist2, index, x_near);
}

extern "C" int gp_nearest_rows(gp_ctx* c, int64_t n_train, const double* Y_train, int64_t n, const double* Y_test, const int32_t* cols, int n_cols,
                               double* dist2, int64_t* index, double* x_near) {
  return nearest_entry(c, "gp_nearest_rows", n_train, Y_train, n, Y_test, cols, n_cols, false, nullptr, dist2, index, x_near);
}

extern "C" int gp_nearest_rows_masked(gp_ctx* c, int64_t n_train, const double* Y_train, int64_t n, const double* Y_test, const uint8_t* observed,
                                      double* dist2, int64_t* index, double* x_near) {
  return nearest_entry(c, "gp_nearest_rows_masked", n_train, Y_train, n, Y_test, nullptr, 0, true, observed, dist2, index, x_near);
}

// The k nearest rows in latent space (csrc/knn.hip).  Nothing of the evaluation is read or written: only the resident X_mu (a NULL side) and the
// plan's buffers.  Every argument is checked before anything is launched.
extern "C" int gp_knn_rows(gp_ctx* c, int64_t n_train, const double* X_train, int64_t n, const double* X, const double* weight, int k, const int64_t* skip,
                           int flags, double* dist2, int64_t* rows) {
  if (!c) return GP_ERR_BAD_ARG;
  if (n < 0) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: n must be >= 0");
  if (X_train && n_train < 0) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: n_train must be >= 0");
  if (k < 1) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: k must be >= 1");
  if (flags & ~1) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: unknown flags 0x%x (bit 0: every query leaves out its own row)", flags);
  const bool self = (flags & 1) != 0;
  if (self && (X_train || X)) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: bit 0 of flags needs the resident rows on both sides (X_train and X NULL)");
  if (self && skip) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: skip and bit 0 of flags are alternatives");
  if (k > 32) return fail(c, GP_ERR_UNSUPPORTED, "gp_knn_rows: k = %d, at most 32 neighbours per query", k);
  if (!X_train) {
    n_train = c->N;       // the resident rows are all of them: only their presence is left to check
    GP_TRY(resident_rows_check(c, "gp_knn_rows", "X_train is NULL (the resident X_mu)", n_train));
  }
  if (!X) GP_TRY(resident_rows_check(c, "gp_knn_rows", "X is NULL (the resident X_mu as queries)", n));
  if (X) GP_TRY(finite_check(c, "gp_knn_rows", "X", X, (size_t)n * c->Q));
  if (X_train) GP_TRY(finite_check(c, "gp_knn_rows", "X_train", X_train, (size_t)n_train * c->Q));
  for (int q = 0; weight && q < c->Q; ++q)
    if (!(weight[q] >= 0.0) || !std::isfinite(weight[q])) return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: weight must be finite and >= 0");
  for (int64_t i = 0; skip && i < n; ++i)
    if (skip[i] < -1 || skip[i] >= n_train)
      return fail(c, GP_ERR_BAD_ARG, "gp_knn_rows: skip[%lld] = %lld is outside -1 .. n_train - 1 = %lld", (long long)i, (long long)skip[i], (long long)n_train - 1);
  if (n == 0 || (!dist2 && !rows)) return GP_OK;
  if (n_train == 0) {
    if (dist2) std::fill(dist2, dist2 + n * k, std::numeric_limits<double>::infinity());
    if (rows) std::fill(rows, rows + n * k, (int64_t)-1);
    return GP_OK;
  }
  GP_HIP(c, hipSetDevice(c->device));
  return run_knn(c, (long)n_train, X_train, (long)n, X, weight, k, skip, self, dist2, rows);
}

// ---- final gradients ---------------------------------------------------------------------------------------------
// final = Kmm parts (global step) + all-reduced data parts (phase 2)
__global__ void add_kernel(const double* a, const double* b, double* out, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) out[i] = a[i] + b[i];
}
// gp_finish's only launch: out = [global-step scalars and failure flags (ngs) | Kmm parts + data parts of grad_Z, grad_alpha (n)], written straight
// into pinned host memory -- one kernel and one stream synchronisation instead of copy, synchronise, kernel, copy, synchronise (r04: the second
// round trip and the two blit dispatches were ~0.1 ms of wall time per evaluation at configs[1]'s size, profiles/r05_config1_timeline.txt)
__global__ void finish_kernel(const double* __restrict__ gs, int ngs, const double* __restrict__ a, const double* __restrict__ b, long n,
                              double* __restrict__ out) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < ngs + n; i += (long)gridDim.x * 256L) out[i] = i < ngs ? gs[i] : a[i - ngs] + b[i - ngs];
}

extern "C" int gp_finish(gp_ctx* c, double* F, double* grad_Z, double* grad_sf2, double* grad_alpha, double* grad_beta) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->life.step_done()) return fail(c, GP_ERR_STATE, "gp_finish before gp_global_step");
  GP_HIP(c, hipSetDevice(c->device));
  const bool want_grads = grad_Z || grad_alpha;
  GP_TRY(resolve_i8_check(c));      // this evaluation ran both phase-1 paths: decide whether the context stays on int8 (only behind a successful global step)
  if (want_grads && !c->life.phase2_done()) {
    GP_TRY(check_global(c));   // a failed global step is the more useful message
    return fail(c, GP_ERR_STATE, "gp_finish: gradients requested before gp_phase2");
  }
  if (!want_grads) {
    GP_TRY(check_global(c));
  } else {
    // the one host synchronisation of an evaluation: scalars + failure flags of the global step and the final gradients in one mapped buffer
    const long n = grads_doubles(c);
    constexpr int ngs = GS_HOST;
    if (!c->h_out) GP_TRY(c->h_out.alloc(c, ngs + n));
    double* dout = nullptr;
    GP_HIP(c, hipHostGetDevicePointer((void**)&dout, c->h_out, 0));
    GP_LAUNCH(c, c->stream, finish_kernel, dim3(blocks_for(ngs + n)), dim3(256), 0, c->gstep.gs, ngs, c->gstep.gK, c->grads, n, dout);
    GP_HIP(c, hipStreamSynchronize(c->stream));
    ++c->sync_epoch;
    GP_TRY(check_global_from(c, c->life.step_outcome_pending() ? c->h_out : nullptr));
    if (grad_Z) memcpy(grad_Z, c->h_out + ngs, (size_t)c->M * c->Q * 8);
    if (grad_alpha) memcpy(grad_alpha, c->h_out + ngs + (size_t)c->M * c->Q, (size_t)c->Q * 8);
  }
  if (F) *F = c->gstep.h_gs[GS_F];
  if (grad_sf2) *grad_sf2 = c->gstep.h_gs[GS_GRAD_SF2];
  if (grad_beta) *grad_beta = c->gstep.h_gs[GS_GRAD_BETA];
  return GP_OK;
}
