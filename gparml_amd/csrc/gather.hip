// Rows of a resident shard into a batch context and the embeddings back (gp_gather_shard, gp_scatter_embeddings).
//
// gp_gather_shard leaves dst as gp_upload_shard(dst, Y[rows], X_mu[rows], X_S[rows], xs_is_raw) would: the Y segment of [Psi1 | Y] with its zero
// padding written, the base embeddings in their stored form, sum_YYT.  Pure data movement, HBM bound: 8 n (2 Dp + 4 Q) bytes for the rows themselves.
// sum_YYT must be the upload's bits, so it takes the upload's road: gather_y_kernel also writes the rows dense [n][D] into the plan's buffer (what the
// upload's host copy delivers) and gp::sum_yyt runs the upload's sumsq_kernel over it -- one more write and read of 8 n D bytes, no second summation
// order to keep in step with the first.
// gp_scatter_embeddings writes a batch context's X_mu / X_S back into the rows they came from; Y never moves back.
#include "gp_common.h"

using namespace gp;

namespace gp {
// the index list on the device, and the dense copy of the gathered Y for sum_YYT; built on first use, each grows on demand
struct GatherPlan {
  DevBuf<long long> idx;      // [n]
  DevBuf<double> dense;       // [n][D] (gp_gather_shard only)
};
void GatherPlanDelete::operator()(GatherPlan* p) const { delete p; }
}  // namespace gp

// One wave per row i of the written context, grid-stride over its Np rows: rows[i] is read once, wave-uniform; the lanes lie along the Dp columns
// of the Y segment, one double2 each per 128 columns (both segments start 1 KB-aligned: Mp and LDK are multiples of 128 doubles).  Rows >= n and
// columns >= D store zeros whatever was there.  64-bit offsets throughout (Np LDK exceeds 2^31 at the full sizes).
__global__ void __launch_bounds__(256) gather_y_kernel(const double* __restrict__ srcK, long src_ld, int src_Mp, const long long* __restrict__ rows,
                                                       long n, long Np, int D, int Dp, double* __restrict__ dstK, long dst_ld, int dst_Mp,
                                                       double* __restrict__ dense) {
  const int lane = threadIdx.x & 63;
  const long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), waves = (long)gridDim.x * 4;
  for (long i = wave; i < Np; i += waves) {
    double2* out = reinterpret_cast<double2*>(dstK + i * dst_ld + dst_Mp);
    if (i < n) {
      const double2* in = reinterpret_cast<const double2*>(srcK + (long)rows[i] * src_ld + src_Mp);
      for (int c = lane; 2 * c < Dp; c += 64) {
        double2 v = in[c];
        if (2 * c >= D) v.x = 0.0;
        if (2 * c + 1 >= D) v.y = 0.0;
        out[c] = v;
        if (2 * c < D) dense[i * D + 2 * c] = v.x;
        if (2 * c + 1 < D) dense[i * D + 2 * c + 1] = v.y;
      }
    } else {
      for (int c = lane; 2 * c < Dp; c += 64) out[c] = double2{0.0, 0.0};
    }
  }
}

// The [N][Q] rows are short: threads over the flat n Q index.  to_rows = 0: out row i = in row rows[i] (gather); 1: out row rows[i] = in row i
// (scatter; the rows are distinct, so no element is written twice)
__global__ void __launch_bounds__(256) move_embeddings_kernel(const double* __restrict__ in_mu, const double* __restrict__ in_s,
                                                              const long long* __restrict__ rows, long n, int Q, int to_rows,
                                                              double* __restrict__ out_mu, double* __restrict__ out_s) {
  const long total = n * Q;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long i = e / Q, q = e - i * Q, r = (long)rows[i] * Q + q;
    const long from = to_rows ? e : r, to = to_rows ? r : e;
    out_mu[to] = in_mu[from];
    out_s[to] = in_s[from];
  }
}

// What both entries ask before anything happens (`dst` is the written context and takes the message): the pair, the shapes, the source's data, the
// count against the batch-sized side and every index against the other.  strict: the list must ascend strictly (no row twice).
static int gather_check(gp_ctx* dst, const gp_ctx* src, const char* who, int64_t n, const int64_t* rows, int64_t want_n, int64_t limit, bool strict) {
  if (!rows) return fail(dst, GP_ERR_BAD_ARG, "%s: rows is NULL", who);
  if (dst == src) return fail(dst, GP_ERR_BAD_ARG, "%s: dst and src are the same context", who);
  if (dst->device != src->device)
    return fail(dst, GP_ERR_UNSUPPORTED, "%s: the contexts are on devices %d and %d (rows move within one device only)", who, dst->device, src->device);
  if (dst->D != src->D || dst->Q != src->Q)
    return fail(dst, GP_ERR_BAD_ARG, "%s: shape mismatch (D %d / %d, Q %d / %d)", who, dst->D, src->D, dst->Q, src->Q);
  if (!src->life.has_data()) return fail(dst, GP_ERR_STATE, "%s: src holds no shard data", who);
  if (n != want_n) return fail(dst, GP_ERR_BAD_ARG, "%s: n must be the batch context's N_s = %ld, got %ld", who, (long)want_n, (long)n);
  for (int64_t i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= limit) return fail(dst, GP_ERR_BAD_ARG, "%s: rows[%ld] = %ld is outside [0, %ld)", who, (long)i, (long)rows[i], (long)limit);
    if (strict && i > 0 && rows[i] <= rows[i - 1]) return fail(dst, GP_ERR_BAD_ARG, "%s: rows must ascend strictly (rows[%ld] = %ld after %ld)", who, (long)i, (long)rows[i], (long)rows[i - 1]);
  }
  return GP_OK;
}

// The written context's plan with room for n indices (and dense doubles), published only once every buffer stands; then the order of
// gp_buffer_combine -- the other context's stream has finished before its buffers are read from this one -- and the index list on the device
static int gather_begin(gp_ctx* dst, const gp_ctx* src, int64_t n, const int64_t* rows, size_t dense) {
  GP_HIP(dst, hipSetDevice(dst->device));
  std::unique_ptr<GatherPlan, GatherPlanDelete> fresh;
  if (!dst->gather) fresh.reset(new GatherPlan());
  GatherPlan& p = dst->gather ? *dst->gather : *fresh;
  GP_TRY_RC(p.idx.grow(dst, (size_t)n, DA_RAW));
  if (dense) GP_TRY_RC(p.dense.grow(dst, dense, DA_RAW));
  if (fresh) dst->gather = std::move(fresh);
  if (src->stream != dst->stream) GP_HIP(dst, hipStreamSynchronize(src->stream));
  static_assert(sizeof(long long) == sizeof(int64_t), "the rows are copied in as they are");
  GP_HIP(dst, hipMemcpyAsync(dst->gather->idx, rows, (size_t)n * 8, hipMemcpyHostToDevice, dst->stream));
  return GP_OK;
}

extern "C" int gp_gather_shard(gp_ctx* dst, const gp_ctx* src, int64_t n, const int64_t* rows) {
  if (!dst || !src) return GP_ERR_BAD_ARG;
  GP_TRY_RC(gather_check(dst, src, "gp_gather_shard", n, rows, dst->N, src->N, false));
  GP_TRY_RC(gather_begin(dst, src, n, rows, (size_t)n * dst->D));
  const GatherPlan& p = *dst->gather;
  const unsigned blocks = (unsigned)std::min<long>((dst->Np + 3) / 4, 16384);
  GP_LAUNCH(dst, dst->stream, gather_y_kernel, dim3(blocks), dim3(256), 0, (const double*)src->Kaug, (long)src->LDK, src->Mp, (const long long*)p.idx,
            (long)n, (long)dst->Np, dst->D, dst->Dp, dst->Kaug, (long)dst->LDK, dst->Mp, p.dense);
  GP_LAUNCH(dst, dst->stream, move_embeddings_kernel, dim3(blocks_for(n * dst->Q)), dim3(256), 0, (const double*)src->Xmu, (const double*)src->Xs,
            (const long long*)p.idx, (long)n, dst->Q, 0, dst->Xmu, dst->Xs);
  GP_TRY_RC(sum_yyt(dst, p.dense, (long)n * dst->D, &dst->sumYY));      // synchronises: rows and the plan's buffers are free again
  ++dst->sync_epoch;
  // the flags and the events of an upload of these rows (api.hip, gp_upload_shard): every row of src is of src's regime
  dst->xs_raw = src->xs_raw;
  dst->regime_A = src->regime_A;
  dst->life.embeddings_changed();
  dst->life.data_uploaded();
  dst->i8.reset();
  return GP_OK;
}

extern "C" int gp_scatter_embeddings(gp_ctx* dst, const gp_ctx* src, int64_t n, const int64_t* rows) {
  if (!dst || !src) return GP_ERR_BAD_ARG;
  GP_TRY_RC(gather_check(dst, src, "gp_scatter_embeddings", n, rows, src->N, dst->N, true));
  if (!dst->life.has_data()) return fail(dst, GP_ERR_STATE, "gp_scatter_embeddings: dst holds no shard data");
  if (dst->xs_raw != src->xs_raw || dst->regime_A != src->regime_A)
    return fail(dst, GP_ERR_BAD_ARG, "gp_scatter_embeddings: the contexts store their variances differently (xs_is_raw %d / %d, fixed %d / %d)",
                (int)dst->xs_raw, (int)src->xs_raw, (int)dst->regime_A, (int)src->regime_A);
  GP_TRY_RC(gather_begin(dst, src, n, rows, 0));
  GP_LAUNCH(dst, dst->stream, move_embeddings_kernel, dim3(blocks_for(n * dst->Q)), dim3(256), 0, (const double*)src->Xmu, (const double*)src->Xs,
            (const long long*)dst->gather->idx, (long)n, dst->Q, 1, dst->Xmu, dst->Xs);
  GP_HIP(dst, hipStreamSynchronize(dst->stream));      // rows is the caller's again
  ++dst->sync_epoch;
  dst->life.embeddings_changed();
  return GP_OK;
}
