// The scoring passes as gp_predict_score (score.hip) and gp_loo_score (loo.hip) share them: the ONE definition of a scored entry's terms, of the
// row sums, of the column sums and of their totals on the host, so that the two entries round alike and sum in the same order by construction.
// An entry source says where the entries come from (PredSrc in score.hip, LooSrc in loo.hip; passed to kernels by value):
//   scored(row, d), term(row, d)    whether the entry enters the sums (a hidden entry is never read), and its ScoreTerm;
//   var(row, d), unfactorised(row)  the variance term() scores it under; the row has none at all (loo: its S did not factorise; else constant false);
//   rows, g0, D                     the rows of the column pass (a window that starts on a segment), the global index of the first, the columns;
//   NFLAGS                          1: first row with a variance that is not > 0; 2: and, behind it, the first unfactorised row.
// A row pass still holds its row's variance in a register and passes a source of its own, scored and term alone (PredRow, LooRow).
// Every body here that does floating-point arithmetic carries its own contract(off): the pragma is scoped to the compound statement it stands in and
// does not reach into what is inlined from elsewhere.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include "gp_common.h"
#include "lane_reduce.h"

namespace gp {

constexpr int SC_SEG = 128;       // rows per segment of the column sums (= TILE: a chunk of gp_predict is a whole number of segments)
constexpr int SC_DW = 128;        // columns per workgroup of the column pass
constexpr long long SC_NONE = LLONG_MAX;
static_assert(SC_SEG == TILE, "gp_predict's chunks are multiples of TILE rows: a segment never straddles two chunks");

struct ScoreTerm { double e, e2, q, lp; };
// the terms of one scored entry; NaN, all four, when the variance is not > 0
__device__ __forceinline__ ScoreTerm score_term(double y, double m, double v) {
#pragma clang fp contract(off)
  ScoreTerm t;
  t.e = y - m;
  t.e2 = t.e * t.e;
  t.q = t.e2 / v;
  t.lp = -0.5 * (log(6.283185307179586476925286766559 * v) + t.q);
  if (!(v > 0.0)) t.e = t.e2 = t.q = t.lp = __builtin_nan("");
  return t;
}

// |a|^2 and |b|^2 of a row g of G = [mean (Dp) | a = Lk^-1 k (Mp) | b = La^-1 k (Mp)], by one wave: lane l takes i = l, l + 64, .. in ascending order,
// then the xor butterfly (wave_sum); the same bits in every lane.  gp_predict's variance and both scorers' are built from this pair.
struct FacNorms { double a2, b2; };
__device__ __forceinline__ FacNorms fac_norms(const double* g, int M, int Dp, int Mp, int lane) {
#pragma clang fp contract(off)
  double sa = 0.0, sb = 0.0;
  for (int i = lane; i < M; i += 64) {
    const double a = g[Dp + i], b = g[Dp + Mp + i];
    sa = fma(a, a, sa);
    sb = fma(b, b, sb);
  }
  return {wave_sum(sa), wave_sum(sb)};
}

// the three sums of a row over its scored entries, by one wave: lane l adds d = l, l + 64, .. in ascending order, then the xor butterfly -- an order
// that is a function of D alone
struct RowSums { double lp, sse, chi; };
template <class RowSrc>
__device__ __forceinline__ RowSums score_row_sums(const RowSrc& src, long row, int D, int lane) {
#pragma clang fp contract(off)
  double lp = 0.0, sse = 0.0, chi = 0.0;
  for (int d = lane; d < D; d += 64) {
    if (!src.scored(row, d)) continue;
    const ScoreTerm t = src.term(row, d);
    lp += t.lp;
    sse += t.e2;
    chi += t.q;
  }
  return {wave_sum(lp), wave_sum(sse), wave_sum(chi)};
}

// grid (segments of src's rows, ceil(D / SC_DW)), 256 threads.  The per-entry terms are RECOMPUTED from the inputs the row pass had, by the same
// function, rather than stored by it: four n x D arrays less to write and read.  Thread (column cc, half h) adds the rows 64 h .. 64 h + 63 of the
// segment in ascending order, the halves are added as half 0 + half 1: part [segment][D][5] = count | sum e | sum e2 | sum q | sum lp (a scored
// entry whose variance is not > 0 puts its NaN into all five).  bad [segment][tile][NFLAGS]: the first such row among the factorised ones, the first
// unfactorised row (whether or not an entry of it is scored); SC_NONE without one.
template <class Src>
__global__ void __launch_bounds__(256) score_cols_kernel(Src a, double* part, long long* bad) {
#pragma clang fp contract(off)
  constexpr int NF = Src::NFLAGS;
  __shared__ double sh[5 * SC_DW];
  __shared__ long long fb[NF][256];
  const int tid = threadIdx.x, cc = tid & (SC_DW - 1), half = tid >> 7;
  const int d = blockIdx.y * SC_DW + cc;
  const long r0 = (long)blockIdx.x * SC_SEG + 64L * half;
  const long r1 = min(r0 + 64, a.rows), g0 = a.g0;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long first = SC_NONE, firstunf = SC_NONE;
  if (d < a.D) {
    for (long i = r0; i < r1; ++i) {
      const auto unf = a.unfactorised(i);             // loaded first, looked at last: the load overlaps the entry's
      if (a.scored(i, d)) {
        const double v = a.var(i, d);
        const ScoreTerm t = a.term(i, d);
        s[0] += (v > 0.0) ? 1.0 : t.e;
        s[1] += t.e;
        s[2] += t.e2;
        s[3] += t.q;
        s[4] += t.lp;
        if (!(v > 0.0) && !unf && first == SC_NONE) first = g0 + i;
      }
      if (unf && firstunf == SC_NONE) firstunf = g0 + i;
    }
  }
  fb[0][tid] = first;
  if (NF > 1) fb[NF - 1][tid] = firstunf;
  if (half == 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[k * SC_DW + cc] = s[k];
  }
  __syncthreads();
  if (half == 0 && d < a.D) {
    double* out = part + ((long)blockIdx.x * a.D + d) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = s[k] + sh[k * SC_DW + cc];
  }
  block_fold<256>([&](int i, int j) {
    fb[0][i] = min(fb[0][i], fb[0][j]);
    if (NF > 1) fb[NF - 1][i] = min(fb[NF - 1][i], fb[NF - 1][j]);
  });
  if (tid < NF) bad[NF * ((long)blockIdx.x * gridDim.y + blockIdx.y) + tid] = fb[tid][0];
}

// The column totals of a call and their owner on the host (functions: score.hip).  The running totals take the segments one by one in ascending
// order, the first segment of a call is added to zero: the ORDER of the column sums depends on the global row index alone.  Every element is written
// before it is read (DA_RAW): part and bad by the column kernel for the segments the final kernel then reads, tot and the call's flags by the final
// kernel, which starts them afresh at a call's first segments.
struct ScoreTotals {
  DevBuf<double> part;        // [segments][D][5]
  DevBuf<double> tot;         // [D][5]
  DevBuf<long long> bad;      // [segments][tiles][flags] | [flags] the call's first bad rows
  long D = 0;
  int tiles = 0, flags = 0;
  long long* call_flags() const { return bad + (bad.size() - (size_t)flags); }
  int alloc(gp_ctx* c, long segments, long D_, int flags_);            // room for `segments` segments per add_segments
  int fold(gp_ctx* c, hipStream_t st, int segs, bool first) const;     // score_cols_final_kernel: tot (first: zero) += the partials of segs segments
  // the first segs segments of src's rows into the totals
  template <class Src>
  int add_segments(gp_ctx* c, hipStream_t st, const Src& src, int segs, bool first) const {
    GP_LAUNCH(c, st, score_cols_kernel<Src>, dim3((unsigned)segs, (unsigned)tiles), dim3(256), 0, src, part.get(), bad.get());
    return fold(c, st, segs, first);
  }
  // tot -> cols [D][5] (NULL: not wanted) and the call's flags -> out[flags], and the stream is synchronised: the end of a scoring call
  int read(gp_ctx* c, hipStream_t st, double* cols, long long* out) const;
};
// GP_ERR_NON_FINITE of `entry`: a scored entry's variance (`which` one) is not > 0, first in `row`
int score_fail_variance(gp_ctx* c, const char* entry, const char* which, long long row, int flags);

}  // namespace gp
