// The terms of one scored entry and the geometry of the column sums, as gp_predict_score (score.hip) and gp_loo_score (loo.hip) share them: one
// definition of the operation order, so that the two entries round alike.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include "gp_common.h"

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

}  // namespace gp
