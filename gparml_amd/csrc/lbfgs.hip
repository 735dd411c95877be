// The resident L-BFGS history (gp_lbfgs_*): the limited-memory pairs of the training loop stay in HBM next to the vectors they are made from.
//
// Vector-free L-BFGS (Chen, Wang, Zhou: "Large-scale L-BFGS using MapReduce", NIPS 2014).  The two-loop recursion only ever needs inner products
// of the basis b = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g] (W = 2m + 1 vectors of n2 = 2 N_s Q doubles, laid out like grad_latest) and ends in one linear
// combination of it.  So the host keeps the W x W Gram matrix and runs the two loops on coefficients (gparml_amd/lbfgs.py); the device does, per
// iteration and whatever m is, ONE pass that refreshes the three rows of the matrix that changed (s and y of the newest pair, and g) and ONE pass
// that writes the new direction -- not 4 m dependent reductions with a host synchronisation each.
//   lb_push_kernel: s[slot] = step * dir, y[slot] = grad_latest - g, g = grad_latest in one sweep (one rounding each; 3 reads, 3 writes per element).
//   lb_dots_kernel<ROWS>: the rows [s[slot], y[slot], g] (ROWS = 3) or [g] (ROWS = 1) against a GROUP of up to LB_G basis vectors: 3 LB_G
//     accumulators in registers (3 W of them do not fit at m = 32), the rows re-read once per group, every basis vector read once per call.  A
//     workgroup takes one segment of LB_SEG = 8192 elements; thread t owns the element pairs 2 (t + 256 k), k = 0 .. 15, and adds their products in
//     ascending order, one fma each (a chain of 32); the 64 lanes of a wave are added by the xor butterfly 32, 16, .., 1 (6 levels), the four waves in
//     ascending order (3 additions); the result is the segment's partial [seg][row][column].  Only filled slots are put into groups: an empty slot is
//     never read.  A short last group repeats the pointer of g in its unused places (the same addresses the wave has just loaded as a row) and does
//     not write them.
//   lb_final_kernel: thread (row, column) adds the partials of its product over the segments in ASCENDING order and writes out[row][column]; a column
//     of an empty slot (and the s, y rows for slot = -1) is written as 0.0 without a read.  No floating-point atomics anywhere: the order of every sum is
//     a function of n2 alone, so a product has the same bits from run to run, on any device, for any m and any grouping (the accumulators of a group do
//     not interact).  The longest chain of a product is 32 + 6 + 3 + (segments - 1) additions.
//   lb_direction_kernel: dir = sum_j coef_j b_j over the active terms (filled, coef != 0) in ascending j: the first a product, each further one an fma.
// Work model at N_s = 1e6, Q = 10 (n2 = 2e7: 160 MB a vector): the dots pass reads the W basis vectors once and the three rows once per group --
// m = 10: (21 + 3 * 2) * 160 MB = 4.3 GB, of which the 3.4 GB of the basis are the floor; m = 32: (65 + 3 * 5) * 160 MB = 12.8 GB.  The direction pass
// reads the active vectors and writes one: (21 + 1) * 160 MB = 3.5 GB at m = 10.  The push moves 6 * 160 MB.  Both passes are memory-bound.
// The vectors belong to the context's LbfgsPlan (gp_lbfgs_begin .. gp_lbfgs_end; freed with the context).  They are DA_RAW (NaN-filled in the poison
// test mode): a vector is written by push / grad before the plan marks it filled, and only filled vectors are ever read.  Nothing of the evaluation
// is touched: grad_latest and the direction array are read, the direction array is written (Lifecycle::direction_rewritten, as gp_cg_update does).
#include "gp_common.h"
#include <cmath>
#include <cstring>

namespace gp {

constexpr int LB_MMAX = 32;       // pairs kept at most
constexpr int LB_SEG = 8192;      // elements per segment of a product: 256 threads x 16 pairs
constexpr int LB_G = 16;          // basis vectors per group of the dots pass
constexpr int LB_W = 2 * LB_MMAX + 1;
constexpr int LB_DSEG = 2048;     // elements per workgroup step of the direction pass: 256 threads x 4 pairs

struct LbfgsPlan {
  int m = 0;
  long n2 = 0;
  std::vector<DevBuf<double>> v;  // [2m+1][n2]: s_0 .. s_{m-1} | y_0 .. y_{m-1} | g
  unsigned long long filled = 0;  // bit k: slot k holds a pair
  bool has_g = false;
  DevBuf<double> part;            // [segments][3][2m+1] the partials of the dots pass
  DevBuf<double> out;             // [3][2m+1]
  int W() const { return 2 * m + 1; }
  long segs() const { return (n2 + LB_SEG - 1) / LB_SEG; }
};
void LbfgsPlanDelete::operator()(LbfgsPlan* p) const { delete p; }

struct LbDots {
  const double* row[3];           // s[slot], y[slot], g (ROWS = 1: only row[2])
  const double* b[LB_G];          // the group's vectors; unused places repeat g
  int col[LB_G];                  // their columns of the Gram rows; -1: unused
};

struct LbTerms {
  const double* p[LB_W];
  double c[LB_W];
  int cnt;
};

__global__ void __launch_bounds__(256) lb_push_kernel(long n2, double step, const double* __restrict__ dir, const double* __restrict__ glatest,
                                                      double* __restrict__ s, double* __restrict__ y, double* __restrict__ g) {
  const long pairs = n2 / 2;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < pairs; i += (long)gridDim.x * 256L) {
    const double2 d = reinterpret_cast<const double2*>(dir)[i], gl = reinterpret_cast<const double2*>(glatest)[i];
    const double2 go = reinterpret_cast<const double2*>(g)[i];
    reinterpret_cast<double2*>(s)[i] = make_double2(step * d.x, step * d.y);
    reinterpret_cast<double2*>(y)[i] = make_double2(gl.x - go.x, gl.y - go.y);
    reinterpret_cast<double2*>(g)[i] = gl;
  }
}

// one launch per group, grid (segments); part [segments][3][W]
template <int ROWS>
__global__ void __launch_bounds__(256) lb_dots_kernel(LbDots a, long n2, int W, double* __restrict__ part) {
  __shared__ double red[4][ROWS * LB_G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long base = (long)blockIdx.x * LB_SEG;
  double acc[ROWS][LB_G];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int j = 0; j < LB_G; ++j) acc[r][j] = 0.0;
  }
#pragma unroll 2
  for (int k = 0; k < LB_SEG / 512; ++k) {
    const long i = base + 2L * (tid + 256 * k);
    if (i < n2) {                                   // n2 is even: a pair is inside or outside as a whole
      double2 rv[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) rv[r] = *reinterpret_cast<const double2*>(a.row[3 - ROWS + r] + i);
      double2 bv[LB_G];
#pragma unroll
      for (int j = 0; j < LB_G; ++j) bv[j] = *reinterpret_cast<const double2*>(a.b[j] + i);
#pragma unroll
      for (int j = 0; j < LB_G; ++j) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r][j] = fma(rv[r].y, bv[j].y, fma(rv[r].x, bv[j].x, acc[r][j]));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int j = 0; j < LB_G; ++j) {
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) acc[r][j] += __shfl_xor(acc[r][j], sh);
      if (lane == 0) red[wave][r * LB_G + j] = acc[r][j];
    }
  }
  __syncthreads();
  if (tid < ROWS * LB_G) {
    const int r = tid / LB_G, j = tid % LB_G;
    const int col = a.col[j];
    if (col >= 0) part[((long)blockIdx.x * 3 + (3 - ROWS + r)) * W + col] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// one workgroup; thread t = row * W + column; live_s / live_y: the filled slots; rows: 3, or 1 (only the g row is summed)
__global__ void __launch_bounds__(256) lb_final_kernel(const double* __restrict__ part, long segs, int m, unsigned long long filled, int rows,
                                                       double* __restrict__ out) {
  const int W = 2 * m + 1, t = threadIdx.x;
  if (t >= 3 * W) return;
  const int r = t / W, col = t % W;
  const bool live = (rows == 3 || r == 2) && (col == 2 * m || ((filled >> (col < m ? col : col - m)) & 1ull));
  double s = 0.0;
  if (live) {
#pragma unroll 8
    for (long g = 0; g < segs; ++g) s += part[g * 3 * W + t];
  }
  out[t] = s;
}

__global__ void __launch_bounds__(256) lb_direction_kernel(LbTerms a, long n2, double* __restrict__ dir) {
  const long steps = (n2 + LB_DSEG - 1) / LB_DSEG;
  for (long st = blockIdx.x; st < steps; st += gridDim.x) {
    const long i0 = st * LB_DSEG + 2L * threadIdx.x;
    double2 acc[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { in[k] = i0 + 512L * k < n2; acc[k] = make_double2(0.0, 0.0); }
    for (int j = 0; j < a.cnt; ++j) {
      const double* p = a.p[j];
      const double cj = a.c[j];
      double2 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = in[k] ? *reinterpret_cast<const double2*>(p + i0 + 512L * k) : make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (j == 0) { acc[k].x = cj * v[k].x; acc[k].y = cj * v[k].y; }
        else { acc[k].x = fma(cj, v[k].x, acc[k].x); acc[k].y = fma(cj, v[k].y, acc[k].y); }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (in[k]) *reinterpret_cast<double2*>(dir + i0 + 512L * k) = acc[k];
  }
}

// gp_debug_peek: "lbfgs_s<k>", "lbfgs_y<k>" (a filled slot), "lbfgs_g" (once set)
const double* lbfgs_debug(const gp_ctx* c, const char* name, long* cnt) {
  *cnt = 0;
  if (!c->lbfgs) return nullptr;
  const LbfgsPlan& p = *c->lbfgs;
  const char* t = name + 6;          // behind "lbfgs_"
  int at = -1;
  if (!std::strcmp(t, "g")) { if (p.has_g) at = 2 * p.m; }
  else if ((t[0] == 's' || t[0] == 'y') && t[1] >= '0' && t[1] <= '9') {
    char* end = nullptr;
    const long k = std::strtol(t + 1, &end, 10);
    if (*end == 0 && k >= 0 && k < p.m && ((p.filled >> k) & 1ull)) at = (int)k + (t[0] == 'y' ? p.m : 0);
  }
  if (at < 0) return nullptr;
  *cnt = p.n2;
  return p.v[at];
}

// the rule of the resident vectors (cg.hip; gp_lbfgs_begin asks no more), then the plan's presence; *pp = the plan
static int lb_vectors_ready(gp_ctx* c, const char* who) { return resident_ready(c, who, "resident L-BFGS history exists"); }
static int lb_ready(gp_ctx* c, const char* who, LbfgsPlan** pp) {
  GP_TRY_RC(lb_vectors_ready(c, who));
  if (!c->lbfgs) return fail(c, GP_ERR_STATE, "%s before gp_lbfgs_begin (or after gp_lbfgs_end)", who);
  *pp = c->lbfgs.get();
  return GP_OK;
}

}  // namespace gp

using namespace gp;

extern "C" int gp_lbfgs_begin(gp_ctx* c, int m) {
  if (!c) return GP_ERR_BAD_ARG;
  if (m < 1 || m > LB_MMAX) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_begin: m must be 1 .. %d, got %d", LB_MMAX, m);
  GP_TRY_RC(lb_vectors_ready(c, "gp_lbfgs_begin"));
  GP_HIP(c, hipSetDevice(c->device));
  const long n2 = 2L * c->N * c->Q;
  if (!c->lbfgs || c->lbfgs->m != m || c->lbfgs->n2 != n2) {
    c->lbfgs.reset();                 // the old vectors go before the new ones come
    std::unique_ptr<LbfgsPlan, LbfgsPlanDelete> p(new LbfgsPlan());
    p->m = m;
    p->n2 = n2;
    p->v.resize((size_t)p->W());
    for (auto& b : p->v) GP_TRY_RC(b.alloc(c, (size_t)n2, DA_RAW));
    GP_TRY_RC(p->part.alloc(c, (size_t)(p->segs() * 3 * p->W()), DA_RAW));
    GP_TRY_RC(p->out.alloc(c, (size_t)(3 * p->W()), DA_RAW));
    c->lbfgs = std::move(p);
  }
  c->lbfgs->filled = 0;               // a plan that stays keeps its g: a restart drops the pairs, not the gradient they start from
  return GP_OK;
}

extern "C" int gp_lbfgs_end(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  if (!c->lbfgs) return fail(c, GP_ERR_STATE, "gp_lbfgs_end before gp_lbfgs_begin (or after gp_lbfgs_end)");
  GP_HIP(c, hipSetDevice(c->device));
  GP_HIP(c, hipStreamSynchronize(c->stream));      // nothing enqueued may still use the vectors
  ++c->sync_epoch;
  c->lbfgs.reset();
  return GP_OK;
}

extern "C" int gp_lbfgs_grad(gp_ctx* c) {
  if (!c) return GP_ERR_BAD_ARG;
  LbfgsPlan* p = nullptr;
  GP_TRY_RC(lb_ready(c, "gp_lbfgs_grad", &p));
  if (!c->life.has_grad_latest()) return fail(c, GP_ERR_STATE, "gp_lbfgs_grad: no grad_latest yet (gp_phase2(ctx, 1) first)");
  GP_HIP(c, hipSetDevice(c->device));
  GP_HIP(c, hipMemcpyAsync(p->v[2 * p->m], c->cg.g_latest, (size_t)p->n2 * 8, hipMemcpyDeviceToDevice, c->stream));
  p->has_g = true;
  return GP_OK;
}

extern "C" int gp_lbfgs_push(gp_ctx* c, int slot, double step) {
  if (!c) return GP_ERR_BAD_ARG;
  LbfgsPlan* p = nullptr;
  GP_TRY_RC(lb_ready(c, "gp_lbfgs_push", &p));
  if (slot < 0 || slot >= p->m) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_push: slot must be 0 .. %d, got %d", p->m - 1, slot);
  if (!std::isfinite(step)) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_push: step is not finite");
  if (!p->has_g) return fail(c, GP_ERR_STATE, "gp_lbfgs_push before gp_lbfgs_grad: there is no g to difference against");
  if (!c->life.has_direction()) return fail(c, GP_ERR_STATE, "gp_lbfgs_push: no search direction (gp_set_direction or gp_lbfgs_direction first)");
  if (!c->life.has_grad_latest()) return fail(c, GP_ERR_STATE, "gp_lbfgs_push: no grad_latest yet (gp_phase2(ctx, 1) first)");
  GP_HIP(c, hipSetDevice(c->device));
  GP_LAUNCH(c, c->stream, lb_push_kernel, dim3(blocks_for(p->n2 / 2)), dim3(256), 0, p->n2, step, c->dir, c->cg.g_latest, p->v[slot], p->v[p->m + slot],
            p->v[2 * p->m]);
  p->filled |= 1ull << slot;
  return GP_OK;
}

template <int ROWS>
static int lb_launch_dots(gp_ctx* c, const LbDots& a, const LbfgsPlan& p) {
  GP_LAUNCH(c, c->stream, lb_dots_kernel<ROWS>, dim3((unsigned)p.segs()), dim3(256), 0, a, p.n2, p.W(), p.part);
  return GP_OK;
}

extern "C" int gp_lbfgs_dots(gp_ctx* c, int slot, double* out) {
  if (!c) return GP_ERR_BAD_ARG;
  LbfgsPlan* pp = nullptr;
  GP_TRY_RC(lb_ready(c, "gp_lbfgs_dots", &pp));
  const LbfgsPlan& p = *pp;
  if (!out) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_dots: out is NULL");
  if (slot < -1 || slot >= p.m) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_dots: slot must be -1 .. %d, got %d", p.m - 1, slot);
  if (!p.has_g) return fail(c, GP_ERR_STATE, "gp_lbfgs_dots before gp_lbfgs_grad: g is not set");
  if (slot >= 0 && !((p.filled >> slot) & 1ull)) return fail(c, GP_ERR_STATE, "gp_lbfgs_dots: slot %d is empty (gp_lbfgs_push first)", slot);
  GP_HIP(c, hipSetDevice(c->device));
  const int m = p.m, W = p.W();
  const double* g = p.v[2 * m];
  // the columns that hold something, ascending: only they are read
  int cols[LB_W], nc = 0;
  for (int j = 0; j < W; ++j) if (j == 2 * m || ((p.filled >> (j < m ? j : j - m)) & 1ull)) cols[nc++] = j;
  for (int j0 = 0; j0 < nc; j0 += LB_G) {
    LbDots a;
    a.row[0] = slot >= 0 ? p.v[slot].get() : g;
    a.row[1] = slot >= 0 ? p.v[m + slot].get() : g;
    a.row[2] = g;
    for (int j = 0; j < LB_G; ++j) {
      const bool used = j0 + j < nc;
      a.b[j] = used ? p.v[cols[j0 + j]].get() : g;
      a.col[j] = used ? cols[j0 + j] : -1;
    }
    GP_TRY_RC(slot >= 0 ? lb_launch_dots<3>(c, a, p) : lb_launch_dots<1>(c, a, p));
  }
  GP_LAUNCH(c, c->stream, lb_final_kernel, dim3(1), dim3(256), 0, p.part, p.segs(), m, p.filled, slot >= 0 ? 3 : 1, p.out);
  GP_HIP(c, hipMemcpyAsync(out, p.out, (size_t)(3 * W) * 8, hipMemcpyDeviceToHost, c->stream));
  GP_HIP(c, hipStreamSynchronize(c->stream));
  ++c->sync_epoch;
  return GP_OK;
}

extern "C" int gp_lbfgs_direction(gp_ctx* c, const double* coef) {
  if (!c) return GP_ERR_BAD_ARG;
  LbfgsPlan* pp = nullptr;
  GP_TRY_RC(lb_ready(c, "gp_lbfgs_direction", &pp));
  const LbfgsPlan& p = *pp;
  if (!coef) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_direction: coef is NULL");
  const int m = p.m, W = p.W();
  for (int j = 0; j < W; ++j) if (!std::isfinite(coef[j])) return fail(c, GP_ERR_BAD_ARG, "gp_lbfgs_direction: coef[%d] is not finite", j);
  if (coef[2 * m] != 0.0 && !p.has_g) return fail(c, GP_ERR_STATE, "gp_lbfgs_direction before gp_lbfgs_grad: g is not set");
  GP_HIP(c, hipSetDevice(c->device));
  LbTerms a;
  a.cnt = 0;
  for (int j = 0; j < W; ++j) {
    const bool holds = j == 2 * m ? p.has_g : ((p.filled >> (j < m ? j : j - m)) & 1ull) != 0;
    if (holds && coef[j] != 0.0) { a.p[a.cnt] = p.v[j]; a.c[a.cnt] = coef[j]; ++a.cnt; }
  }
  for (int j = a.cnt; j < LB_W; ++j) { a.p[j] = nullptr; a.c[j] = 0.0; }
  const long steps = (p.n2 + LB_DSEG - 1) / LB_DSEG;
  GP_LAUNCH(c, c->stream, lb_direction_kernel, dim3((unsigned)std::min<long>(steps, 4096)), dim3(256), 0, a, p.n2, c->dir);
  c->life.direction_rewritten();
  return GP_OK;
}
