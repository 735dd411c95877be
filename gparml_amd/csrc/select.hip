// Greedy conditional-variance selection of the inducing points on the device (gp_select_begin / run / candidate / apply / end): the pivoted Cholesky
// factorisation of K_nn (Burt, Rasmussen and van der Wilk 2019), one pivot per step.
//
// State per row n: d_n, the conditional variance given the pivots so far (start: sf2), and the row of the factor L_n[0 .. j).  Step j with pivot p:
//   c_n = (k(x_n, x_p) - sum_{i<j} L_ni L_pi) / sqrt(d_p),   L_nj = c_n,   d_n <- d_n - c_n^2
// with k(x, z) = sf2 exp(-1/2 sum_q alpha_q (x_q - z_q)^2): the difference first, q ascending, one fma per term, fexp; the sum over i ascending from 0 with
// one fma per term; the update of d in one fma.  A row's L and d depend on that row and on the pivot's data (x_p, L_p[0 .. j), d_p) only.
//   sel_update_kernel<QT>: the hot kernel.  L is column-major [K][npad], so the lanes of a wave -- rows -- read consecutive addresses for each i; a lane
//     owns the two adjacent rows 2 t, 2 t + 1, so every load and store of L and d is 16 bytes.  The pivot's data is wave-uniform: it comes from the
//     pivot record [alpha (QS) | d_p, 0 | x_p (QS) | L_p (K)] through scalar loads (the record is read-only in this kernel).  QT: compile-time row
//     width as in km_assign_kernel (the record's padding coordinates and alphas are exact zeros); QT = 0: a run-time Q.  Ends with the workgroup's
//     partial (largest d among the unselected rows, of equal ones the lowest row) and its trace partial sum max(d, 0) over the unselected rows (LDS
//     tree, fixed order).
//   sel_reduce_kernel: one workgroup; thread t folds the partials t, t + 256, .. in ascending order, then an LDS tree: the next candidate (d, row)
//     and the trace after the step.  No floating-point atomics anywhere.
//   sel_pivot_kernel: gathers the candidate's (d, x, L row) into the pivot record, marks the row selected, records it; or raises the stop flag
//     (d_p <= tol sf2, or no unselected row), which every later kernel of the call respects: gp_select_run has no host round trip per step.
// gp_select_apply writes the record from the host instead and runs the same update and reduce kernels: the same bits.
// Every buffer belongs to the context's SelPlan (built aside, published whole, freed with the context or by gp_select_end); all of them are written
// before they are read (DA_RAW).  Nothing of the evaluation is touched: only the resident X_mu is read (X == NULL).
#include "gp_common.h"
#include "fexp.h"
#include "lane_reduce.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace gp {

constexpr int SEL_ROWS = 512;     // rows per workgroup of the update kernel (256 lanes, two rows each)
enum { SEL_CAND = 0, SEL_STOP = 1, SEL_DONE = 2, SEL_CTL = 4 };    // ctl: the candidate's row (-1: none) | the stop flag | steps done | (unused)

// d = sf2, the padding rows marked as selected, the first candidate (row 0 with d = sf2; none without rows)
__global__ void __launch_bounds__(256) sel_init_kernel(double* __restrict__ d, unsigned char* __restrict__ mark, long n, long npad, double sf2,
                                                       double* __restrict__ best, long long* __restrict__ ctl) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < npad; r += (long)gridDim.x * 256L) { d[r] = sf2; mark[r] = r < n ? 0 : 1; }
  if (blockIdx.x == 0 && threadIdx.x == 0) { best[0] = sf2; ctl[SEL_CAND] = n > 0 ? 0 : -1; ctl[SEL_STOP] = 0; ctl[SEL_DONE] = 0; ctl[3] = 0; }
}

// (d, row) a replaces b when larger, or equal with the lower row: the rule of every level
__device__ __forceinline__ bool sel_better(double da, long long ia, double db, long long ib) { return da > db || (da == db && ia < ib); }

// rec = [alpha (QS) | d_p, 0 | x_p (QS) | L_p (K)]; L [K][npad]; d [npad]; mark [npad]; pd, pi, pt [gridDim.x]
template <int QT>
__global__ void __launch_bounds__(256) sel_update_kernel(const double* __restrict__ X, const double* __restrict__ rec, const long long* __restrict__ ctl,
                                                         const unsigned char* __restrict__ mark, double* __restrict__ L, double* __restrict__ d, long n,
                                                         long npad, int Q, int QS, int j, double sf2, double* __restrict__ pd, long long* __restrict__ pi,
                                                         double* __restrict__ pt) {
  __shared__ double red_d[256];
  __shared__ double red_t[256];
  __shared__ long long red_i[256];
  if (ctl[SEL_STOP]) return;
  const int tid = threadIdx.x;
  const long r0 = (blockIdx.x * 256L + tid) * 2;
  double bd = -std::numeric_limits<double>::infinity(), tr = 0.0;
  long long bi = -1;
  if (r0 < npad) {            // npad is even: the lane's two rows exist in L, d and mark
    const double* xa = X + (r0 < n ? r0 : n - 1) * Q;
    const double* xb = X + (r0 + 1 < n ? r0 + 1 : n - 1) * Q;        // a padding row repeats the last row: finite, never a candidate
    const double* al = rec;
    const double dp = rec[QS];
    const double* z = rec + QS + 2;
    const double* lp = z + QS;
    double s0 = 0.0, s1 = 0.0;
    if constexpr (QT > 0) {
      constexpr int UNROLL = QT > 16 ? 8 : QT;      // the wide rows in groups of eight coordinates: unrolled whole they take every register
#pragma unroll UNROLL
      for (int q = 0; q < QT; ++q) {
        const double a = al[q], zq = z[q];
        const double e0 = (q < Q ? xa[q] : 0.0) - zq, e1 = (q < Q ? xb[q] : 0.0) - zq;
        s0 = fma(a * e0, e0, s0);
        s1 = fma(a * e1, e1, s1);
      }
    } else {
      for (int q = 0; q < Q; ++q) {
        const double a = al[q], zq = z[q];
        const double e0 = xa[q] - zq, e1 = xb[q] - zq;
        s0 = fma(a * e0, e0, s0);
        s1 = fma(a * e1, e1, s1);
      }
    }
    const double k0 = sf2 * fexp(-0.5 * s0), k1 = sf2 * fexp(-0.5 * s1);
    const double2* col = reinterpret_cast<const double2*>(L + r0);
    const long stride = npad / 2;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
    for (int i = 0; i < j; ++i) {
      const double2 v = col[i * stride];
      const double l = lp[i];
      a0 = fma(v.x, l, a0);
      a1 = fma(v.y, l, a1);
    }
    const double root = sqrt(dp);
    const double c0 = (k0 - a0) / root, c1 = (k1 - a1) / root;
    const double2 dv = *reinterpret_cast<const double2*>(d + r0);
    const double d0 = fma(-c0, c0, dv.x), d1 = fma(-c1, c1, dv.y);
    *reinterpret_cast<double2*>(L + (long)j * npad + r0) = make_double2(c0, c1);
    *reinterpret_cast<double2*>(d + r0) = make_double2(d0, d1);
    const unsigned short mm = *reinterpret_cast<const unsigned short*>(mark + r0);
    if (!(mm & 0xff)) { bd = d0; bi = r0; tr = fmax(d0, 0.0); }
    if (!(mm >> 8)) {
      if (sel_better(d1, r0 + 1, bd, bi) || bi < 0) { bd = d1; bi = r0 + 1; }
      tr += fmax(d1, 0.0);
    }
  }
  red_d[tid] = bd; red_i[tid] = bi; red_t[tid] = tr;
  __syncthreads();
  block_fold<256>([&](int a, int b) {
    if (red_i[b] >= 0 && (red_i[a] < 0 || sel_better(red_d[b], red_i[b], red_d[a], red_i[a]))) { red_d[a] = red_d[b]; red_i[a] = red_i[b]; }
    red_t[a] += red_t[b];
  });
  if (tid == 0) { pd[blockIdx.x] = red_d[0]; pi[blockIdx.x] = red_i[0]; pt[blockIdx.x] = red_t[0]; }
}

// the partials of `blocks` workgroups -> the candidate (best[0], ctl[SEL_CAND]) and trace[j]
__global__ void __launch_bounds__(256) sel_reduce_kernel(const double* __restrict__ pd, const long long* __restrict__ pi, const double* __restrict__ pt,
                                                         int blocks, int j, double* __restrict__ best, long long* __restrict__ ctl,
                                                         double* __restrict__ trace) {
  __shared__ double red_d[256];
  __shared__ double red_t[256];
  __shared__ long long red_i[256];
  if (ctl[SEL_STOP]) return;
  const int tid = threadIdx.x;
  double bd = -std::numeric_limits<double>::infinity(), tr = 0.0;
  long long bi = -1;
  for (int g = tid; g < blocks; g += 256) {
    const long long i = pi[g];
    if (i >= 0 && (bi < 0 || sel_better(pd[g], i, bd, bi))) { bd = pd[g]; bi = i; }
    tr += pt[g];
  }
  red_d[tid] = bd; red_i[tid] = bi; red_t[tid] = tr;
  __syncthreads();
  block_fold<256>([&](int a, int b) {
    if (red_i[b] >= 0 && (red_i[a] < 0 || sel_better(red_d[b], red_i[b], red_d[a], red_i[a]))) { red_d[a] = red_d[b]; red_i[a] = red_i[b]; }
    red_t[a] += red_t[b];
  });
  if (tid == 0) { best[0] = red_d[0]; ctl[SEL_CAND] = red_i[0]; trace[j] = red_t[0]; }
}

// The candidate's data into the pivot record.  commit = 1 (gp_select_run): stop -- for this and every later kernel of the call -- when there is no
// candidate or its d is not above thr = tol sf2; else mark the row, record it as pivot j and count the step.  commit = 0 (gp_select_candidate): the
// record only (nothing is written without a candidate).
__global__ void __launch_bounds__(256) sel_pivot_kernel(const double* __restrict__ X, const double* __restrict__ L, const double* __restrict__ best,
                                                        long long* __restrict__ ctl, unsigned char* __restrict__ mark, double* __restrict__ rec,
                                                        long long* __restrict__ rows, long npad, int Q, int QS, int j, double thr, int commit) {
  __shared__ long long sp;
  __shared__ int go;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const long long p = ctl[SEL_CAND];
    const double dp = best[0];
    sp = p;
    go = p >= 0 && !(commit && (ctl[SEL_STOP] || !(dp > thr)));
    if (!go && commit) ctl[SEL_STOP] = 1;
    if (go) {
      rec[QS] = dp; rec[QS + 1] = 0.0;
      if (commit) { mark[p] = 1; rows[j] = p; ctl[SEL_DONE] = j + 1; }
    }
  }
  __syncthreads();
  if (!go) return;
  const long long p = sp;
  double* z = rec + QS + 2;
  for (int q = tid; q < QS; q += 256) z[q] = q < Q ? X[p * Q + q] : 0.0;
  for (int i = tid; i < j; i += 256) z[QS + i] = L[(long)i * npad + p];
}

// test hook (gp_debug_set_option "select_rows"): host rows per upload chunk of gp_select_begin (any k >= 1); 0 = the default below
std::atomic<int> g_opt_sel_rows{0};

struct SelPlan {
  long n = 0, npad = 0;       // rows, and rounded up to 64 (the columns of L stay 512-byte aligned)
  int K = 0, j = 0, QT = 0, QS = 0, blocks = 0;
  double sf2 = 0, thr = 0;    // thr = tol sf2: a pivot needs d above it
  bool resident = false;      // the rows are the context's X_mu (which must not change before gp_select_end)
  DevBuf<double> X;           // [n][Q] host rows
  DevBuf<double> L;           // [K][npad] the factor, column-major
  DevBuf<double> d;           // [npad] conditional variances
  DevBuf<unsigned char> mark; // [npad] 1: selected (or padding)
  DevBuf<double> rec;         // [QS | 2 | QS | K] alpha | d_p, 0 | x_p | L_p: the pivot record
  DevBuf<double> best;        // [1] the candidate's d
  DevBuf<long long> ctl;      // [SEL_CTL]
  DevBuf<long long> rows;     // [K] the pivots of gp_select_run
  DevBuf<double> trace;       // [K] the trace after every step
  DevBuf<double> pd, pt;      // [blocks] per-workgroup partials
  DevBuf<long long> pi;
};
void SelPlanDelete::operator()(SelPlan* p) const { delete p; }

long select_bytes(const gp_ctx* c, long n, int K, bool host_rows) {
  const long npad = round_up(std::max<long>(n, 1), 64), QS = psi1_qp(c->Q) > 0 ? psi1_qp(c->Q) : c->Q;
  return 8 * ((long)K * npad + npad + (host_rows ? n * c->Q : 0) + 2 * QS + 2 + 3L * K + 3 * (npad / SEL_ROWS + 1) + 8) + npad;
}

int run_select_begin(gp_ctx* c, long n, const double* X, int K, double sf2, const double* alpha, double tol) {
  const long Q = c->Q;
  hipStream_t st = c->stream;
  std::unique_ptr<SelPlan, SelPlanDelete> np(new SelPlan());
  SelPlan& p = *np;
  p.n = n; p.npad = round_up(std::max<long>(n, 1), 64); p.K = K; p.sf2 = sf2; p.thr = tol * sf2; p.resident = X == nullptr;
  p.QT = psi1_qp((int)Q); p.QS = p.QT > 0 ? p.QT : (int)Q;
  p.blocks = (int)((p.npad + SEL_ROWS - 1) / SEL_ROWS);
  if (X) GP_TRY_RC(p.X.alloc(c, (size_t)std::max<long>(n * Q, 1), DA_RAW));
  GP_TRY_RC(p.L.alloc(c, (size_t)K * p.npad, DA_RAW));
  GP_TRY_RC(p.d.alloc(c, (size_t)p.npad, DA_RAW));
  GP_TRY_RC(p.mark.alloc(c, (size_t)p.npad, DA_RAW));
  GP_TRY_RC(p.rec.alloc(c, (size_t)(2 * p.QS + 2 + K), DA_RAW));
  GP_TRY_RC(p.best.alloc(c, 1, DA_RAW));
  GP_TRY_RC(p.ctl.alloc(c, SEL_CTL, DA_RAW));
  GP_TRY_RC(p.rows.alloc(c, (size_t)K, DA_RAW));
  GP_TRY_RC(p.trace.alloc(c, (size_t)K, DA_RAW));
  GP_TRY_RC(p.pd.alloc(c, (size_t)p.blocks, DA_RAW));
  GP_TRY_RC(p.pt.alloc(c, (size_t)p.blocks, DA_RAW));
  GP_TRY_RC(p.pi.alloc(c, (size_t)p.blocks, DA_RAW));
  std::vector<double> ha((size_t)p.QS, 0.0);
  std::copy(alpha, alpha + Q, ha.begin());
  GP_HIP(c, hipMemcpyAsync(p.rec, ha.data(), ha.size() * 8, hipMemcpyHostToDevice, st));
  if (X && n > 0) {
    const int opt = g_opt_sel_rows.load();
    const long R = opt > 0 ? opt : std::max<long>(1, (64L << 20) / (8 * Q));      // a chunk of host rows stays near 64 MB
    for (long n0 = 0; n0 < n; n0 += R) {
      const long cnt = std::min(R, n - n0);
      GP_HIP(c, hipMemcpyAsync(p.X + n0 * Q, X + n0 * Q, (size_t)(cnt * Q) * 8, hipMemcpyHostToDevice, st));
    }
  }
  GP_LAUNCH(c, st, sel_init_kernel, dim3(blocks_for(p.npad)), dim3(256), 0, p.d, p.mark, n, p.npad, sf2, p.best, p.ctl);
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  c->sel = std::move(np);
  return GP_OK;
}

template <int QT>
static int sel_launch_update(gp_ctx* c, hipStream_t st, SelPlan& p, const double* X, int j) {
  GP_LAUNCH(c, st, sel_update_kernel<QT>, dim3((unsigned)p.blocks), dim3(256), 0, X, p.rec, p.ctl, p.mark, p.L, p.d, p.n, p.npad, c->Q, p.QS, j, p.sf2,
            p.pd, p.pi, p.pt);
  return GP_OK;
}

// step j's update and the reduction behind it (the pivot record is in place)
static int sel_step(gp_ctx* c, hipStream_t st, SelPlan& p, const double* X, int j) {
  // (width 0: the kernel with a run-time Q, beyond the 64-wide records)
  GP_TRY_RC((for_width<2, 4, 6, 8, 10, 12, 14, 16, 24, 32, 52, 64, 0>(c, "selection update kernel", p.QT, [&](auto W) {
    return sel_launch_update<W()>(c, st, p, X, j);
  })));
  GP_LAUNCH(c, st, sel_reduce_kernel, dim3(1), dim3(256), 0, p.pd, p.pi, p.pt, p.blocks, j, p.best, p.ctl, p.trace);
  return GP_OK;
}

static const double* sel_rows_of(const gp_ctx* c, const SelPlan& p) { return p.resident ? c->Xmu.get() : p.X.get(); }

int run_select_run(gp_ctx* c, int steps, int32_t* n_done, int64_t* rows, double* trace) {
  SelPlan& p = *c->sel;
  hipStream_t st = c->stream;
  const int j0 = p.j, todo = p.n > 0 ? std::min(steps, p.K - j0) : 0;
  *n_done = 0;
  if (todo <= 0) return GP_OK;
  const double* X = sel_rows_of(c, p);
  const long long head[2] = {0, (long long)j0};      // the stop flag of this call | steps done
  GP_HIP(c, hipMemcpyAsync(p.ctl + SEL_STOP, head, sizeof(head), hipMemcpyHostToDevice, st));
  for (int j = j0; j < j0 + todo; ++j) {
    GP_LAUNCH(c, st, sel_pivot_kernel, dim3(1), dim3(256), 0, X, p.L, p.best, p.ctl, p.mark, p.rec, p.rows, p.npad, c->Q, p.QS, j, p.thr, 1);
    GP_TRY_RC(sel_step(c, st, p, X, j));
  }
  long long done = j0;
  std::vector<long long> hr((size_t)todo);
  std::vector<double> ht((size_t)todo);
  GP_HIP(c, hipMemcpyAsync(&done, p.ctl + SEL_DONE, 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipMemcpyAsync(hr.data(), p.rows + j0, (size_t)todo * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipMemcpyAsync(ht.data(), p.trace + j0, (size_t)todo * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  const int got = (int)(done - j0);
  for (int s = 0; s < got; ++s) {
    if (rows) rows[s] = (int64_t)hr[(size_t)s];
    if (trace) trace[s] = ht[(size_t)s];
  }
  p.j = j0 + got;
  *n_done = got;
  return GP_OK;
}

int run_select_candidate(gp_ctx* c, double* d, int64_t* row, double* x, double* l) {
  SelPlan& p = *c->sel;
  hipStream_t st = c->stream;
  *d = -std::numeric_limits<double>::infinity();
  *row = -1;
  if (p.n == 0) return GP_OK;
  const double* X = sel_rows_of(c, p);
  GP_LAUNCH(c, st, sel_pivot_kernel, dim3(1), dim3(256), 0, X, p.L, p.best, p.ctl, p.mark, p.rec, p.rows, p.npad, c->Q, p.QS, p.j, p.thr, 0);
  long long cand = -1;
  std::vector<double> h((size_t)(2 + p.QS + p.j));
  GP_HIP(c, hipMemcpyAsync(&cand, p.ctl + SEL_CAND, 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipMemcpyAsync(h.data(), p.rec + p.QS, h.size() * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  if (cand < 0) return GP_OK;       // every row is selected: the record was not written
  *d = h[0];
  *row = (int64_t)cand;
  if (x) std::copy(h.begin() + 2, h.begin() + 2 + c->Q, x);
  if (l) std::copy(h.begin() + 2 + p.QS, h.end(), l);
  return GP_OK;
}

int run_select_apply(gp_ctx* c, const double* x_p, const double* l_p, double d_p, int64_t own_row, double* trace) {
  SelPlan& p = *c->sel;
  hipStream_t st = c->stream;
  const int j = p.j;
  if (p.n > 0) {
    std::vector<double> h((size_t)(2 + p.QS + j), 0.0);
    h[0] = d_p;
    std::copy(x_p, x_p + c->Q, h.begin() + 2);
    if (j > 0) std::copy(l_p, l_p + j, h.begin() + 2 + p.QS);
    const long long go = 0;
    GP_HIP(c, hipMemcpyAsync(p.rec + p.QS, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
    GP_HIP(c, hipMemcpyAsync(p.ctl + SEL_STOP, &go, 8, hipMemcpyHostToDevice, st));
    if (own_row >= 0) GP_HIP(c, hipMemsetAsync(p.mark + own_row, 1, 1, st));
    GP_TRY_RC(sel_step(c, st, p, sel_rows_of(c, p), j));
    double t = 0.0;
    GP_HIP(c, hipMemcpyAsync(&t, p.trace + j, 8, hipMemcpyDeviceToHost, st));
    GP_HIP(c, hipStreamSynchronize(st));
    ++c->sync_epoch;
    if (trace) *trace = t;
  } else if (trace) {
    *trace = 0.0;
  }
  p.j = j + 1;
  return GP_OK;
}

// what the entry points check before they run: rows, steps wanted and steps done of the plan (api.hip)
void select_info(const gp_ctx* c, long* n, int* K, int* j) { *n = c->sel->n; *K = c->sel->K; *j = c->sel->j; }

// gp_debug_peek: "select_L" = the columns written so far, [j][npad]; "select_d" = [npad]; NULL / 0 without a plan
const double* select_debug(const gp_ctx* c, bool want_L, long* cnt) {
  *cnt = 0;
  if (!c->sel) return nullptr;
  *cnt = want_L ? (long)c->sel->j * c->sel->npad : c->sel->npad;
  return want_L ? c->sel->L.get() : c->sel->d.get();
}

}  // namespace gp
