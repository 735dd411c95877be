// The start of latent inference on the device (gp_nearest_rows): per new row the nearest training row.
//
// predict.test places every new point at the trained embedding of the training output nearest to it (predict.py:44-66), searched on the host with a
// k-d tree per shard -- at D = 100 .. 1000 a brute-force search in disguise, over host copies of rows that are resident in every engine.  The search
// has the map-reduce shape of everything else here: a shard yields per new row its least squared distance and the row that has it, the minimum over
// shards and ranks wins (gparml_amd/init.py: nearest_start).
//   nn_search_kernel: workgroup = (block of NN_NY new rows) x (slice of training rows).  Training rows are lanes: a tile of 256 rows x NN_CT observed
//     columns passes through LDS transposed (coalesced reads of Y along a row, then every thread reads its own row without bank conflicts; the
//     next tile is fetched into registers while this one is used).  The new rows are a register block of NN_NY accumulators per thread; their
//     values, stored [block][column][row of the block], are wave-uniform reads.  Columns are streamed in tiles, so any D works.  The distance is the
//     direct form sum_j (y[cols[j]] - t[cols[j]])^2, j ascending, one fma per term (never |y|^2 - 2 y.t + |t|^2: at near-ties its cancellation
//     decides the row, kmeans.hip).  A thread walks its rows in ascending order and keeps its running best in registers; a row replaces the best
//     only when strictly nearer.  Across the lanes of a wave and the waves of the workgroup the pairs (distance, row) are compared: an equally
//     near row replaces the best only when its index is lower -- a lane's best need not lie below its neighbour's.  Out: one partial per
//     (slice, new row).  The padded rows [N, Np) of Kaug are never read, nor any column outside cols (the Psi1 columns among them).
//     nn_search_kernel<true> (gp_nearest_rows_masked) is the same kernel for new rows that each observe their own columns: two wave-uniform
//     values per (column, new row) instead of one, the same two operations per term, the same bits over the observed columns of a row.
//   nn_reduce_kernel: folds the slices in ascending order onto the running best of the call (set by the first chunk of training rows): strictly
//     nearer only, so the lowest row wins across workgroups and chunks too.  No atomics anywhere; the result does not depend on the slicing.
//   nn_gather_kernel: the base means Xmu[row] of the winners (resident rows only).
// New rows are taken in chunks, and so are host training rows; the slice count follows the grid (about NN_BLOCKS workgroups), so the partials are
// [slices][rows of the chunk] -- kilobytes, whatever N is.  Every buffer belongs to the context's NnPlan (allocated on first use, grown on demand,
// freed with the context) and is written before it is read (DA_RAW).  Nothing of the evaluation is touched: only Kaug's Y columns and Xmu are read.
#include "gp_common.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace gp {

constexpr int NN_NY = 16;         // new rows per workgroup: the register block of accumulators
constexpr int NN_CT = 16;         // observed columns per LDS tile
constexpr int NN_ROWS = 256;      // training rows per LDS tile: one per thread
constexpr int NN_RS = 260;        // the tile's row stride (256 rows + 4: the transposing stores are 2-way conflicts instead of 16-way)
constexpr int NN_BLOCKS = 2048;   // workgroups a launch aims at: the slices of the training rows make up what the blocks of new rows leave

// (od, oi) replaces (d, i) when nearer, or equally near with a lower row (no row yet: -1, the largest unsigned)
__device__ __forceinline__ void nn_take(double& d, int& i, double od, int oi) {
  if (od < d || (od == d && (unsigned)oi < (unsigned)i)) { d = od; i = oi; }
}

// T [cnt][ld] (column 0 = the first data column); Yb [gridDim.x][ncp][NN_NY] (zero beyond n_cols and beyond the call's rows); cols [ncp] (zero
// beyond n_cols); pd, pi [gridDim.y][ry]: per slice and new row the least distance and its row of T (-1, +inf: none)
// MASKED (gp_nearest_rows_masked: every new row has its own observed set): Yb [gridDim.x][ncp][2][NN_NY], per column the rows' wy = o ? y : 0, then
// their nw = o ? -1 : -0.0 (both zero beyond n_cols and beyond the call's rows).  The difference is fma(nw, t, wy): y - t rounded once where
// the row observes the column -- the bits of the other form -- and an exact zero where it does not (t is finite), which leaves the sum as it is.
template <bool MASKED>
__global__ void __launch_bounds__(256) nn_search_kernel(const double* __restrict__ T, long ld, long cnt, int tps, const double* __restrict__ Yb,
                                                        const int* __restrict__ cols, int n_cols, int ncp, long ry, double* __restrict__ pd,
                                                        int* __restrict__ pi) {
  __shared__ double tile[NN_CT * NN_RS];
  __shared__ double red_d[4][NN_NY];
  __shared__ int red_i[4][NN_NY];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sj = tid & (NN_CT - 1), sr = tid >> 4;        // staging: this thread's column of the tile, and its row among 16
  constexpr int YS = MASKED ? 2 * NN_NY : NN_NY;          // doubles of Yb per column
  const double* y = Yb + (long)blockIdx.x * ncp * YS;
  const long tiles = (cnt + NN_ROWS - 1) / NN_ROWS;
  const long t0 = (long)blockIdx.y * tps, t1 = min(tiles, t0 + tps);      // t0 < t1: the grid has no empty slice
  const int nct = ncp / NN_CT;

  double best[NN_NY], acc[NN_NY];
  int bi[NN_NY];
#pragma unroll
  for (int i = 0; i < NN_NY; ++i) { best[i] = std::numeric_limits<double>::infinity(); bi[i] = -1; acc[i] = 0.0; }

  double f[NN_ROWS / 16];
  // column tile ct of row tile t into registers: 16 lanes read 16 columns of one row.  The loads of a row at or beyond cnt and of a column at or
  // beyond n_cols are redirected to the last row and to column cols[0] (no branches: the sixteen loads are in flight together), so nothing
  // outside the rows [0, cnt) and the columns of cols is ever read; put() replaces what they fetched by exact zeros, on both sides of the difference
  auto fetch = [&](long t, int ct) {
    const int col = ct * NN_CT + sj;
    const long c = cols[col < n_cols ? col : 0];
#pragma unroll
    for (int i = 0; i < NN_ROWS / 16; ++i) f[i] = T[min(t * NN_ROWS + i * 16 + sr, cnt - 1) * ld + c];
  };
  auto put = [&](long t, int ct) {
    const bool lc = ct * NN_CT + sj < n_cols;
#pragma unroll
    for (int i = 0; i < NN_ROWS / 16; ++i) tile[sj * NN_RS + i * 16 + sr] = (lc && t * NN_ROWS + i * 16 + sr < cnt) ? f[i] : 0.0;
  };

  fetch(t0, 0);
  put(t0, 0);
  __syncthreads();
  for (long t = t0; t < t1; ++t) {
    const long row = t * NN_ROWS + tid;
    for (int ct = 0; ct < nct; ++ct) {
      const bool last_ct = ct + 1 == nct;
      const bool more = !last_ct || t + 1 < t1;
      const long tn = last_ct ? t + 1 : t;
      const int cn = last_ct ? 0 : ct + 1;
      if (more) fetch(tn, cn);
      const int jn = min(NN_CT, n_cols - ct * NN_CT);
      const double* yc = y + (long)ct * NN_CT * YS;             // wave-uniform
#pragma unroll 2
      for (int jj = 0; jj < jn; ++jj) {
        const double tv = tile[jj * NN_RS + tid];
#pragma unroll
        for (int i = 0; i < NN_NY; ++i) {
          double d;
          if constexpr (MASKED) d = fma(yc[jj * YS + NN_NY + i], tv, yc[jj * YS + i]);
          else d = yc[jj * YS + i] - tv;
          acc[i] = fma(d, d, acc[i]);
        }
      }
      if (last_ct) {
#pragma unroll
        for (int i = 0; i < NN_NY; ++i) {
          if (row < cnt && acc[i] < best[i]) { best[i] = acc[i]; bi[i] = (int)row; }
          acc[i] = 0.0;
        }
      }
      __syncthreads();                                  // the tile has been consumed
      if (more) put(tn, cn);
      __syncthreads();
    }
  }

#pragma unroll
  for (int i = 0; i < NN_NY; ++i) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) nn_take(best[i], bi[i], __shfl_xor(best[i], sh), __shfl_xor(bi[i], sh));
    if (lane == 0) { red_d[wave][i] = best[i]; red_i[wave][i] = bi[i]; }
  }
  __syncthreads();
  if (tid < NN_NY) {
    double d = red_d[0][tid];
    int b = red_i[0][tid];
    for (int w = 1; w < 4; ++w) nn_take(d, b, red_d[w][tid], red_i[w][tid]);
    const long o = (long)blockIdx.y * ry + (long)blockIdx.x * NN_NY + tid;
    pd[o] = d;
    pi[o] = b;
  }
}

// bd, bi [ry]: the call's running best, set when first, else a slice's row (plus base, the chunk's first row) replaces it only when strictly nearer
__global__ void __launch_bounds__(256) nn_reduce_kernel(const double* __restrict__ pd, const int* __restrict__ pi, int slices, long ry, long long base,
                                                        int first, double* __restrict__ bd, long long* __restrict__ bi) {
  const long r = blockIdx.x * 256L + threadIdx.x;
  if (r >= ry) return;
  double d = first ? std::numeric_limits<double>::infinity() : bd[r];
  long long b = first ? -1 : bi[r];
  for (int s = 0; s < slices; ++s) {
    const double od = pd[s * ry + r];
    if (od < d) { d = od; b = base + pi[s * ry + r]; }
  }
  bd[r] = d;
  bi[r] = b;
}

// out [cnt][Q] = Xmu[bi[r]] (zeros for a new row without a training row)
__global__ void __launch_bounds__(256) nn_gather_kernel(const double* __restrict__ Xmu, int Q, const long long* __restrict__ bi, long cnt,
                                                        double* __restrict__ out) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < cnt * Q; e += (long)gridDim.x * 256L) {
    const long long b = bi[e / Q];
    out[e] = b >= 0 ? Xmu[b * Q + e % Q] : 0.0;
  }
}

// test hook (gp_debug_set_option "nearest_rows"): rows per chunk, of the new rows (rounded up to NN_NY) and of host training rows (rounded up to
// NN_ROWS); 0 = the defaults below
std::atomic<int> g_opt_nn_rows{0};

struct NnPlan {
  DevBuf<double> in;          // [rows][D] a chunk of host training rows (not used with the resident Y)
  DevBuf<double> y;           // [rows / NN_NY][ncp][NN_NY] a chunk of new rows: their observed columns ([ncp][2][NN_NY] with a mask: wy, nw)
  DevBuf<int> cols;           // [ncp] the observed columns, zero beyond n_cols
  DevBuf<double> pd;          // [slices][rows] per-slice least distances
  DevBuf<int> pi;             // [slices][rows] and their rows
  DevBuf<double> bd;          // [rows] the running best of the chunk of new rows
  DevBuf<long long> bi;       // [rows]
  DevBuf<double> x;           // [rows][Q] the winners' base means
};
void NnPlanDelete::operator()(NnPlan* p) const { delete p; }

// observed (n,D), nonzero = observed, or NULL: the one column list cols (NULL: all D columns) for every new row.  With a mask the columns of the
// call are those that some row of the call observes, ascending: a column nobody observes costs nothing, and one that only other rows observe adds
// an exact zero to a row's sum, so a row's result does not depend on the rows it is called with
int run_nearest(gp_ctx* c, long n_train, const double* Y_train, long n, const double* Y_test, const int* cols, int n_cols, const uint8_t* observed,
                double* dist2, int64_t* index, double* x_near) {
  const int D = c->D, Q = c->Q;
  std::vector<int> ocols;
  if (observed) {
    std::vector<uint8_t> any((size_t)D, 0);
    for (long r = 0; r < n; ++r)
      for (int j = 0; j < D; ++j) any[j] |= observed[r * D + j];
    for (int j = 0; j < D; ++j)
      if (any[j]) ocols.push_back(j);
    cols = ocols.data();
    n_cols = (int)ocols.size();
  }
  const int nc = cols ? n_cols : D, ncp = (int)round_up(nc, NN_CT), ys = observed ? 2 : 1;       // ys: values per (column, new row)
  const int opt = g_opt_nn_rows.load();
  // a chunk of new rows [rows][ncp] and a chunk of host training rows [rows][D] stay near 64 MB each
  const long RY = std::min(round_up(n, NN_NY), opt > 0 ? round_up(opt, NN_NY) : std::max<long>(NN_NY, std::min<long>(1L << 16, (64L << 20) / (8L * ncp * ys)) / NN_NY * NN_NY));
  const long RT = !Y_train ? n_train
                           : std::min(round_up(n_train, NN_ROWS),
                                      opt > 0 ? round_up(opt, NN_ROWS) : std::max<long>(NN_ROWS, std::min<long>(1L << 20, (64L << 20) / (8L * D)) / NN_ROWS * NN_ROWS));
  if (RT > std::numeric_limits<int>::max()) return fail(c, GP_ERR_UNSUPPORTED, "gp_nearest_rows: %ld training rows in one launch (the row index is 32-bit)", RT);
  // slices x rows of a launch: at most ceil(NN_BLOCKS / blocks) slices of blocks x NN_NY rows
  const size_t part = (size_t)NN_BLOCKS * NN_NY + (size_t)RY;
  if (!c->nn) c->nn.reset(new NnPlan());
  NnPlan& p = *c->nn;
  if (Y_train) GP_TRY_RC(p.in.grow(c, (size_t)(RT * D), DA_RAW));
  GP_TRY_RC(p.y.grow(c, (size_t)(RY * ncp * ys), DA_RAW));
  GP_TRY_RC(p.cols.grow(c, (size_t)ncp, DA_RAW));
  GP_TRY_RC(p.pd.grow(c, part, DA_RAW));
  GP_TRY_RC(p.pi.grow(c, part, DA_RAW));
  GP_TRY_RC(p.bd.grow(c, (size_t)RY, DA_RAW));
  GP_TRY_RC(p.bi.grow(c, (size_t)RY, DA_RAW));
  if (x_near) GP_TRY_RC(p.x.grow(c, (size_t)(RY * Q), DA_RAW));
  hipStream_t st = c->stream;
  std::vector<int> hcols((size_t)ncp, 0);
  for (int j = 0; j < nc; ++j) hcols[j] = cols ? cols[j] : j;
  GP_HIP(c, hipMemcpyAsync(p.cols, hcols.data(), hcols.size() * 4, hipMemcpyHostToDevice, st));
  std::vector<double> hy((size_t)(RY * ncp * ys));
  static_assert(sizeof(long long) == sizeof(int64_t), "the rows are copied out as they are");
  for (long n0 = 0; n0 < n; n0 += RY) {
    const long cnt = std::min(RY, n - n0), ry = round_up(cnt, NN_NY), yb = ry / NN_NY;
    // the chunk's observed columns, [block][column][row of the block]: columns outside cols are never read, on the host or on the device; with a
    // mask [block][column][wy | nw][row of the block], and an entry that its row does not observe is not read either
    std::fill(hy.begin(), hy.begin() + (size_t)(ry * ncp * ys), 0.0);
    for (long r = 0; r < cnt; ++r) {
      const double* src = Y_test + (n0 + r) * D;
      double* dst = hy.data() + (size_t)(r / NN_NY) * ncp * NN_NY * ys + r % NN_NY;
      if (observed) {
        const uint8_t* o = observed + (n0 + r) * D;
        for (int j = 0; j < nc; ++j) {
          const bool on = o[hcols[j]] != 0;
          dst[(size_t)j * 2 * NN_NY] = on ? src[hcols[j]] : 0.0;
          dst[(size_t)j * 2 * NN_NY + NN_NY] = on ? -1.0 : -0.0;
        }
      } else {
        for (int j = 0; j < nc; ++j) dst[(size_t)j * NN_NY] = src[hcols[j]];
      }
    }
    GP_HIP(c, hipMemcpyAsync(p.y, hy.data(), (size_t)(ry * ncp * ys) * 8, hipMemcpyHostToDevice, st));
    for (long m0 = 0; m0 < n_train; m0 += RT) {
      const long rows = std::min(RT, n_train - m0);
      const double* t = c->Kaug + c->Mp;
      long ld = c->LDK;
      if (Y_train) {
        GP_HIP(c, hipMemcpyAsync(p.in, Y_train + m0 * D, (size_t)(rows * D) * 8, hipMemcpyHostToDevice, st));
        t = p.in;
        ld = D;
      }
      const long tiles = (rows + NN_ROWS - 1) / NN_ROWS;
      const auto [tps, slices] = slice_plan(tiles, yb, NN_BLOCKS);
      if (observed)
        GP_LAUNCH(c, st, nn_search_kernel<true>, dim3((unsigned)yb, (unsigned)slices), dim3(256), 0, t, ld, rows, tps, p.y, p.cols, nc, ncp, ry, p.pd, p.pi);
      else
        GP_LAUNCH(c, st, nn_search_kernel<false>, dim3((unsigned)yb, (unsigned)slices), dim3(256), 0, t, ld, rows, tps, p.y, p.cols, nc, ncp, ry, p.pd, p.pi);
      GP_LAUNCH(c, st, nn_reduce_kernel, dim3((unsigned)((ry + 255) / 256)), dim3(256), 0, p.pd, p.pi, slices, ry, (long long)m0, m0 == 0 ? 1 : 0,
                p.bd, p.bi);
    }
    if (dist2) GP_HIP(c, hipMemcpyAsync(dist2 + n0, p.bd, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (index) GP_HIP(c, hipMemcpyAsync(index + n0, p.bi, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    if (x_near) {
      GP_LAUNCH(c, st, nn_gather_kernel, dim3(blocks_for(cnt * Q)), dim3(256), 0, c->Xmu, Q, p.bi, cnt, p.x);
      GP_HIP(c, hipMemcpyAsync(x_near + n0 * Q, p.x, (size_t)(cnt * Q) * 8, hipMemcpyDeviceToHost, st));
    }
    GP_HIP(c, hipStreamSynchronize(st));              // the staging vector is refilled for the next chunk
    ++c->sync_epoch;
  }
  return GP_OK;
}

}  // namespace gp
