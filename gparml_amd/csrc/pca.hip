// The PCA that initialises the embeddings, on the device (gp_scatter_accumulate, gp_project_rows).
//
// supporting_functions.PCA (supporting_functions.py:102-121) over ALL data (local_MapReduce.py:50-65) is, in its streaming form
// (gparml_amd/init.py: pca_axes), a sum over shards of the D x D Gram matrix and the column sums of the rows shifted by a centre, an eigh of the
// D x D scatter matrix on the host, and a projection of every row on the leading axes.  Y is resident already: columns [Mp, Mp + D) of Kaug, stored
// [row][column], which is the [k][free] operand layout of phase 1 -- the Gram matrix is Kaug^T Kaug restricted to those columns.
//   pca_scatter_kernel: workgroup = (tile pair ti <= tj of the upper triangle of 128 x 128 tiles) x (slice of rows).  Four waves as 2 x 2 of 64 x 64
//     on the 4x4x4 FP64 matrix-core instruction (mma_f64.h: mma_chunk, both operands FREE_CONTIG), 16 rows per chunk through two LDS buffers.  The
//     operand tiles are staged through registers, not by LDS-DMA: the centre is subtracted from every element BEFORE the product (never
//     Y^T Y - n c c^T), and the rows beyond the slice's end and the columns beyond D are replaced by exact zeros on the way (the padded rows of
//     Kaug minus the centre would add c c^T each).  A diagonal tile stages one operand and reads it twice.  Out: one partial tile per
//     (slice, tile pair).
//   pca_gram_reduce_kernel: adds the slices in ascending order onto the running Gram matrix (set by a call's first chunk) and writes every
//     element of the upper triangle (of a diagonal tile: its elements r <= c) a second time transposed: gram[i][j] and gram[j][i] are one value.
//   pca_colsum_kernel / pca_sum_reduce_kernel: the column sums in the same slices.  Wave p of four adds the slice's rows p, p + 4, .. in
//     ascending order (64 lanes = 64 columns), the four are added as (0 + 1) + (2 + 3); the slices, then the chunks, in ascending order.  The
//     sums are always computed here, also next to a Gram matrix: a sum-only call returns the same bits, at the price of a second read of Y
//     in a Gram call.
//   pca_project_kernel<QT>: one row per thread, QT outputs in registers; 256 rows x 16 columns of Y - mean pass through LDS (coalesced reads of
//     Y, transposed so that a thread reads its row without bank conflicts), the rows of P are wave-uniform reads.  x_q = sum_d (y_d - mean_d) P[d][q],
//     d ascending, one fma per term: a row's result never depends on the other rows of the call.
// Slices: pca_slice_rows(n, Dp) rows each, a function of the call's n and D alone (never of the device); slice s holds the rows
// [s * rows, (s + 1) * rows) of the call, host chunks are multiples of it and resident rows go in one launch: the summation order is a function of the row index, and host rows
// and resident rows give the same bits.  Every buffer belongs to the context's PcaPlan (grown on demand, freed with the context) and is
// written before it is read (DA_RAW).  Nothing of the evaluation is touched: only Kaug's Y columns are read (Y == NULL).
#include "gp_common.h"
#include <algorithm>
#include <cmath>

namespace gp {

constexpr int PCA_SLICE_MIN = 512;   // rows of the shortest slice
constexpr int PCA_SLICE_Q = 64;      // slice lengths are multiples of this (of KC, and of the four row phases of the column sums)
constexpr int PCA_SLICES_MAX = 512;  // two workgroups per CU at one tile pair
constexpr int PJ_DT = 16;            // columns of Y per LDS tile of the projection
constexpr int PJ_RS = 260;           // its row stride (256 rows + 4: the transposing stores are 2-way conflicts instead of 16-way)

// Y [rows][ld] (column 0 = the first data column); cen [Dp] (zero beyond D); part [gridDim.y][gridDim.x][TILE * TILE]
__global__ void __launch_bounds__(256) pca_scatter_kernel(const double* __restrict__ Y, long ld, long cnt, long slice_rows, int D, int nt,
                                                          const double* __restrict__ cen, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][TILE_LDS_DOUBLES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wrow0 = (wave >> 1) * WT, wcol0 = (wave & 1) * WT;
  int ti = 0, rem = blockIdx.x;
  while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const long r0 = (long)blockIdx.y * slice_rows, r1 = min(cnt, r0 + slice_rows);
  const int nc = (int)((r1 - r0 + KC - 1) / KC);                // >= 1: the grid has no empty slice
  const int ca = ti * TILE + 2 * lane, cb = tj * TILE + 2 * lane;
  const double ca0 = cen[ca], ca1 = cen[ca + 1], cb0 = cen[cb], cb1 = cen[cb + 1];
  const bool ma0 = ca < D, ma1 = ca + 1 < D, mb0 = cb < D, mb1 = cb + 1 < D;

  double2 ra[4], rb[4];
  // chunk c of the slice into registers: wave w takes the rows 4 w .. 4 w + 3, a lane two columns.  A row at or beyond r1 is not read at all.
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long r = r0 + (long)c * KC + wave * 4 + i;
      ra[i] = make_double2(0.0, 0.0);
      rb[i] = make_double2(0.0, 0.0);
      if (r < r1) {
        ra[i] = *reinterpret_cast<const double2*>(Y + r * ld + ca);
        if (!diag) rb[i] = *reinterpret_cast<const double2*>(Y + r * ld + cb);
      }
    }
  };
  auto put = [&](int buf, int c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i;
      const bool live = r0 + (long)c * KC + row < r1;
      *reinterpret_cast<double2*>(&lds[buf][0][row * LDS_RC + 2 * lane]) =
          make_double2(live && ma0 ? ra[i].x - ca0 : 0.0, live && ma1 ? ra[i].y - ca1 : 0.0);
      if (!diag)
        *reinterpret_cast<double2*>(&lds[buf][1][row * LDS_RC + 2 * lane]) =
            make_double2(live && mb0 ? rb[i].x - cb0 : 0.0, live && mb1 ? rb[i].y - cb1 : 0.0);
    }
  };

  Acc acc;
  acc.zero();
  const LaneOfs ofs = lane_offsets<FREE_CONTIG, FREE_CONTIG>(wrow0, wcol0, lane);
  fetch(0);
  put(0, 0);
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const int cur = c & 1;
    if (c + 1 < nc) fetch(c + 1);
    mma_chunk<FREE_CONTIG, FREE_CONTIG>(lds[cur][0], lds[cur][diag ? 0 : 1], acc, ofs);
    if (c + 1 < nc) put(cur ^ 1, c + 1);      // lds[cur ^ 1] was last read before the barrier that ended the previous iteration
    __syncthreads();
  }
  acc.drain();
  double* w = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (TILE * TILE);
#pragma unroll
  for (int ar = 0; ar < 4; ++ar)
#pragma unroll
    for (int bc = 0; bc < 16; ++bc) w[(wrow0 + acc_row(ar, lane)) * TILE + wcol0 + acc_col(bc, lane)] = acc.v[ar][bc];
}

// gram [D][D] (set when first, else added to); grid (tile pairs, TILE * TILE / 256)
__global__ void __launch_bounds__(256) pca_gram_reduce_kernel(const double* __restrict__ part, int slices, int D, int nt, int first,
                                                              double* __restrict__ gram) {
  int ti = 0, rem = blockIdx.x;
  while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
  const int tj = ti + rem;
  const int e = blockIdx.y * 256 + threadIdx.x, r = e >> 7, c = e & 127;
  const long gi = (long)ti * TILE + r, gj = (long)tj * TILE + c;
  if (gi >= D || gj >= D || gi > gj) return;
  double s = first ? 0.0 : gram[gi * D + gj];
  const long T = gridDim.x;
  for (int g = 0; g < slices; ++g) s += part[((long)g * T + blockIdx.x) * (TILE * TILE) + e];
  gram[gi * D + gj] = s;
  gram[gj * D + gi] = s;
}

// part [gridDim.x][Dp]; grid (slices, Dp / 64)
__global__ void __launch_bounds__(256) pca_colsum_kernel(const double* __restrict__ Y, long ld, long cnt, long slice_rows, int D, int Dp,
                                                         const double* __restrict__ cen, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = blockIdx.y * 64 + lane;
  const long r0 = (long)blockIdx.x * slice_rows, r1 = min(cnt, r0 + slice_rows);
  double s = 0.0;
  if (col < D) {
    const double c = cen[col];
#pragma unroll 8
    for (long r = r0 + ph; r < r1; r += 4) s += Y[r * ld + col] - c;
  }
  red[ph][lane] = s;
  __syncthreads();
  if (ph == 0) part[(long)blockIdx.x * Dp + col] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ void __launch_bounds__(256) pca_sum_reduce_kernel(const double* __restrict__ part, int slices, int Dp, int first, double* __restrict__ sum) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= Dp) return;
  double s = first ? 0.0 : sum[col];
  for (int g = 0; g < slices; ++g) s += part[(long)g * Dp + col];
  sum[col] = s;
}

// Y [cnt][ld]; mean [Dr], P [Dr][QP] (Dr = D rounded up to PJ_DT, QP = the q tiles: zero-padded); X [cnt][Q]; grid (ceil(cnt / 256), QP / QT)
template <int QT>
__global__ void __launch_bounds__(256) pca_project_kernel(const double* __restrict__ Y, long ld, long cnt, int D, const double* __restrict__ mean,
                                                          const double* __restrict__ P, int QP, int Q, double* __restrict__ X) {
  __shared__ double tile[PJ_DT * PJ_RS];
  const int tid = threadIdx.x;
  const long row0 = blockIdx.x * 256L;
  const int q0 = blockIdx.y * QT;
  double acc[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) acc[q] = 0.0;
  for (int d0 = 0; d0 < D; d0 += PJ_DT) {
    __syncthreads();                                  // the previous tile has been consumed
    // 256 rows x 8 column pairs: eight lanes read one row's 128 bytes.  Columns D .. Dr - 1 lie inside the row's padding; they and the rows
    // beyond cnt (never read) become exact zeros
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = i * 32 + (tid >> 3), d = d0 + 2 * (tid & 7);
      double2 v = make_double2(0.0, 0.0);
      if (row0 + rr < cnt) {
        v = *reinterpret_cast<const double2*>(Y + (row0 + rr) * ld + d);
        v.x = d < D ? v.x - mean[d] : 0.0;
        v.y = d + 1 < D ? v.y - mean[d + 1] : 0.0;
      }
      tile[(d - d0) * PJ_RS + rr] = v.x;
      tile[(d - d0 + 1) * PJ_RS + rr] = v.y;
    }
    __syncthreads();
#pragma unroll 4
    for (int dd = 0; dd < PJ_DT; ++dd) {
      const double y = tile[dd * PJ_RS + tid];
      const double* p = P + (long)(d0 + dd) * QP + q0;           // wave-uniform
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = fma(y, p[q], acc[q]);
    }
  }
  if (row0 + tid < cnt) {
    double* x = X + (row0 + tid) * Q + q0;
#pragma unroll
    for (int q = 0; q < QT; ++q) if (q0 + q < Q) x[q] = acc[q];
  }
}

static long pca_tile_pairs(int Dp) { const long nt = Dp / TILE; return nt * (nt + 1) / 2; }

// rows of a slice: the partial tiles of a launch stay within 64 MB (one tile pair is 128 KB: 512 slices at D <= 128, 14 at D = 1000)
static long pca_slice_rows(long n, int Dp) {
  const long smax = std::max<long>(1, std::min<long>(PCA_SLICES_MAX, (64L << 20) / (pca_tile_pairs(Dp) * TILE * TILE * 8)));
  return std::max<long>(PCA_SLICE_MIN, round_up((n + smax - 1) / smax, PCA_SLICE_Q));
}

// rows of a launch.  Resident rows (host == false): all slices at once -- the slice count is what fills the device, and the partial tiles are
// bounded by it already.  Host rows: whole slices (the summation order is a function of the row index), as many as fit in 64 MB of [rows][Dp],
// at least one: n / S rows, which is 585 MB at N = 1e6, D = 1000 (14 slices of 71488 rows).  Test hook: gp_debug_set_option "kmeans_rows", the
// host chunk length of both initialisation passes (kmeans.hip), here rounded up to whole slices; 0 = the default
static long pca_chunk_rows(const gp_ctx* c, long n, long slice, bool host) {
  if (!host) return round_up(n, slice);
  const int opt = g_opt_km_rows.load();
  const long rows = opt > 0 ? round_up(opt, slice) : std::max(slice, std::min<long>(1L << 20, (64L << 20) / (8L * c->Dp)) / slice * slice);
  return std::min(rows, round_up(n, slice));
}

struct PcaPlan {
  DevBuf<double> in;          // [rows][Dp] a chunk of host rows (not used with the resident Y)
  DevBuf<double> cen;         // [Dp] the centre, zero beyond D | the projection's mean [Dr]
  DevBuf<double> part;        // [slices][tile pairs][TILE * TILE] partial tiles
  DevBuf<double> spart;       // [slices][Dp] partial column sums
  DevBuf<double> gram;        // [D][D]
  DevBuf<double> sum;         // [Dp]
  DevBuf<double> P;           // [Dr][QP]
  DevBuf<double> out;         // [rows][Q_out]
};
void PcaPlanDelete::operator()(PcaPlan* p) const { delete p; }

// the rows [n0, n0 + cnt) of the call on the device: the resident Y columns of Kaug, or the chunk copied into the plan's buffer
static int pca_rows(gp_ctx* c, PcaPlan& p, const double* Y, long n0, long cnt, const double** y, long* ld) {
  if (!Y) {
    *y = c->Kaug + n0 * c->LDK + c->Mp;
    *ld = c->LDK;
    return GP_OK;
  }
  GP_HIP(c, hipMemcpy2DAsync(p.in, (size_t)c->Dp * 8, Y + n0 * c->D, (size_t)c->D * 8, (size_t)c->D * 8, (size_t)cnt, hipMemcpyHostToDevice, c->stream));
  *y = p.in;
  *ld = c->Dp;
  return GP_OK;
}

int run_scatter(gp_ctx* c, long n, const double* Y, const double* centre, double* sum, double* gram) {
  const int D = c->D, Dp = c->Dp, nt = Dp / TILE;
  const long T = pca_tile_pairs(Dp), SL = pca_slice_rows(n, Dp), R = pca_chunk_rows(c, n, SL, Y != nullptr), smax = R / SL;
  if (!c->pca) c->pca.reset(new PcaPlan());
  PcaPlan& p = *c->pca;
  if (Y) GP_TRY_RC(p.in.grow(c, (size_t)(R * Dp), DA_RAW));
  GP_TRY_RC(p.cen.grow(c, (size_t)Dp + PJ_DT, DA_RAW));
  GP_TRY_RC(p.spart.grow(c, (size_t)(smax * Dp), DA_RAW));
  GP_TRY_RC(p.sum.grow(c, (size_t)Dp, DA_RAW));
  if (gram) {
    GP_TRY_RC(p.part.grow(c, (size_t)(smax * T) * TILE * TILE, DA_RAW));
    GP_TRY_RC(p.gram.grow(c, (size_t)D * D, DA_RAW));
  }
  hipStream_t st = c->stream;
  std::vector<double> hc((size_t)Dp, 0.0);
  std::copy(centre, centre + D, hc.begin());
  GP_HIP(c, hipMemcpyAsync(p.cen, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, st));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    const unsigned slices = (unsigned)((cnt + SL - 1) / SL);
    const int first = n0 == 0 ? 1 : 0;
    const double* y = nullptr;
    long ld = 0;
    GP_TRY_RC(pca_rows(c, p, Y, n0, cnt, &y, &ld));
    if (gram) {
      GP_LAUNCH(c, st, pca_scatter_kernel, dim3((unsigned)T, slices), dim3(256), 0, y, ld, cnt, SL, D, nt, p.cen, p.part);
      GP_LAUNCH(c, st, pca_gram_reduce_kernel, dim3((unsigned)T, TILE * TILE / 256), dim3(256), 0, p.part, (int)slices, D, nt, first, p.gram);
    }
    GP_LAUNCH(c, st, pca_colsum_kernel, dim3(slices, (unsigned)(Dp / 64)), dim3(256), 0, y, ld, cnt, SL, D, Dp, p.cen, p.spart);
    GP_LAUNCH(c, st, pca_sum_reduce_kernel, dim3((unsigned)((Dp + 255) / 256)), dim3(256), 0, p.spart, (int)slices, Dp, first, p.sum);
  }
  if (gram) GP_HIP(c, hipMemcpyAsync(gram, p.gram, (size_t)D * D * 8, hipMemcpyDeviceToHost, st));
  if (sum) GP_HIP(c, hipMemcpyAsync(sum, p.sum, (size_t)D * 8, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

template <int QT>
static int pca_launch_project(gp_ctx* c, hipStream_t st, dim3 grid, const double* y, long ld, long cnt, int D, const double* mean, const double* P,
                              int QP, int Q, double* X) {
  GP_LAUNCH(c, st, pca_project_kernel<QT>, grid, dim3(256), 0, y, ld, cnt, D, mean, P, QP, Q, X);
  return GP_OK;
}

int run_project(gp_ctx* c, long n, const double* Y, const double* mean, const double* P, int Q, double* X) {
  const int D = c->D, Dp = c->Dp, Dr = (int)round_up(D, PJ_DT);
  const int QT = Q <= 8 ? 8 : Q <= 16 ? 16 : Q <= 32 ? 32 : 64, QP = (int)round_up(Q, QT);
  // rows are independent, any chunk length gives the same bits: host rows as the scatter pass at the shortest slice, resident rows as many as
  // keep the output buffer [rows][Q] within 64 MB
  const long R = Y ? pca_chunk_rows(c, n, PCA_SLICE_MIN, true)
                   : std::min(round_up(n, 256), std::max<long>(256, std::min<long>(1L << 20, (64L << 20) / (8L * Q)) / 256 * 256));
  if (!c->pca) c->pca.reset(new PcaPlan());
  PcaPlan& p = *c->pca;
  if (Y) GP_TRY_RC(p.in.grow(c, (size_t)(R * Dp), DA_RAW));
  GP_TRY_RC(p.cen.grow(c, (size_t)Dp + PJ_DT, DA_RAW));
  GP_TRY_RC(p.P.grow(c, (size_t)Dr * QP, DA_RAW));
  GP_TRY_RC(p.out.grow(c, (size_t)(R * Q), DA_RAW));
  hipStream_t st = c->stream;
  std::vector<double> hm((size_t)Dr, 0.0), hp((size_t)Dr * QP, 0.0);
  std::copy(mean, mean + D, hm.begin());
  for (int d = 0; d < D; ++d) std::copy(P + (size_t)d * Q, P + (size_t)(d + 1) * Q, hp.begin() + (size_t)d * QP);
  GP_HIP(c, hipMemcpyAsync(p.cen, hm.data(), hm.size() * 8, hipMemcpyHostToDevice, st));
  GP_HIP(c, hipMemcpyAsync(p.P, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, st));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    const double* y = nullptr;
    long ld = 0;
    GP_TRY_RC(pca_rows(c, p, Y, n0, cnt, &y, &ld));
    const dim3 grid((unsigned)((cnt + 255) / 256), (unsigned)(QP / QT));
    GP_TRY_RC((for_width<8, 16, 32, 64>(c, "PCA projection kernel", QT, [&](auto W) {
      return pca_launch_project<W()>(c, st, grid, y, ld, cnt, D, p.cen, p.P, QP, Q, p.out);
    })));
    GP_HIP(c, hipMemcpyAsync(X + n0 * Q, p.out, (size_t)(cnt * Q) * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
