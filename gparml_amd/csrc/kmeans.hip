// One Lloyd assignment pass of k-means on the device (gp_kmeans_accumulate): the initialisation of the inducing points.
//
// parallel_GPLVM.init_statistics places Z with scipy.cluster.vq.kmeans(embeddings, M) on the host (parallel_GPLVM.py:179-186): per pass, vq assigns
// every row to its nearest centre and update_cluster_means averages the rows of every centre.  One pass is N K Q distance terms and has the
// map-reduce shape of everything else here -- a shard yields per-centre sums, counts and the summed distances, the host (or an all-reduce) adds them
// over shards and divides (gparml_amd/init.py) -- so all shards can be clustered, not only the first ones that reach M rows.
//   km_assign_kernel: one row per thread, its Q coordinates in registers; the centres pass through LDS in tiles of KM_TILE / QT rows (K Q of any
//     size: M = 1024, Q = 50 is 400 KB), every lane reads the same centre element (a broadcast, no bank conflicts).  The distance is the direct form
//     sum_q (x_q - z_q)^2, q ascending, one fma per term (never |x|^2 - 2 x.z + |z|^2: at near-ties its cancellation decides the label); a centre
//     replaces the best one only when strictly nearer, so ties go to the lowest index.  Out: the row's label, and per workgroup of 256 rows the
//     partial [sum d^2, sum d] (LDS tree, fixed order).  QT: compile-time row width (psi1_qp: Q rounded up to 2 up to 16, then 24, 32, 52, 64; the
//     padding coordinates are 0 in the row and in the centre: exact zeros added).  QT = 0 (Q > 64): rows and centres are read from memory.
//   km_reduce_kernel: per-centre sums and counts WITHOUT floating-point atomics.  Workgroup (segment of KM_SEG rows, group of KM_CG centres): the
//     segment's labels are staged in LDS once; a wave takes a centre k, lane l walks the rows l, l + 64, .. of the segment in ascending order and
//     adds the rows labelled k into 16 registers (16 coordinates per sweep over the labels), the 64 lane sums are added pairwise (distance 32 .. 1)
//     and written as the partial [segment][k][q].  The label scan is K n / 64 LDS reads, 1 / (2 Q) of the distance work.
//   km_final_kernel: sums[k][q] (+)= partials over the segments in ascending order, the same for the counts and for the distance partials of the
//     workgroups (thread t adds the partials t, t + 256, .., then an LDS tree).  A call's chunks accumulate in ascending order.
// Every buffer belongs to the context's KmPlan (allocated on first use, grown on demand, freed with the context).  All of them are written before
// they are read (DA_RAW: NaN-filled in the poison test mode).  Nothing of the evaluation is touched: only the resident X_mu is read (X == NULL).
#include "gp_common.h"
#include "lane_reduce.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace gp {

constexpr int KM_TILE = 4096;     // doubles of centres per LDS tile (32 KB: five workgroups per CU)
constexpr int KM_SEG = 4096;      // rows per segment of the reduction (16 KB of labels in LDS)
constexpr int KM_CG = 16;         // centres per workgroup of the reduction (four per wave)
constexpr int KM_QS = 16;         // coordinates per sweep of the reduction

// cen [K][QT] (rows zero-padded; [K][Q] for QT = 0); X [cnt][Q]; labels [cnt]; dpart [gridDim.x][2]
template <int QT>
__global__ void __launch_bounds__(256) km_assign_kernel(const double* __restrict__ X, const double* __restrict__ cen, long cnt, int Q, int K,
                                                        int* __restrict__ labels, double* __restrict__ dpart) {
  constexpr int QS = QT > 0 ? QT : 1;
  __shared__ double tile[QT > 0 ? KM_TILE : 1];
  __shared__ double red[2 * 256];
  const int tid = threadIdx.x;
  const long i = blockIdx.x * 256L + tid;
  const bool live = i < cnt;
  const double* xr = X + (live ? i : 0) * Q;
  double best = std::numeric_limits<double>::infinity();
  int bl = 0;
  if constexpr (QT > 0) {
    double x[QS];
#pragma unroll
    for (int q = 0; q < QT; ++q) x[q] = (q < Q) ? xr[q] : 0.0;
    constexpr int KT = KM_TILE / QS;
    for (int k0 = 0; k0 < K; k0 += KT) {
      const int kt = min(KT, K - k0);
      __syncthreads();                                  // the previous tile has been consumed
      for (int e = tid; e < kt * QT; e += 256) tile[e] = cen[(long)k0 * QT + e];
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < kt; ++kk) {
        const double* z = tile + kk * QT;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < QT; ++q) { const double d = x[q] - z[q]; s = fma(d, d, s); }
        if (s < best) { best = s; bl = k0 + kk; }
      }
    }
  } else {
    for (int k = 0; k < K; ++k) {
      const double* z = cen + (long)k * Q;
      double s = 0.0;
      for (int q = 0; q < Q; ++q) { const double d = xr[q] - z[q]; s = fma(d, d, s); }
      if (s < best) { best = s; bl = k; }
    }
  }
  if (live) labels[i] = bl;
  red[tid] = live ? best : 0.0;
  red[256 + tid] = live ? sqrt(best) : 0.0;
  __syncthreads();
  block_fold<256>([&](int i, int j) { red[i] += red[j]; red[256 + i] += red[256 + j]; });
  if (tid == 0) { dpart[2 * blockIdx.x] = red[0]; dpart[2 * blockIdx.x + 1] = red[256]; }
}

// part [segs][K][Q], pcnt [segs][K]; grid (segs, ceil(K / KM_CG))
__global__ void __launch_bounds__(256) km_reduce_kernel(const double* __restrict__ X, const int* __restrict__ labels, long cnt, int Q, int K,
                                                        double* __restrict__ part, int* __restrict__ pcnt) {
  __shared__ int lab[KM_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long base = (long)blockIdx.x * KM_SEG;
  const int rows = (int)min((long)KM_SEG, cnt - base);          // >= 1
  const int iters = (rows + 63) / 64;
  for (int e = tid; e < iters * 64; e += 256) lab[e] = e < rows ? labels[base + e] : -1;
  __syncthreads();
  const int kend = min(K, ((int)blockIdx.y + 1) * KM_CG);
  for (int k = blockIdx.y * KM_CG + wave; k < kend; k += 4) {
    double* out = part + ((long)blockIdx.x * K + k) * Q;
    for (int q0 = 0; q0 < Q; q0 += KM_QS) {
      double acc[KM_QS];
#pragma unroll
      for (int j = 0; j < KM_QS; ++j) acc[j] = 0.0;
      int mine = 0;
      for (int it = 0; it < iters; ++it) {
        const int r = it * 64 + lane;
        if (lab[r] == k) {
          ++mine;
          const double* xr = X + (base + r) * Q + q0;
#pragma unroll
          for (int j = 0; j < KM_QS; ++j) if (q0 + j < Q) acc[j] += xr[j];
        }
      }
#pragma unroll
      for (int j = 0; j < KM_QS; ++j) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) acc[j] += __shfl_xor(acc[j], sh);      // wave_sum (lane_reduce.h) spelled out: KM_QS calls change the register allocation
      }
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KM_QS; ++j) if (q0 + j < Q) out[q0 + j] = acc[j];
      }
      if (q0 == 0) {
        mine = wave_sum(mine);
        if (lane == 0) pcnt[(long)blockIdx.x * K + k] = mine;
      }
    }
  }
}

// sums [K][Q], counts [K], dist [2]: set (first chunk) or added to; the last workgroup folds the distance partials
__global__ void __launch_bounds__(256) km_final_kernel(const double* __restrict__ part, const int* __restrict__ pcnt, const double* __restrict__ dpart,
                                                       int segs, int dblocks, long kq, int K, int first, double* __restrict__ sums,
                                                       long long* __restrict__ counts, double* __restrict__ dist) {
  __shared__ double red[2 * 256];
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const long e = blockIdx.x * 256L + tid;
    if (e < kq) {
      double s = 0.0;
      for (int g = 0; g < segs; ++g) s += part[g * kq + e];
      sums[e] = first ? s : sums[e] + s;
    }
    if (e < K) {
      long long n = 0;
      for (int g = 0; g < segs; ++g) n += pcnt[(long)g * K + e];
      counts[e] = first ? n : counts[e] + n;
    }
    return;
  }
  double a = 0.0, b = 0.0;
  for (int g = tid; g < dblocks; g += 256) { a += dpart[2 * g]; b += dpart[2 * g + 1]; }
  red[tid] = a;
  red[256 + tid] = b;
  __syncthreads();
  block_fold<256>([&](int i, int j) { red[i] += red[j]; red[256 + i] += red[256 + j]; });
  if (tid == 0) { dist[0] = first ? red[0] : dist[0] + red[0]; dist[1] = first ? red[256] : dist[1] + red[256]; }
}

// test hook (gp_debug_set_option "kmeans_rows"): rows per chunk, rounded up to KM_SEG; 0 = the default below (pca.hip reads the same switch)
std::atomic<int> g_opt_km_rows{0};

static long km_rows_for(const gp_ctx* c) {
  const int opt = g_opt_km_rows.load();
  if (opt > 0) return round_up(opt, KM_SEG);
  // a chunk of host rows [rows][Q] stays near 64 MB, at most 2^20 rows
  return std::max<long>(KM_SEG, std::min<long>(1L << 20, (64L << 20) / (8L * c->Q) / KM_SEG * KM_SEG));
}

// the buffers of a pass; the row buffers hold min(n, chunk) rows, the centre-sized ones K centres: each grows on demand
struct KmPlan {
  DevBuf<double> in;          // [rows][Q] a chunk of host rows (not used with the resident X_mu)
  DevBuf<int> lab;            // [rows]
  DevBuf<double> dpart;       // [rows / 256][2] per-workgroup [sum d^2, sum d]
  DevBuf<double> cen;         // [K][QT] the centres, rows zero-padded to the kernel's width
  DevBuf<double> part;        // [segs][K][Q] per-segment sums
  DevBuf<int> pcnt;           // [segs][K] per-segment counts
  DevBuf<double> out;         // [K][Q] sums | [2] distances
  DevBuf<long long> cnt;      // [K]
};
void KmPlanDelete::operator()(KmPlan* p) const { delete p; }

template <int QT>
static int km_launch_assign(gp_ctx* c, hipStream_t st, unsigned blocks, const double* X, const double* cen, long cnt, int Q, int K, int* lab, double* dpart) {
  GP_LAUNCH(c, st, km_assign_kernel<QT>, dim3(blocks), dim3(256), 0, X, cen, cnt, Q, K, lab, dpart);
  return GP_OK;
}

int run_kmeans(gp_ctx* c, long n, const double* X, int K, const double* centres, double* sums, int64_t* counts, double* dist2, int32_t* labels) {
  const long Q = c->Q, R = std::min(km_rows_for(c), round_up(n, KM_SEG)), kq = (long)K * Q;
  const int QT = psi1_qp((int)Q), QS = QT > 0 ? QT : (int)Q;
  const long segs_max = R / KM_SEG, blocks_max = R / 256;
  if (!c->km) c->km.reset(new KmPlan());
  KmPlan& p = *c->km;
  if (X) GP_TRY_RC(p.in.grow(c, (size_t)(R * Q), DA_RAW));
  GP_TRY_RC(p.lab.grow(c, (size_t)R, DA_RAW));
  GP_TRY_RC(p.dpart.grow(c, (size_t)(2 * blocks_max), DA_RAW));
  GP_TRY_RC(p.cen.grow(c, (size_t)K * QS, DA_RAW));
  GP_TRY_RC(p.part.grow(c, (size_t)(segs_max * kq), DA_RAW));
  GP_TRY_RC(p.pcnt.grow(c, (size_t)(segs_max * K), DA_RAW));
  GP_TRY_RC(p.out.grow(c, (size_t)(kq + 2), DA_RAW));
  GP_TRY_RC(p.cnt.grow(c, (size_t)K, DA_RAW));
  hipStream_t st = c->stream;
  std::vector<double> hc((size_t)K * QS, 0.0);
  for (int k = 0; k < K; ++k) std::copy(centres + k * Q, centres + (k + 1) * Q, hc.begin() + (size_t)k * QS);
  GP_HIP(c, hipMemcpyAsync(p.cen, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, st));
  for (long n0 = 0; n0 < n; n0 += R) {
    const long cnt = std::min(R, n - n0);
    const double* x = c->Xmu + n0 * Q;
    if (X) {
      GP_HIP(c, hipMemcpyAsync(p.in, X + n0 * Q, (size_t)(cnt * Q) * 8, hipMemcpyHostToDevice, st));
      x = p.in;
    }
    const unsigned blocks = (unsigned)((cnt + 255) / 256), segs = (unsigned)((cnt + KM_SEG - 1) / KM_SEG);
    // (width 0: the kernel with a run-time Q, beyond the 64-wide records)
    GP_TRY_RC((for_width<2, 4, 6, 8, 10, 12, 14, 16, 24, 32, 52, 64, 0>(c, "k-means assignment kernel", QT, [&](auto W) {
      return km_launch_assign<W()>(c, st, blocks, x, p.cen, cnt, (int)Q, K, p.lab, p.dpart);
    })));
    if (labels) GP_HIP(c, hipMemcpyAsync(labels + n0, p.lab, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    if (sums || counts) {
      GP_LAUNCH(c, st, km_reduce_kernel, dim3(segs, (unsigned)((K + KM_CG - 1) / KM_CG)), dim3(256), 0, x, p.lab, cnt, (int)Q, K, p.part, p.pcnt);
    }
    // without sums and counts only the last workgroup (the distances) has work
    const unsigned fblocks = (sums || counts) ? (unsigned)((std::max<long>(kq, K) + 255) / 256) : 0u;
    GP_LAUNCH(c, st, km_final_kernel, dim3(fblocks + 1), dim3(256), 0, p.part, p.pcnt, p.dpart, (int)segs, (int)blocks, kq, K, n0 == 0 ? 1 : 0, p.out,
              p.cnt, p.out + kq);
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "counts are copied out as they are");
  if (sums) GP_HIP(c, hipMemcpyAsync(sums, p.out, (size_t)kq * 8, hipMemcpyDeviceToHost, st));
  if (counts) GP_HIP(c, hipMemcpyAsync(counts, p.cnt, (size_t)K * 8, hipMemcpyDeviceToHost, st));
  if (dist2) GP_HIP(c, hipMemcpyAsync(dist2, p.out + kq, 16, hipMemcpyDeviceToHost, st));
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
