// The k nearest rows in latent space on the device (gp_knn_rows): per query row the k training rows of least weighted squared distance.
//
// The first question a GPLVM paper asks of a trained embedding -- the leave-one-out nearest-neighbour error of the latent means (Lawrence 2005;
// Titsias & Lawrence 2010) -- and what restarts of the latent inference, geodesic graphs and local subsets need: neighbour LISTS, with the query's
// own row left out and the dimensions weighted by the learnt ARD relevances.  kmeans.hip and nearest.hip return one neighbour; the all-pairs search
// of a shard is n n_train Q terms, hopeless on the host.  The search has the map-reduce shape of everything else here: a shard yields per query its
// k least pairs (distance, row), the caller merges the shards (gparml_amd/init.py: knn).
//   knn_search_kernel: workgroup = (block of 256 queries) x (slice of training rows).  One query per thread, its Q coordinates in registers (QT:
//     the compile-time width of km_assign_kernel, psi1_qp; padding coordinates are 0 on both sides: exact zeros added).  The training rows pass
//     through LDS in tiles of KNN_TILE / QT rows, every lane reads the same element (a broadcast, no bank conflicts); the next tile is fetched into
//     registers while this one is used and stored into the other of two buffers: one barrier per tile.  The distance is the direct form
//     sum_q w_q (x_q - t_q)^2, difference first, q ascending: acc = fma(e, e, acc) without weights, p = w_q e rounded once and acc = fma(p, e, acc)
//     with them (never |x|^2 - 2 x.t + |t|^2: at near-ties its cancellation decides the row, kmeans.hip).  The candidate list -- KT pairs
//     (distance, row), ascending in that pair -- lives in registers: a row is compared with the thread's worst first, and only a row that beats it
//     is inserted, by one fully unrolled pass of KT compare-and-swaps (knn_insert: no dynamic register index, so nothing goes to scratch).  The
//     insertion is a divergent branch that soon becomes rare: a list of k among r rows seen changes with probability k / r.  KT is 4, 16 or 32, the
//     least that holds k.  QT = 0 (Q > 64): query and training rows are read from memory.
//     Out: per (slice, query) the first k pairs of its list, rows local to the launch (-1, +inf: no row).
//   knn_fold_kernel: one query per thread; folds the slices in ascending order onto the running list of the call (set by the first chunk of
//     training rows), by the same insertion on the pairs (distance, global row): an equally near row goes behind a lower one at every level.
// Both sides are taken in chunks (host rows are streamed through the plan's buffers, resident rows are read in place), the slice count follows the
// grid (about KNN_BLOCKS workgroups), row indices are chunk offset + local, 64-bit on the way out.  A pair (query, training row) meets the same
// arithmetic wherever a chunk, slice or tile boundary falls, and a list is the k least of a total order: the outputs do not depend on any of them,
// nor on the other queries.  No atomics.  Every buffer belongs to the context's KnnPlan (built on first use, grown on demand, freed with the
// context) and is written before it is read (DA_RAW).  Nothing of the evaluation is touched: only the resident X_mu is read.
#include "gp_common.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace gp {

constexpr int KNN_TILE = 2048;    // doubles of training rows per LDS buffer (two buffers: 32 KB)
constexpr int KNN_PF = KNN_TILE / 256;      // doubles a thread fetches per tile
constexpr int KNN_MROWS = 64;     // QT = 0: training rows per "tile" (the unit the slices are counted in)
constexpr int KNN_BLOCKS = 2048;  // workgroups a launch aims at: the slices of the training rows make up what the blocks of queries leave
constexpr int KNN_KMAX = 32;

// (d, r) before (od, orow) in the order of the lists: nearer, or equally near with a lower row; no row (-1) is the largest row
template <typename R>
__device__ __forceinline__ bool knn_less(double d, R r, double od, R orow) {
  using U = std::make_unsigned_t<R>;
  return d < od || (d == od && (U)r < (U)orow);
}

// the sorted list (d, r)[0 .. KT) takes the pair (cd, cr), which comes before its last one: every pair behind (cd, cr) moves down one (the last one
// leaves), from the end upwards, so that a step reads two neighbours and writes the lower one in place
template <int KT, typename R>
__device__ __forceinline__ void knn_insert(double (&d)[KT], R (&r)[KT], double cd, R cr) {
#pragma unroll
  for (int j = KT - 1; j > 0; --j) {
    const bool up = knn_less(cd, cr, d[j - 1], r[j - 1]);       // the pair above moves down into j
    const bool here = knn_less(cd, cr, d[j], r[j]);             // else (cd, cr) lands in j, or j keeps its pair
    d[j] = up ? d[j - 1] : here ? cd : d[j];
    r[j] = up ? r[j - 1] : here ? cr : r[j];
  }
  const bool here = knn_less(cd, cr, d[0], r[0]);
  d[0] = here ? cd : d[0];
  r[0] = here ? cr : r[0];
}

// X [cnt][Q] the queries; T [rows][Q] the training rows of the launch; w [QT] (Q for QT = 0) the weights, 0 beyond Q (read only when WT);
// tr rows per tile (tr QT <= KNN_TILE), tps tiles per slice; skip [cnt] (or NULL) the GLOBAL training row a query leaves out (-1: none), self0
// >= 0 (with skip NULL): query i leaves out the global row self0 + i; tbase: the global row of T's first; pd, pi [gridDim.y][cnt][k]
template <int QT, int KT, bool WT>
__global__ void __launch_bounds__(256) knn_search_kernel(const double* __restrict__ X, long cnt, const double* __restrict__ T, long rows, int Q, int tr,
                                                         int tps, const double* __restrict__ w, const long long* __restrict__ skip, long long self0,
                                                         long long tbase, int k, double* __restrict__ pd, int* __restrict__ pi) {
  constexpr int QS = QT > 0 ? QT : 1;
  __shared__ double tile[QT > 0 ? 2 * KNN_TILE : 1];
  const int tid = threadIdx.x;
  const long i = blockIdx.x * 256L + tid;
  const bool live = i < cnt;
  const double* xr = X + (live ? i : 0) * Q;
  long long sk = -1;                                    // the row of T this query leaves out (outside [0, rows): none)
  if (live) {
    const long long g = skip ? skip[i] : (self0 >= 0 ? self0 + i : -1);
    sk = g >= 0 ? g - tbase : -1;
  }
  const long tiles = (rows + tr - 1) / tr;
  const long t0 = (long)blockIdx.y * tps, t1 = min(tiles, t0 + tps);      // t0 < t1: the grid has no empty slice

  double d[KT];
  int r[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) { d[j] = std::numeric_limits<double>::infinity(); r[j] = -1; }

  if constexpr (QT > 0) {
    double x[QS];
#pragma unroll
    for (int q = 0; q < QT; ++q) x[q] = (q < Q) ? xr[q] : 0.0;
    double f[KNN_PF];
    // tile t into registers: element e of the tile is coordinate e % QT of its row e / QT; zeros beyond Q, beyond the tile's rows and beyond the
    // launch's (nothing outside T[0, rows) is read)
    auto fetch = [&](long t) {
#pragma unroll
      for (int j = 0; j < KNN_PF; ++j) {
        const int e = tid + j * 256, row = e / QT, q = e % QT;
        const long g = t * tr + row;
        f[j] = (row < tr && g < rows && q < Q) ? T[g * Q + q] : 0.0;
      }
    };
    auto put = [&](int b) {
#pragma unroll
      for (int j = 0; j < KNN_PF; ++j) tile[b * KNN_TILE + tid + j * 256] = f[j];
    };
    fetch(t0);
    put(0);
    __syncthreads();
    for (long t = t0; t < t1; ++t) {
      const int b = (int)(t - t0) & 1;
      const bool more = t + 1 < t1;
      if (more) fetch(t + 1);
      const int kt = (int)min((long)tr, rows - t * tr);
      const int row0 = (int)(t * tr);
#pragma unroll 2
      for (int kk = 0; kk < kt; ++kk) {
        const double* z = tile + b * KNN_TILE + kk * QT;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
          const double e = x[q] - z[q];
          if constexpr (WT) s = fma(__dmul_rn(w[q], e), e, s);
          else s = fma(e, e, s);
        }
        const int row = row0 + kk;
        if (row != sk && knn_less(s, row, d[KT - 1], r[KT - 1])) knn_insert<KT>(d, r, s, row);
      }
      // the other buffer was last read in the previous round, which every thread has left (the barrier below)
      if (more) put(b ^ 1);
      __syncthreads();
    }
  } else {
    const long r0 = t0 * tr, r1 = min(rows, t1 * tr);
    for (long g = r0; g < r1; ++g) {
      const double* z = T + g * Q;
      double s = 0.0;
      for (int q = 0; q < Q; ++q) {
        const double e = xr[q] - z[q];
        if constexpr (WT) s = fma(__dmul_rn(w[q], e), e, s);
        else s = fma(e, e, s);
      }
      const int row = (int)g;
      if (row != sk && knn_less(s, row, d[KT - 1], r[KT - 1])) knn_insert<KT>(d, r, s, row);
    }
  }
  if (live) {
    const long o = ((long)blockIdx.y * cnt + i) * k;
#pragma unroll
    for (int j = 0; j < KT; ++j)
      if (j < k) { pd[o + j] = d[j]; pi[o + j] = r[j]; }
  }
}

// bd, bi [cnt][k]: the call's running lists, set when first, else merged with the slices' lists (rows plus tbase, the chunk's first row)
template <int KT>
__global__ void __launch_bounds__(256) knn_fold_kernel(const double* __restrict__ pd, const int* __restrict__ pi, int slices, long cnt, int k,
                                                       long long tbase, int first, double* __restrict__ bd, long long* __restrict__ bi) {
  const long q = blockIdx.x * 256L + threadIdx.x;
  if (q >= cnt) return;
  double d[KT];
  long long r[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    const bool have = !first && j < k;
    d[j] = have ? bd[q * k + j] : std::numeric_limits<double>::infinity();
    r[j] = have ? bi[q * k + j] : -1;
  }
  for (int s = 0; s < slices; ++s) {
    const long o = ((long)s * cnt + q) * k;
    for (int j = 0; j < k; ++j) {
      const int li = pi[o + j];
      if (li < 0) break;                                          // the slice had fewer rows
      const double cd = pd[o + j];
      const long long cr = tbase + li;
      if (!knn_less(cd, cr, d[KT - 1], r[KT - 1])) break;        // nor does any later pair of this slice's list come before the worst
      knn_insert<KT>(d, r, cd, cr);
    }
  }
#pragma unroll
  for (int j = 0; j < KT; ++j)
    if (j < k) { bd[q * k + j] = d[j]; bi[q * k + j] = r[j]; }
}

// test hook (gp_debug_set_option "knn_rows"): rows per chunk of either side, as given (not rounded), with a quarter of it per tile and one tile
// per slice, so that small cases cross every boundary; 0 = the defaults below
std::atomic<int> g_opt_knn_rows{0};

struct KnnPlan {
  DevBuf<double> q;           // [rows][Q] a chunk of host queries (not used with resident queries)
  DevBuf<double> in;          // [rows][Q] a chunk of host training rows (not used with the resident X_mu)
  DevBuf<double> w;           // [QT] the weights, zero beyond Q
  DevBuf<long long> skip;     // [rows] the chunk's skip entries
  DevBuf<double> pd;          // [slices][rows][k] per-slice lists: distances
  DevBuf<int> pi;             // and rows, local to the launch
  DevBuf<double> bd;          // [rows][k] the running lists of the chunk of queries
  DevBuf<long long> bi;
};
void KnnPlanDelete::operator()(KnnPlan* p) const { delete p; }

struct KnnLaunch {
  unsigned qblocks, slices;
  const double* X; long cnt; const double* T; long rows; int Q, tr, tps; const double* w; const long long* skip; long long self0, tbase; int k;
  double* pd; int* pi;
};

template <int QT, int KT, bool WT>
static int knn_launch_search(gp_ctx* c, hipStream_t st, const KnnLaunch& a) {
  GP_LAUNCH(c, st, (knn_search_kernel<QT, KT, WT>), dim3(a.qblocks, a.slices), dim3(256), 0, a.X, a.cnt, a.T, a.rows, a.Q, a.tr, a.tps, a.w, a.skip,
            a.self0, a.tbase, a.k, a.pd, a.pi);
  return GP_OK;
}
template <int QT, int KT>
static int knn_launch_search_w(gp_ctx* c, hipStream_t st, bool weighted, const KnnLaunch& a) {
  return weighted ? knn_launch_search<QT, KT, true>(c, st, a) : knn_launch_search<QT, KT, false>(c, st, a);
}
template <int KT>
static int knn_launch_fold(gp_ctx* c, hipStream_t st, const double* pd, const int* pi, int slices, long cnt, int k, long long tbase, int first, double* bd,
                           long long* bi) {
  GP_LAUNCH(c, st, knn_fold_kernel<KT>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, pd, pi, slices, cnt, k, tbase, first, bd, bi);
  return GP_OK;
}

// X_train / X NULL: the resident X_mu on that side; self: every query leaves out the row of its own index (both sides resident).  n, n_train >= 1
int run_knn(gp_ctx* c, long n_train, const double* X_train, long n, const double* X, const double* weight, int k, const int64_t* skip, bool self,
            double* dist2, int64_t* rows_out) {
  const long Q = c->Q;
  const int QT = psi1_qp((int)Q), QS = QT > 0 ? QT : (int)Q;
  const int KT = k <= 4 ? 4 : k <= 16 ? 16 : KNN_KMAX;
  const int opt = g_opt_knn_rows.load();
  const int tr_max = QT > 0 ? KNN_TILE / QT : KNN_MROWS;
  const int tr = opt > 0 ? std::max(1, std::min(tr_max, opt / 4)) : tr_max;
  // a chunk of host rows [rows][Q] stays near 64 MB, at most 2^20 rows; a chunk of queries is at most 2^17 (its lists: [rows][k] twice)
  const long cap = std::max<long>(256, std::min<long>(1L << 20, (64L << 20) / (8L * Q)));
  const long RQ = std::min(n, opt > 0 ? (long)opt : std::min<long>(cap, 1L << 17));
  const long RT = std::min(n_train, opt > 0 ? (long)opt : cap);
  // slices x queries of a launch: at most ceil(KNN_BLOCKS / blocks) slices of blocks x 256 queries
  const size_t part = ((size_t)KNN_BLOCKS * 256 + (size_t)RQ) * k;
  std::unique_ptr<KnnPlan, KnnPlanDelete> fresh;
  if (!c->knn) fresh.reset(new KnnPlan());
  KnnPlan& p = c->knn ? *c->knn : *fresh;
  if (X) GP_TRY_RC(p.q.grow(c, (size_t)(RQ * Q), DA_RAW));
  if (X_train) GP_TRY_RC(p.in.grow(c, (size_t)(RT * Q), DA_RAW));
  if (weight) GP_TRY_RC(p.w.grow(c, (size_t)QS, DA_RAW));
  if (skip) GP_TRY_RC(p.skip.grow(c, (size_t)RQ, DA_RAW));
  GP_TRY_RC(p.pd.grow(c, part, DA_RAW));
  GP_TRY_RC(p.pi.grow(c, part, DA_RAW));
  GP_TRY_RC(p.bd.grow(c, (size_t)RQ * k, DA_RAW));
  GP_TRY_RC(p.bi.grow(c, (size_t)RQ * k, DA_RAW));
  if (fresh) c->knn = std::move(fresh);                 // published whole: every buffer of this call is in place
  hipStream_t st = c->stream;
  std::vector<double> hw;
  if (weight) {
    hw.assign((size_t)QS, 0.0);
    std::copy(weight, weight + Q, hw.begin());
    GP_HIP(c, hipMemcpyAsync(p.w, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "skip and the rows are copied as they are");
  for (long n0 = 0; n0 < n; n0 += RQ) {
    const long cnt = std::min(RQ, n - n0);
    const double* x = c->Xmu + n0 * Q;
    if (X) {
      GP_HIP(c, hipMemcpyAsync(p.q, X + n0 * Q, (size_t)(cnt * Q) * 8, hipMemcpyHostToDevice, st));
      x = p.q;
    }
    if (skip) GP_HIP(c, hipMemcpyAsync(p.skip, skip + n0, (size_t)cnt * 8, hipMemcpyHostToDevice, st));
    const unsigned qblocks = (unsigned)((cnt + 255) / 256);
    for (long m0 = 0; m0 < n_train; m0 += RT) {
      const long rows = std::min(RT, n_train - m0);
      const double* t = c->Xmu + m0 * Q;
      if (X_train) {
        // one chunk holds all of them: it is still there from the previous chunk of queries
        if (n0 == 0 || RT < n_train) GP_HIP(c, hipMemcpyAsync(p.in, X_train + m0 * Q, (size_t)(rows * Q) * 8, hipMemcpyHostToDevice, st));
        t = p.in;
      }
      const long tiles = (rows + tr - 1) / tr;
      const auto [tps, slices] = opt > 0 ? SlicePlan{1, (int)tiles} : slice_plan(tiles, qblocks, KNN_BLOCKS);      // "knn_rows": a slice per tile
      if ((size_t)slices * cnt * k > part) return fail(c, GP_ERR_UNSUPPORTED, "gp_knn_rows: %d slices of %ld queries exceed the plan's lists", slices, cnt);
      const KnnLaunch a{qblocks, (unsigned)slices, x, cnt, t, rows, (int)Q, tr, tps, weight ? p.w.get() : nullptr, skip ? p.skip.get() : nullptr,
                        self ? (long long)n0 : -1LL, (long long)m0, k, p.pd, p.pi};
      // (width 0: the kernel with a run-time Q, beyond the 64-wide records)
      GP_TRY_RC((for_width<2, 4, 6, 8, 10, 12, 14, 16, 24, 32, 52, 64, 0>(c, "k nearest rows kernel", QT, [&](auto W) {
        return KT == 4 ? knn_launch_search_w<W(), 4>(c, st, weight != nullptr, a)
                       : KT == 16 ? knn_launch_search_w<W(), 16>(c, st, weight != nullptr, a) : knn_launch_search_w<W(), KNN_KMAX>(c, st, weight != nullptr, a);
      })));
      const int first = m0 == 0 ? 1 : 0;
      GP_TRY_RC(KT == 4 ? knn_launch_fold<4>(c, st, p.pd, p.pi, slices, cnt, k, (long long)m0, first, p.bd, p.bi)
                        : KT == 16 ? knn_launch_fold<16>(c, st, p.pd, p.pi, slices, cnt, k, (long long)m0, first, p.bd, p.bi)
                                   : knn_launch_fold<KNN_KMAX>(c, st, p.pd, p.pi, slices, cnt, k, (long long)m0, first, p.bd, p.bi));
    }
    if (dist2) GP_HIP(c, hipMemcpyAsync(dist2 + n0 * k, p.bd, (size_t)(cnt * k) * 8, hipMemcpyDeviceToHost, st));
    if (rows_out) GP_HIP(c, hipMemcpyAsync(rows_out + n0 * k, p.bi, (size_t)(cnt * k) * 8, hipMemcpyDeviceToHost, st));
  }
  GP_HIP(c, hipStreamSynchronize(st));
  ++c->sync_epoch;
  return GP_OK;
}

}  // namespace gp
