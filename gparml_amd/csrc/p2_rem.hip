// Phase 2, fixed embeddings: the ragged last round of row tiles, spread over every workgroup (run_phase2, psi.hip).
//
// p2_fast8_kernel deals whole 128-row tiles to S slices.  With ntiles = q S + r, 0 < r < S, its plan is q + 1 tiles per slice: every workgroup pays for
// q + 1 tile-times and the last round keeps r of S slices busy (headline shape: 7813 = 61 * 128 + 5, 20 of 512 workgroups).  Here the main launch runs q
// full rounds and the last r row tiles -- r * MT tile products of 128 x 128 x (Mp + Dp) -- are cut along k instead:
//   p2_rem_kernel      one workgroup per (tile product, k split): G's partial over a range of whole KC chunks, on the shared eight-wave pieces
//                      (mma_f64.h: Wave8, stage8_kf, kstep8), stored as a 128 x 128 partial tile in the context's workspace
//   p2_rem_fix_kernel  one workgroup per (tile product, row group): adds the partials in ascending split order, W = G o Psi1, and contracts W^T [mu, 1]
//                      and sum_n h_n mu_n^2 into extra rows of Rpart / hgpart that p2_reduce_kernel and colsum2_kernel pick up through their nparts
// No atomics: every sum has one fixed order, and the split boundaries are a function of the shape alone (p2_rem_plan).
#include "gp_common.h"
#include "lane_reduce.h"

namespace gp {

std::atomic<int> g_opt_p2_rem{env_int("GPARML_P2_REM", 1)};

// k-step 0 of a chunk for the first chunk of an accumulator chain: kstep8<0, true> with C = 0 as an inline constant (hipcc does not model the MFMAs
// inside the asm strings; an accumulator zeroed in C++ may be rematerialised in front of the MFMA that reads it: DESIGN.md section 3)
__device__ __forceinline__ void kstep8_first(double (&acc)[4][8], unsigned aA, unsigned aB) {
  double a[4], b[8];
  static_for<0, 4>([&](auto ic) { constexpr int ar = decltype(ic)::value; a[ar] = ds_read64<2048 * ar>(aA); });
  static_for<0, 8>([&](auto jc) { constexpr int j = decltype(jc)::value; b[j] = ds_read64<32 * j>(aB); });
  static_for<0, 8>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    lgkm_wait<7 - j>();
#pragma unroll
    for (int ar = 0; ar < 4; ++ar) mfma444_zero(acc[ar][j], a[ar], b[j]);
  });
}

struct P2RemArgs {
  const double* Kaug; long ld; const double* Bm; const double* Xa;
  double* part;        // [r * MT * splits][128][128] partial tiles of G
  double* Rpart;       // first extra part: [r * RG][Mp][XS]
  double* gapart;      // first extra row: [r * MT * RG][XS]
  int Mp, CXp, MT, t0 /* first remainder row tile */, kbeg, nc /* chunks of the whole k range */, splits, RG;
};

// grid: r * MT * splits workgroups, block = (tile product) * splits + split
__global__ void __launch_bounds__(512, 4) p2_rem_kernel(P2RemArgs p) {
  __shared__ __attribute__((aligned(16))) double lds[2 * 4608];     // two buffers of [A tile | B tile], as p2_fast8_kernel's
  const int tp = blockIdx.x / p.splits, s = blockIdx.x - tp * p.splits;
  const int rt = tp / p.MT, mt = tp - rt * p.MT;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Wave8 w(wave);
  const LaneOfs ofs = lane_offsets<K_CONTIG, FREE_CONTIG>(w.wrow0, w.wcol0, lane);
  // chunks [c0, c1) of the nc: the same count for every split, +-1 (splits <= nc, so none is empty)
  const int c0 = (int)((long)s * p.nc / p.splits), c1 = (int)((long)(s + 1) * p.nc / p.splits);
  const int nc = c1 - c0;
  const long n0 = (long)(p.t0 + rt) * TILE;
  const double* Ab = p.Kaug + n0 * p.ld + (long)(p.kbeg + c0) * KC;
  const double* Bb = p.Bm + (long)(p.kbeg + c0) * KC * p.Mp + (long)mt * TILE;
  const unsigned lds_base = lds_byte_addr(lds);
  double acc[4][8];
  stage8_kf(lds, Ab, Bb, p.ld, p.Mp, wave, lane);
  dma_wait();
  __syncthreads();
  auto chunk = [&](int c, auto first) {
    const int cur = c & 1;
    if (c + 1 < nc) stage8_kf(lds + (cur ^ 1) * 4608, Ab + (long)(c + 1) * KC, Bb + (long)(c + 1) * KC * p.Mp, p.ld, p.Mp, wave, lane);
    const unsigned sbase_b = lds_base + (unsigned)cur * (4608u * 8u);
    const unsigned aB = sbase_b + TILE_LDS_DOUBLES * 8 + 8u * (unsigned)ofs.b[0];
    static_for<0, KC / 4>([&](auto k4c) {
      constexpr int k4 = decltype(k4c)::value;
      if constexpr (k4 == 0 && decltype(first)::value) kstep8_first(acc, sbase_b + 8u * (unsigned)ofs.a[0], aB);
      else kstep8<k4, true>(acc, sbase_b + 8u * (unsigned)ofs.a[k4], aB);
    });
    dma_wait();
    __syncthreads();
  };
  chunk(0, std::true_type{});
  for (int c = 1; c < nc; ++c) chunk(c, std::false_type{});
  mfma_drain(acc[3][7]);
#pragma unroll
  for (int ar = 0; ar < 4; ++ar) acc_fence8(acc[ar]);
  double* out = p.part + (long)blockIdx.x * (TILE * TILE);
#pragma unroll
  for (int ar = 0; ar < 4; ++ar)
#pragma unroll
    for (int j = 0; j < 8; ++j) out[(w.wrow0 + acc_row(ar, lane)) * TILE + w.wcol0 + acc_col(j, lane)] = acc[ar][j];
}

// grid: r * MT * RG workgroups, block = (tile product) * RG + row group; a row group is 128 / RG >= 16 rows.  Thread t owns column t & 127 of the
// tile and every second row of the group, eight rows per pass.
template <int NRB>
__global__ void __launch_bounds__(256) p2_rem_fix_kernel(P2RemArgs p) {
  constexpr int XS = 4 * NRB;
  __shared__ double xa_s[TILE * XS];          // the group's feature rows [rows][XS]
  __shared__ double red[256 * XS];
  const int tp = blockIdx.x / p.RG, rg = blockIdx.x - tp * p.RG;
  const int rt = tp / p.MT, mt = tp - rt * p.MT;
  const int RB = TILE / p.RG, r0 = rg * RB;
  const long n0 = (long)(p.t0 + rt) * TILE + r0;
  const int t = threadIdx.x, col = t & 127, half = t >> 7;
  for (int e = t; e < RB * XS; e += 256) { const int row = e / XS; xa_s[e] = p.Xa[(n0 + row) * p.CXp + (e - row * XS)]; }
  __syncthreads();
  const double* part = p.part + (long)tp * p.splits * (TILE * TILE) + (long)r0 * TILE + col;
  const double* psi1 = p.Kaug + n0 * p.ld + (long)mt * TILE + col;
  double racc[XS], gacc[NRB * 4];
#pragma unroll
  for (int c = 0; c < XS; ++c) { racc[c] = 0.0; gacc[c] = 0.0; }
  for (int rb = half; rb < RB; rb += 16) {          // rows rb, rb + 2, ..., rb + 14
    double g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = part[(rb + 2 * u) * TILE];
    for (int s = 1; s < p.splits; ++s) {
      const double* ps = part + (long)s * (TILE * TILE);
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = ps[(rb + 2 * u) * TILE];
#pragma unroll
      for (int u = 0; u < 8; ++u) g[u] += x[u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = rb + 2 * u;
      const double wv = g[u] * psi1[(long)row * p.ld];
      const double* x = xa_s + row * XS;
#pragma unroll
      for (int c = 0; c < XS; ++c) {
        racc[c] = fma(wv, x[c], racc[c]);
        gacc[c] = fma(wv * x[c], x[c], gacc[c]);   // grad_alpha's mu^2 term, sum_n W[n][m] mu_nq^2 (columns >= Q are never read)
      }
    }
  }
  // R: the two row halves of a column, in order
#pragma unroll
  for (int c = 0; c < XS; ++c) red[t * XS + c] = racc[c];
  __syncthreads();
  if (half == 0) {
    double* Rmine = p.Rpart + ((long)(rt * p.RG + rg) * p.Mp + (long)mt * TILE + col) * XS;
#pragma unroll
    for (int c = 0; c < XS; ++c) Rmine[c] = racc[c] + red[(t + 128) * XS + c];
  }
  __syncthreads();
  // the mu^2 term: fixed tree over the 256 threads, one row of gapart per workgroup
#pragma unroll
  for (int c = 0; c < XS; ++c) red[c * 256 + t] = gacc[c];
  __syncthreads();
  block_fold<256>([&](int i, int j) {
#pragma unroll
    for (int c = 0; c < XS; ++c) red[c * 256 + i] += red[c * 256 + j];
  });
  if (t < XS) p.gapart[(long)blockIdx.x * XS + t] = -0.5 * red[t * 256];
}

// The plan, from the shape alone.  ntiles = q S + r row tiles on S slices: is the remainder worth its own two launches, and how is it cut?
//   r * MT <= 512     the partial tiles fit the workgroups resident at once (and the workspace: its capacity is at least 1100 tiles)
//   r / S <= 1 / 16   past the crossover the round trip of G's partials and the two launches cost more than the idle round saves.  Measured on one MI355X,
//                     phase-2 kernels between their two events, whole-tile plan -> this path, alternating on one context:
//                       M = 512, D = 100, Q = 10 (S = 128, a tile-time of 159 us), ntiles = 4 S + r:
//                         r / S  5/128   16/128  32/128  48/128  64/128  96/128  127/128
//                         us     -110    -96     -77     -37     -42     +40     +43
//                       M = 128, D = 10, Q = 10 (S = 512, the shape of configs[1]), ntiles = S + r:
//                         r / S  8/512   32/512  64/512  128/512  192/512  270/512 (configs[1])  400/512
//                         us     -22     -13     +0      +7       +17      +28                   +31
//                     The crossover moves with the tile-time (0.5 ... 0.75 at M = 512, 0.06 ... 0.125 at M = 128, where the two launches and the reduce's
//                     longer chain weigh more: phase 2 as a whole -8 us at 32/512, +5 us at 64/512); the bound is the largest ratio at which both won.
constexpr int P2_REM_NUM = 1, P2_REM_DEN = 16;
bool p2_rem_plan(int ntiles, int S, int MT, int nc, P2Rem* pl) {
  const int mode = g_opt_p2_rem.load();
  *pl = P2Rem{};
  if (!mode || S <= 0 || nc <= 0) return false;
  const int q = ntiles / S, r = ntiles % S;
  if (q == 0 || r == 0 || (long)r * MT > 512) return false;
  if (mode == 1 && (long)r * P2_REM_DEN > (long)P2_REM_NUM * S) return false;     // mode 2 (the crossover measurements): the hard limits only
  pl->q = q; pl->r = r;
  pl->splits = std::max(1, std::min(512 / (r * MT), nc));
  int rg = 1;
  while (rg < 8 && 2 * rg * r * MT <= 256) rg *= 2;
  pl->RG = rg;
  return true;
}

int run_phase2_rem(gp_ctx* c, const P2Rem& pl, int S, int kbeg, int kend, int nrb, int main_blocks) {
  P2RemArgs p;
  p.Kaug = c->Kaug; p.ld = c->LDK; p.Bm = c->gstep.Bm; p.Xa = c->Xa;
  p.Mp = c->Mp; p.CXp = c->CXp; p.MT = c->Mp / TILE; p.t0 = pl.q * S; p.kbeg = kbeg; p.nc = kend - kbeg; p.splits = pl.splits; p.RG = pl.RG;
  const int xs = 4 * nrb, tps = pl.r * p.MT;
  GP_TRY_RC(c->ws.take(c, (size_t)tps * pl.splits * TILE * TILE, "phase 2 (remainder tiles)", &p.part));
  if ((size_t)(2 * S + pl.r * pl.RG) * c->Mp * xs > c->p2.Rpart.size() || (size_t)(main_blocks * 8 + tps * pl.RG) * xs > c->p2.hgpart.size())
    return fail(c, GP_ERR_STATE, "phase 2 (remainder tiles): %d extra partial rows do not fit Rpart / hgpart", pl.r * pl.RG);
  p.Rpart = c->p2.Rpart + (size_t)2 * S * c->Mp * xs;
  p.gapart = c->p2.hgpart + (size_t)main_blocks * 8 * xs;
  GP_LAUNCH(c, c->stream, p2_rem_kernel, dim3(tps * pl.splits), dim3(512), 0, p);
  return for_width<1, 2, 3>(c, "phase-2 remainder kernel (groups of four feature columns)", nrb,
                            [&](auto W) -> int { GP_LAUNCH(c, c->stream, (p2_rem_fix_kernel<W()>), dim3(tps * pl.RG), dim3(256), 0, p); return GP_OK; });
}

}  // namespace gp
