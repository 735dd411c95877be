// Shared host-side declarations of the gparml HIP library (context, error handling, launch helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstdarg>
#include <atomic>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/gparml_hip.h"
#include "devbuf.h"
#include "lifecycle.h"
#include "mma_f64.h"

namespace gp {

#ifndef GP_I8_DIGITS
#define GP_I8_DIGITS 6     // signed 7-bit digits per operand of the int8 phase-1 prototype (p1i8.hip): 42 bits below the operand's scale
#endif

// run-time switches read from the environment when the library is loaded (or on first use).  A flag that defaults to on is switched off by a value
// starting with '0', one that defaults to off is switched on by a value starting with '1'; anything else leaves the default
inline bool env_flag(const char* name, bool dflt) { const char* e = getenv(name); return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt; }
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline bool env_is(const char* name, const char* value) { const char* e = getenv(name); return e && std::string(e) == value; }

inline long round_up(long x, long m) { return (x + m - 1) / m * m; }
inline int blocks_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }   // grid of a grid-stride kernel over n elements
// nearest.hip, knn.hip: `tiles` tiles of training rows in slices, for a grid of (blocks, slices) workgroups that aims at `target` of them; no empty slice
struct SlicePlan { int tps, slices; };     // tiles per slice, slices
inline SlicePlan slice_plan(long tiles, long blocks, long target) {
  const long want = std::min(tiles, std::max<long>(1, (target + blocks - 1) / blocks)), tps = (tiles + want - 1) / want;
  return {(int)tps, (int)((tiles + tps - 1) / tps)};
}
// latent width of the packed per-point records of psi1_kernel (Q <= 16: Q rounded up to 2) / psi1_wide_kernel (24, 32, 52, 64); 0: none
inline int psi1_qp(int Q) { return Q <= 16 ? (Q + 1) / 2 * 2 : Q <= 24 ? 24 : Q <= 32 ? 32 : Q <= 52 ? 52 : Q <= 64 ? 64 : 0; }

// dense batched GEMM on tile-aligned buffers: C = alpha * op(A) op(B) + beta * C
// A product is built in one expression by gemm_of() and the setters below, at the point of the call; no field is assigned afterwards.
struct GemmP {
  const double* A = nullptr;
  const double* B = nullptr;
  double* C = nullptr;
  long lda = 0, ldb = 0, ldc = 0;
  long sA = 0, sB = 0, sC = 0;  // batch strides (doubles) of the inner batch index
  int K = 0;            // multiple of KC
  double alpha = 0.0, beta = 0.0;
  int tri = 0;          // 0 all tiles, 1 only tiles with row-tile >= col-tile (lower), 2 only upper
  int inner = 1 << 30;  // blockIdx.z = i + inner * o: inner index i uses sA/sB/sC, outer index o uses oA/oB/oC
  long oA = 0, oB = 0, oC = 0;
  int splits = 1;       // split-k: partial tiles go to ws, gemm_splitk_reduce applies alpha/beta (small grids only)
  double* ws = nullptr;
  // X^T X with X lower-triangular (both operands FREE_CONTIG, stored [k][free], zero for k < free): with tri = 1 only the tiles on or below the diagonal
  // are computed, klow = 1 starts their k-range at the tile's first possibly non-zero k = max(row0, col0) (the skipped products are exact zeros:
  // same bits, also under split-k -- the splits keep the full product's boundaries, gemm128_kernel), mirror = 1 stores every off-diagonal tile a second time transposed (the two halves were equal bit for bit before: same k order, and a
  // product does not depend on which factor is the A operand).
  // mirror REQUIRES beta == 0: the transposed element would have to be C0's own transposed element times beta, which none of the kernels reads -- the
  // 32-tile kernel and the split-k reduce would copy beta * C0(r,c) across, the unsplit 128-tile kernel would not mirror at all.  launch_gemm, the one
  // launch site of all three, refuses the combination (a programming error: GP_ERR_STATE before anything is launched), so no kernel is reachable with it
  // (the fused tail of the global step walks gemm32_tile itself and never sets mirror).
  int klow = 0, mirror = 0;
  int big = 0;          // 1: the 128 x 128-tile kernel (with splits) whatever the tile count (the M x M x M products at M >= 1024)
  // the modifiers: each returns the product with one group of fields set
  __host__ __device__ GemmP triangle(int t, int kl = 0, int mir = 0) const { GemmP p = *this; p.tri = t; p.klow = kl; p.mirror = mir; return p; }
  __host__ __device__ GemmP batched(int inner_count) const { GemmP p = *this; p.inner = inner_count; return p; }
  __host__ __device__ GemmP split(int s, double* w) const { GemmP p = *this; p.splits = s; p.ws = w; return p; }
  __host__ __device__ GemmP on_big(int b) const { GemmP p = *this; p.big = b; return p; }
};
// an operand of a product: pointer, leading dimension, inner and outer batch stride (doubles)
template <class T> struct GemmOpT { T* p; long ld; long s = 0, o = 0; };
using GemmIn = GemmOpT<const double>;
using GemmOut = GemmOpT<double>;
// C = alpha op(A) op(B) + beta C over K; every other field keeps GemmP's default
__host__ __device__ inline GemmP gemm_of(GemmIn A, GemmIn B, GemmOut C, int K, double alpha = 1.0, double beta = 0.0) {
  GemmP p;
  p.A = A.p; p.lda = A.ld; p.sA = A.s; p.oA = A.o;
  p.B = B.p; p.ldb = B.ld; p.sB = B.s; p.oB = B.o;
  p.C = C.p; p.ldc = C.ld; p.sC = C.s; p.oC = C.o;
  p.K = K; p.alpha = alpha; p.beta = beta;
  return p;
}
// m, n multiples of TILE; la/lb: Layout of A (free index = rows of C) and B (free index = cols of C).  c may be NULL (the debug hooks).  GP_ERR_STATE,
// with nothing launched, when C meets an operand (checked for batch entry 0 only) or mirror comes with beta != 0; GP_ERR_HIP when a launch is refused
int launch_gemm(gp_ctx* c, hipStream_t st, Layout la, Layout lb, int m, int n, int batch, const GemmP& p);

// index of the scalars at the tail of the packed statistics buffer
enum { SC_SUM_YYT = 0, SC_PSI0 = 1, SC_KL = 2, SC_NLOCAL = 3, SC_COUNT = 8 };
// device scalars produced by the global step (GP_ARR_SCALARS order after the first three)
enum { GS_LOGDET_K = 0, GS_LOGDET_A = 1, GS_F = 2, GS_GRAD_BETA = 3, GS_GRAD_SF2 = 4, GS_FAIL = 5, GS_TR_KIPSI2 = 6, GS_TR_PPSI2 = 7,
       GS_TR_CE = 8, GS_TR_EPSI2E = 9, GS_SUM_V = 10, GS_SUM_AC = 11, GS_SUM_BPSI2 = 12, GS_COUNT = 16 };
// regions of the global step's device buffer GsState::gs: [GS_COUNT] scalars | [8] failure flags (two used) | dots_kernel's partials [8 jobs][64 blocks]
enum { GS_FLAGS = GS_COUNT, GS_HOST = GS_FLAGS + 8 /* what the host reads back: scalars | flags */, GS_DOTS = GS_HOST, GS_TOTAL = GS_DOTS + 8 * 64,
       GS_PROBE = GS_COUNT - 1 /* the last scalar is unused by the step: gp_comm_info's probe borrows it between evaluations */ };

struct P1Plan;     // p1v2.hip
struct I8Plan;     // p1i8.hip
struct BPlan;      // psi2_plan.h
struct PredPlan;   // predict.hip
struct InferPlan;  // infer.hip
struct KmPlan;     // kmeans.hip
struct PcaPlan;    // pca.hip
struct NnPlan;     // nearest.hip
struct JointPlan;  // joint.hip
struct GradPlan;   // grad.hip
struct PathsPlan;  // paths.hip
struct SelPlan;    // select.hip
struct CurvePlan;  // curve.hip
struct ScorePlan;  // score.hip
struct LbfgsPlan;  // lbfgs.hip
struct KnnPlan;    // knn.hip
struct LooPlan;    // loo.hip
struct CondPlan;   // condition.hip
struct SviPlan;    // svi.hip
struct GatherPlan; // gather.hip
struct SviPlanDelete { void operator()(SviPlan* p) const; };
struct P1PlanDelete { void operator()(P1Plan* p) const; };
struct I8PlanDelete { void operator()(I8Plan* p) const; };
struct BPlanDelete { void operator()(BPlan* p) const; };
struct PredPlanDelete { void operator()(PredPlan* p) const; };
struct InferPlanDelete { void operator()(InferPlan* p) const; };
struct KmPlanDelete { void operator()(KmPlan* p) const; };
struct PcaPlanDelete { void operator()(PcaPlan* p) const; };
struct NnPlanDelete { void operator()(NnPlan* p) const; };
struct JointPlanDelete { void operator()(JointPlan* p) const; };
struct GradPlanDelete { void operator()(GradPlan* p) const; };
struct PathsPlanDelete { void operator()(PathsPlan* p) const; };
struct SelPlanDelete { void operator()(SelPlan* p) const; };
struct CurvePlanDelete { void operator()(CurvePlan* p) const; };
struct ScorePlanDelete { void operator()(ScorePlan* p) const; };
struct LbfgsPlanDelete { void operator()(LbfgsPlan* p) const; };
struct KnnPlanDelete { void operator()(KnnPlan* p) const; };
struct LooPlanDelete { void operator()(LooPlan* p) const; };
struct CondPlanDelete { void operator()(CondPlan* p) const; };
struct GatherPlanDelete { void operator()(GatherPlan* p) const; };

}  // namespace gp

// ---- the stages' own state -------------------------------------------------------------------------------------------------------------
// One struct per stage of an evaluation: its buffers and the scalars that go with them.  alloc() holds the stage's size formulas and is called
// once by gp_create (eagerly: nothing here is allocated during an evaluation unless its comment says so); poison() refills, in the test mode
// (devbuf.h, g_opt_poison), what an evaluation must write before it reads.  Both live next to the code that uses the state.  Nothing outside a
// stage's home file writes its struct, except where a comment here names the reader.
namespace gp {

// tile form of phase 1 and the prep kernels' KL partials (psi.hip)
struct P1Tiles {
  DevBuf<int> tiles;          // phase-1 tile table (int2): Psi2 upper tiles first, then the C tiles
  int n_tiles = 0;
  DevBuf<int> bmap;           // phase-1 block -> (slice, tile type) placement table (built for the (T, S) it was last run with)
  int bmap_T = -1, bmap_S = -1, bmap_blocks = 0;
  DevBuf<double> klpart;      // [kl_blocks] partial KL sums of prep_row_kernel (read by the phase-1 scalars kernels; regime B's table kernel uses the same grid)
  int kl_blocks = 0;
  int alloc(gp_ctx* c);
};

// the int8 phase 1's switches and its run-time guard (p1i8.hip, "guard"); gp_i8_status reports them
struct I8Guard {
  bool active = false;        // this evaluation's phase 1 runs on the int8 matrix core (psi1_kernel wrote the digits)
  bool y_valid = false;       // Y's digits are current (reset by gp_upload_shard)
  bool unsupported = false;   // the int8 plan could not be built for this context (falls back to the float64 kernels)
  int guard = 0;              // 0 = not checked since the last upload, 1 = accepted, 2 = rejected (float64 from then on)
  bool check_pending = false; // this evaluation ran both phase-1 paths: gp_finish reads the comparison and decides
  long since_check = 0, checks = 0;
  double rel_psi2 = 0, rel_c = 0, cond_lb = 0;
  DevBuf<double> cmp;         // device: [4] squared Frobenius norms (dPsi2, Psi2, dC, C) | [2] max diag(Psi2), max diag(P) | partials (allocated by the first check)
  void reset() { y_valid = false; guard = 0; since_check = 0; check_pending = false; }   // new data: the int8 path is measured again
};

// the global step (linalg.hip; gsd / gss: gsi8.hip).  Readers elsewhere: phase 2 (Bm, Bbar), gp_predict / gp_infer_* (Inv, Linv, E), the guard (Inv),
// gp_download, gp_finish (gs, gK)
struct GsState {
  DevBuf<double> Kmm;         // batch of 2: [Kmm ; A] -> factorised in place into [Lk ; La]
  DevBuf<double> Lmat;        // [2][Mp][Mp] Cholesky factors
  DevBuf<double> Linv;        // [2][Mp][Mp] inverse factors
  DevBuf<double> Inv;         // [2][Mp][Mp] Ki, P
  DevBuf<double> KmmKeep;     // [Mp][Mp] Kmm (kept for downloads / derivative parts)
  DevBuf<double> T1;          // [Mp][max(Mp, Dp, 256)] scratch
  // [Mp][max(Mp, Dp)] scratch.  The step leaves nothing in it that anyone reads: once the step is enqueued phase 2 borrows its first [M][Q] doubles for
  // the per-row alpha partials (run_phase2: p2_reduce_kernel writes them, colsum2_kernel sums them), and gp_set_local_statistics stages its uploads in it
  DevBuf<double> T2;
  DevBuf<double> dFdK;        // [Mp][Mp]
  DevBuf<double> Bbar;        // [Mp][Mp]
  DevBuf<double> E;           // [Mp][Dp]
  DevBuf<double> PsiE;        // [Mp][Dp]
  DevBuf<double> Abar;        // [Mp][Dp]
  DevBuf<double> Bm;          // [LDK][Mp] = [2 Bbar ; Abar^T]
  DevBuf<double> gs;          // [GS_TOTAL] device scalars | failure flags | dots_kernel's partials (the GS_* regions above)
  DevBuf<double> gK;          // [M*Q + Q] Kmm-parts of grad_Z / grad_alpha (+ regime-B alpha term)
  DevBuf<int8_t> gsd;         // gsi8.hip (M >= 1024): digit planes of the two double-double-grade products on the int8 matrix core
  DevBuf<double> gss;         // their column scales
  double h_gs[GS_COUNT] = {0};
  int gs_status = 0;          // outcome of the last global step once read back (GP_OK, GP_ERR_NOT_PD, GP_ERR_NON_FINITE, GP_RETRY_JITTER)
  std::string gs_msg;
  int jitter_mask = 0;        // bit 0: Kmm, bit 1: Kmm + beta*Psi2 get 1e-7 * I in this global step (partial_terms.py:452-456)
  int retry_mask = 0;         // what a GP_RETRY_JITTER asks the caller to pass to gp_global_step_jitter
  bool svi_step = false;      // the step whose outcome is pending is a gp_svi_step (svi.hip): the second failure flag is Lambda_v's
  int alloc(gp_ctx* c);
  int poison(gp_ctx* c);
};

// phase 2 (psi.hip)
struct P2State {
  DevBuf<double> Rpart;       // [2 (p2_slices + 8) + 512 / MT][Mp][CXp]: (slice, wave-row) partials, then the remainder path's (row tile, row group) ones (p2_rem.hip)
  int p2_slices = 0;
  DevBuf<double> HZp;         // [Mp/128][Np][CZp] per-point partials (one array per 128 inducing columns)
  DevBuf<double> gapart;      // [ga_blocks][Q] per-block alpha partial sums from the per-point kernel
  int ga_blocks = 0;
  DevBuf<unsigned long long> p2prog;  // p2_fast8_kernel: [slices][MT] tile progress of the workgroups of a slice (kept in step for the L2), bases grow per launch (allocated on first use)
  unsigned long long p2_epoch = 0;
  DevBuf<double> hgpart;      // partial sums of the fast path's mu^2 term of grad_alpha (per wave, or per 256 points from p2_ga_kernel)
  int alloc(gp_ctx* c);
  int poison(gp_ctx* c);
};

// resident CG vectors (the gp_cg_* functions, cg.hip): grad_latest/new/old (2,N,Q) each
struct CgState {
  DevBuf<double> g_latest;    // written by gp_phase2 with embedding gradients
  DevBuf<double> g_new;
  DevBuf<double> g_old;
  int alloc(gp_ctx* c);
};

// gp_set_globals (api.hip): pinned host staging (two slots, [M*Q + Q] doubles each, allocated on first use) so that the upload of Z and alpha is a
// true asynchronous copy -- an evaluation then has ONE host synchronisation, the read-back in gp_finish; a slot is reused two calls later
struct GlobSlots {
  PinnedBuf<double> h_glob[2];
  hipEvent_t glob_ev[2] = {nullptr, nullptr};
  int glob_slot = 0;
  long glob_epoch[2] = {-1, -1};   // gp_ctx::sync_epoch when the slot was last handed to zaug_kernel
};

}  // namespace gp

struct gp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t N = 0, Np = 0;   // local shard rows, and padded to TILE
  int D = 0, M = 0, Q = 0;
  int Mp = 0, Dp = 0, LDK = 0;  // padded M, D (multiples of TILE) and the row stride of Kaug = Mp + Dp
  int CX = 0, CXp = 0;          // per-point feature columns [f1(Q), f2(Q), 1], padded to 4
  int CZ = 0, CZp = 0;          // inducing feature columns [1, Z(Q), Z^2(Q)], padded to 4
  int64_t N_global = 0;
  double sf2 = 1, beta = 1, step = 0;
  bool regime_A = true;   // every variance exactly zero (fixed embeddings)
  bool xs_raw = false;    // X_S stored in softplus-inverse space
  gp::Lifecycle life;     // where the context is in its evaluation (lifecycle.h): every entry point raises its events and asks its queries
  // ---- the shard's data and what the prep kernels derive from it ----
  gp::DevBuf<double> Kaug;    // [Np][LDK]  Psi1 | Y
  gp::DevBuf<double> Xmu;     // [N][Q] base means
  gp::DevBuf<double> Xs;      // [N][Q] base variances (raw or actual)
  gp::DevBuf<double> dir;     // [2][N][Q] search direction
  gp::DevBuf<double> mu;      // [Np][Q] trial means
  gp::DevBuf<double> S;       // [Np][Q] trial variances (actual)
  gp::DevBuf<double> U;       // [Np][Q] u = alpha / (alpha S + 1)
  gp::DevBuf<double> PU;      // [Np][2*QP+2] packed [mu | u | ln c1] rows for psi1_kernel (QP = Q rounded up to 2, <= 16)
  gp::DevBuf<double> lnc1;    // [Np] ln(sf2) - 1/2 sum ln(a S + 1)
  gp::DevBuf<double> Xa;      // [Np][CXp] per-point features for the n-contraction
  double sumYY = 0;           // host copy, computed at upload
  // ---- the globals ----
  gp::DevBuf<double> Z;       // [Mp][Q] (rows >= M zero)
  gp::DevBuf<double> alpha;   // [Q]
  gp::DevBuf<double> Zaug;    // [Mp][CZp]
  gp::DevBuf<double> Zt;      // [Q][Mp] the inducing points transposed (kmm_grads_lds_kernel: lanes = inducing points)
  // The origin of the latent space the kernels work in ("Translation of the latent space"): gp_set_globals subtracts it from Z on the host,
  // the prep kernels (psi.hip, predict.hip, infer.hip) from every mean, so Z, Zaug, Zt, mu and every table made from them hold CENTRED coordinates and
  // products of coordinates scale with the spread of the points, not with their offset.  The statistics and every gradient depend on differences only;
  // the two places that need the caller's mu -- the KL term and its derivative -mu -- add the origin back.
  gp::DevBuf<double> shift;   // [Q]
  std::vector<double> h_shift;  // its host copy (empty until the first gp_set_globals)
  // ---- the outputs ----
  gp::DevBuf<double> stats;   // packed: Psi2 [Mp*Mp] | C [Mp*Dp] | scalars [SC_COUNT]
  gp::DevBuf<double> spack;   // Psi2 upper triangle | C [M][D] | scalars: the all-reduce payload across processes (allocated on first use)
  gp::DevBuf<double> grads;   // packed: gZ_data [M*Q] | galpha_data [Q]
  gp::DevBuf<double> gXmu, gXs;   // [N][Q] each: the embedding gradients
  gp::PinnedBuf<double> h_out;  // gp_finish: pinned, mapped [GS_HOST | M*Q + Q] -- finish_kernel writes the evaluation's results straight into it
  gp::DevBuf<double> staging; // landing buffer for a peer copy from a shard on another device (gp_buffer_combine)
  // ---- the stages' own state (each struct above, next to its alloc / poison) and what they may borrow ----
  gp::P1Tiles p1t;
  gp::I8Guard i8;
  gp::GsState gstep;
  gp::P2State p2;
  gp::CgState cg;
  gp::GlobSlots glob;
  gp::Workspace ws;           // the one borrowed workspace (devbuf.h): a stage takes it for the length of its own launches
  gp::DevBuf<double> red;     // [8192] per-block partials of the host-side reductions (sum_YYT at upload, gp_cg_dots, gp_cg_abs)
  // ---- plans of the on-demand features, each built on first use ----
  std::unique_ptr<gp::P1Plan, gp::P1PlanDelete> p1plan;   // regime-A phase-1 plan (job and output tables of p1v2.hip)
  std::unique_ptr<gp::I8Plan, gp::I8PlanDelete> i8plan;   // int8 phase 1 (p1i8.hip): digit buffers, job tables
  std::unique_ptr<gp::BPlan, gp::BPlanDelete> bplan;          // regime B (variances > 0): the pairwise psi2 kernels' plan (psi2_plan.h)
  std::unique_ptr<gp::PredPlan, gp::PredPlanDelete> pred;     // gp_predict's buffers (predict.hip)
  std::unique_ptr<gp::InferPlan, gp::InferPlanDelete> infer;  // gp_infer_objective / gp_infer_latent's buffers (infer.hip)
  std::unique_ptr<gp::KmPlan, gp::KmPlanDelete> km;          // gp_kmeans_accumulate's buffers (kmeans.hip)
  std::unique_ptr<gp::PcaPlan, gp::PcaPlanDelete> pca;       // gp_scatter_accumulate / gp_project_rows' buffers (pca.hip)
  std::unique_ptr<gp::NnPlan, gp::NnPlanDelete> nn;          // gp_nearest_rows' buffers (nearest.hip)
  std::unique_ptr<gp::JointPlan, gp::JointPlanDelete> joint;  // gp_predict_joint / gp_predict_sample's buffers (joint.hip)
  std::unique_ptr<gp::GradPlan, gp::GradPlanDelete> grad;     // gp_predict_grad's buffers (grad.hip)
  std::unique_ptr<gp::PathsPlan, gp::PathsPlanDelete> paths;  // gp_paths_set's draws and gp_paths_eval's buffers (paths.hip)
  std::unique_ptr<gp::SelPlan, gp::SelPlanDelete> sel;        // gp_select_begin's state: rows, factor, conditional variances (select.hip)
  std::unique_ptr<gp::CurvePlan, gp::CurvePlanDelete> curve;  // gp_curve_energy's buffers (curve.hip)
  std::unique_ptr<gp::ScorePlan, gp::ScorePlanDelete> score;  // gp_predict_score's buffers (score.hip)
  std::unique_ptr<gp::LbfgsPlan, gp::LbfgsPlanDelete> lbfgs;  // gp_lbfgs_begin .. gp_lbfgs_end: the history vectors (lbfgs.hip)
  std::unique_ptr<gp::KnnPlan, gp::KnnPlanDelete> knn;        // gp_knn_rows' buffers (knn.hip)
  std::unique_ptr<gp::LooPlan, gp::LooPlanDelete> loo;        // gp_loo_score's buffers (loo.hip)
  std::unique_ptr<gp::CondPlan, gp::CondPlanDelete> cond;     // gp_condition_set's rows [V | T] and gp_condition_predict's buffers (condition.hip)
  std::unique_ptr<gp::SviPlan, gp::SviPlanDelete> svi;        // gp_svi_begin .. gp_svi_end: q(v) in natural parameters and the whitened statistics (svi.hip)
  std::unique_ptr<gp::GatherPlan, gp::GatherPlanDelete> gather;  // gp_gather_shard / gp_scatter_embeddings: the index list and the dense Y rows (gather.hip)
  void* comm = nullptr;       // RCCL communicator of this context's rank (comm.hip; NULL until gp_comm_init)
  int comm_ranks = 0, comm_rank = -1;
  // timing: 2 = HIP events around every phase and the dominant kernels (gp_last_timings reports all eight numbers; the default), 1 = only the
  // evaluation's first and last event (total_ms), 0 = none.  Every recorded event is a signal packet the stream waits on: ~4-7 us of idle
  // stream each, thirteen per evaluation -- 0.3 % of an evaluation at configs[2]'s size, 15 % at configs[1]'s (gp_set_timing)
  int timing = [] { const int t = gp::env_int("GPARML_TIMING", 2); return t >= 0 && t <= 2 ? t : 2; }();
  long sync_epoch = 0;        // stream synchronisations seen so far (gp_set_globals' pinned slots are reused without an event once one has passed)
  hipEvent_t ev[14] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double t_ms[5] = {0, 0, 0, 0, 0};
};

namespace gp {
extern thread_local std::string g_create_error;
// element counts of the padded statistics buffer, of the gradient sums and of the packed all-reduce payload (Psi2's upper triangle | C | scalars)
inline int64_t stats_doubles(const gp_ctx* c) { return (int64_t)c->Mp * c->Mp + (int64_t)c->Mp * c->Dp + SC_COUNT; }
inline int64_t grads_doubles(const gp_ctx* c) { return (int64_t)c->M * c->Q + c->Q; }
inline int64_t spack_doubles(const gp_ctx* c) { return (int64_t)c->M * (c->M + 1) / 2 + (int64_t)c->M * c->D + SC_COUNT; }
// poison mode (devbuf.h, g_opt_poison): refills a buffer an evaluation must write before it reads (the stages' poison() and api.hip's poison_scratch)
inline hipError_t poison_fill(gp_ctx* c, const DevBuf<double>& b) { return b.size() ? hipMemsetAsync(b, 0xFF, b.bytes(), c->stream) : hipSuccess; }

// api.hip: sum_YYT of a dense device array [n] in the one summation order of the statistic (gp_upload_shard, gp_gather_shard); synchronises the stream
int sum_yyt(gp_ctx* c, const double* dY, long n, double* out);
// psi.hip
int run_upload_y(gp_ctx* c, const double* dY);
int run_prep_and_generate(gp_ctx* c);
int run_phase1(gp_ctx* c);
int run_phase2(gp_ctx* c);
bool p2_fast_mode(const gp_ctx* c);
// psi1.hip
int run_psi1(gp_ctx* c, bool kfix);      // Psi1 of the prepared trial point into Kaug (kfix: every variance zero, the fixed-variance form)
int launch_psi1_rows(gp_ctx* c, const double* mu, const double* U, const double* lnc1, double* out, long n, long rows, long ld);
// p2_rem.hip (fixed-embedding phase 2: the ragged last round of row tiles, cut along k)
struct P2Rem { int q = 0, r = 0, splits = 0, RG = 0; };   // ntiles = q S + r; k splits per tile product; row groups per tile product in the fix-up
bool p2_rem_plan(int ntiles, int S, int MT, int nc, P2Rem* pl);    // false: the whole-tile plan stands
int run_phase2_rem(gp_ctx* c, const P2Rem& pl, int S, int kbeg, int kend, int nrb, int main_blocks);
// p1i8.hip (regime A phase 1 on the int8 matrix core)
bool p1i8_applicable(const gp_ctx* c);
bool p1i8_applicable_static(const gp_ctx* c);     // the shape / regime conditions alone (not the opt-in switch, not the guard)
int p1i8_prepare(gp_ctx* c, int8_t** Sl, long* strideJ, double** Dpart, int row_blocks);
int run_phase1_i8(gp_ctx* c);
int p1i8_check_begin(gp_ctx* c);      // after run_phase1_i8: keep the int8 statistics aside (the caller then runs the float64 phase 1)
int p1i8_check_compare(gp_ctx* c);    // after the float64 phase 1: norms of the difference (device)
int p1i8_check_finish(gp_ctx* c);     // gp_finish, after the stream synchronisation of a checked evaluation: decide
// p1v2.hip (regime A phase 1 without wasted tile slots)
bool p1v2_applicable(const gp_ctx* c);
int run_phase1_v2(gp_ctx* c);
// psi2.hip (regime B; the psi2 trio's own declarations: psi2_plan.h)
int run_generate_b(gp_ctx* c);
int run_phase1_b(gp_ctx* c);
int run_phase2_b(gp_ctx* c);
int b_poison(gp_ctx* c);                                              // poison mode: refills the plan's per-evaluation buffers (BPlan::poisoned)
int b_point_tables(gp_ctx* c, const double** LE, bool* le_il, const double** Vn, const double** DZ2);   // compat: runs dz2_kernel, hands out the tables
const double* b_debug_table(const gp_ctx* c, bool lea, long* n);      // gp_debug_peek: LE or LEA, NULL / 0 without a plan
// lea.hip: LE (NULL: not wanted) and LEA [rows][Mp] of the points in the rows of mu, w, v2 (row stride ld) and lnc2h (stride ldl) against the rows of
// Z (stride ldz), Q latent dimensions; rows >= cnt and columns >= M get kPadLog; rows a mask (NULL: none) switches off are not written
struct LeaRows {
  const double* mu; const double* w; const double* v2; long ld; const double* lnc2h; long ldl; const double* Z; long ldz;
  int Q; long cnt, rows; int M, Mp; const unsigned char* mask; double* LE; double* LEA;
};
int launch_lea_rows(gp_ctx* c, hipStream_t st, const LeaRows& a);
// predict.hip (its chunk pipeline, which the other features at new inputs share: pred_chunk.h)
int run_predict(gp_ctx* c, long n, const double* X_mu, const double* X_S, int raw, int flags, double* mean, double* var);
// score.hip
int run_predict_score(gp_ctx* c, long n, const double* X_mu, const double* X_S, int raw, bool resident, bool resident_S, const double* Y,
                      const uint8_t* observed, int flags, double* row_logp, double* row_sse, double* row_chi2, double* cols);
// loo.hip (the arguments have been checked: api.hip)
int run_loo_score(gp_ctx* c, int block, const uint8_t* observed, int flags, double* row_logp, double* row_sse, double* row_chi2, double* lev,
                  double* var_loo, double* cols);
// condition.hip (the arguments have been checked: api.hip)
int run_condition_set(gp_ctx* c, long m, const double* Xc, const double* Yc);
bool cond_plan_current(gp_ctx* c);                                   // a set of the model as it is now; a stale one is dropped
int run_condition_predict(gp_ctx* c, long n, const double* X, int flags, double* mean, double* var, double* reduction);
// joint.hip
int run_predict_joint(gp_ctx* c, long n, const double* X, int flags, double* mean, double* cov);
int run_predict_sample(gp_ctx* c, long n, const double* X, int flags, double jitter, int n_draws, const double* eps, double* out, double* mean);
// paths.hip
long paths_operand_bytes(const gp_ctx* c, int n_draws, int F);       // the packed operand [Wt ; -G ; E] of gp_paths_set (its size limit: api.hip)
int run_paths_set(gp_ctx* c, int n_draws, int F, const double* omega, const double* centre, const double* w, const double* eps_u);
bool paths_plan_current(gp_ctx* c);                                  // a plan of the model as it is now; a stale one is dropped
int run_paths_eval(gp_ctx* c, long n, const double* X, double* out, double* mean);
int paths_plan_draws(const gp_ctx* c);                               // n_draws of the plan (there is one)
int run_paths_grad(gp_ctx* c, long n, const double* X, int flags, const double* weights, double* jac, double* grad, double* metric, double* mean_jac);
// grad.hip
int run_predict_grad(gp_ctx* c, long n, const double* X, double* jac, double* dvar, double* metric, double* logdet);
// curve.hip
int run_curve_energy(gp_ctx* c, long n_curves, int T, const double* X, double* energy, double* seg, double* grad);
// infer.hip
int run_infer(gp_ctx* c, int mode, long n, const double* Y, const int* cols, int n_cols, double* X_mu, double* X_S, int raw, int max_iters, double gtol,
              double* L, double* grad_mu, double* grad_S, int* iters);
int run_infer_rows(gp_ctx* c, int mode, long n, const double* Y, const unsigned char* observed, double* X_mu, double* X_S, int raw, int max_iters,
                   double gtol, double* L, double* grad_mu, double* grad_S, int* iters);
const double* infer_debug_lea(const gp_ctx* c, long* n);              // gp_debug_peek: the chunk's LEA, NULL / 0 without a plan
// gp_debug_peek "infer_x", "_gn", "_go", "_d", "_Scur", "_sc", "_si" (ints: *ints set), "_xe", "_fe", "_ge": NULL / 0 before gp_infer_latent, NULL / -1 unknown
const void* infer_debug_scg(const gp_ctx* c, const char* name, long* cnt, bool* ints);
// kmeans.hip
int run_kmeans(gp_ctx* c, long n, const double* X, int K, const double* centres, double* sums, int64_t* counts, double* dist2, int32_t* labels);
// select.hip (the plan lives from gp_select_begin to gp_select_end; the entry points check its presence and the arguments: api.hip)
long select_bytes(const gp_ctx* c, long n, int K, bool host_rows);     // device bytes a plan of this size takes
int run_select_begin(gp_ctx* c, long n, const double* X, int K, double sf2, const double* alpha, double tol);
int run_select_run(gp_ctx* c, int steps, int32_t* n_done, int64_t* rows, double* trace);
int run_select_candidate(gp_ctx* c, double* d, int64_t* row, double* x, double* l);
int run_select_apply(gp_ctx* c, const double* x_p, const double* l_p, double d_p, int64_t own_row, double* trace);
void select_info(const gp_ctx* c, long* n, int* K, int* j);
const double* select_debug(const gp_ctx* c, bool want_L, long* cnt);   // gp_debug_peek: the factor's written columns or d, NULL / 0 without a plan
// cg.hip: the one rule of gp_cg_* and gp_lbfgs_* (`who`): shard data, then free embeddings; `what`: the message's subject and verb, "resident CG vectors exist"
int resident_ready(gp_ctx* c, const char* who, const char* what);
// lbfgs.hip
const double* lbfgs_debug(const gp_ctx* c, const char* name, long* cnt);     // gp_debug_peek: "lbfgs_s<k>", "lbfgs_y<k>", "lbfgs_g"; NULL / 0 for a vector that holds nothing
// pca.hip
int run_scatter(gp_ctx* c, long n, const double* Y, const double* centre, double* sum, double* gram);
int run_project(gp_ctx* c, long n, const double* Y, const double* mean, const double* P, int Q, double* X);
// nearest.hip
int run_nearest(gp_ctx* c, long n_train, const double* Y_train, long n, const double* Y_test, const int* cols, int n_cols, const uint8_t* observed,
                double* dist2, int64_t* index, double* x_near);
// knn.hip (X_train / X NULL: the resident X_mu on that side; self: every query leaves out its own row; the arguments are checked in api.hip)
int run_knn(gp_ctx* c, long n_train, const double* X_train, long n, const double* X, const double* weight, int k, const int64_t* skip, bool self,
            double* dist2, int64_t* rows);
// compat.hip
int compat_build(gp_ctx* c, int which, DevBuf<double>& out);
// comm.hip
void comm_free(gp_ctx* c);
// linalg.hip
int run_global_step(gp_ctx* c);
// pieces of the global step that gp_svi_step runs on its own matrices: K_mm (into Kmm, and GsState::KmmKeep) with A = K_mm + beta Psi2, the trace jobs'
// partial sums part [jobs][DOT_BLOCKS], and the K_mm parts of grad_Z / grad_alpha from GsState's dFdK and Bbar into gK
struct DotJob { const double* x; const double* y; long ld; int rows, cols; int slot; };    // sum over the rows x cols block of x o y -> out[slot]
struct DotJobs { DotJob j[8]; int n; };
constexpr int DOT_BLOCKS = 64;
int launch_build_kmm(gp_ctx* c, hipStream_t st, double* Kmm, double* A, double jitK, double jitA, double* gs_zero /*[GS_HOST] zeroed*/, double* Acopy);
int launch_dots(gp_ctx* c, hipStream_t st, const DotJobs& jobs, double* part);
int launch_kmm_grads(gp_ctx* c, hipStream_t st);
// gsi8.hip: the global step's two double-double-grade products on the int8 matrix core (M >= 1024)
bool gs_i8_wanted(const gp_ctx* c);
int run_gs_i8_product(gp_ctx* c, hipStream_t st, const double* A, long lda, int nA, const double* B, long ldb, int nB, int K, double* out, long ldo,
                      const double* Csub);
int check_global(gp_ctx* c);
// the same with the scalars + failure flags already on the host (h = [GS_HOST] doubles, or NULL when nothing is pending)
int check_global_from(gp_ctx* c, const double* h);
// PRECONDITION: the 128-blocks of Linv strictly above the block diagonal must be ZERO on entry -- they are never written here and
// Inv = Linv^T Linv reads the whole matrix.  GsState::alloc allocates Linv zeroed and nothing else writes those blocks; the test hook
// gp_debug_potrf_inverse memsets its own buffer.  A caller that hands in a reused scratch buffer must clear it first.
int potrf_inverse_batched(gp_ctx* c, hipStream_t st, int Mp, int batch, double* A /*in: SPD, out: L*/, double* Linv, double* Inv,
                          double* Twork /*batch * Mp * Mp / 2 doubles*/, double* logdet2 /*device, [batch]*/, double* fail_flag /*device, [batch]*/,
                          double* splitk_ws /*may be NULL*/, size_t splitk_cap = 0, bool factor_only = false, bool no_inverse = false /*L and L^-1 only*/);
int potrf_trinv128_tiles(gp_ctx* c, hipStream_t st, int tiles, double* A /*[tiles][128][128] in: SPD, out: L*/, double* Linv, double* fail /*[tiles], zero*/,
                         double* logdet2 /*[tiles], zero*/);
extern bool g_force_staging;                                  // debug.hip (gp_debug_force_staging): gp_buffer_combine takes its cross-device path on one device
// the options of gp_debug_set_option (debug.hip holds the table), each next to the code it switches; g_opt_poison and g_alloc_fail_after: devbuf.h
extern std::atomic<int> g_opt_dd_kipsi2, g_opt_refine_E, g_opt_xtx_tri, g_opt_residual_dd, g_opt_trtri_rec, g_opt_gemm_big, g_opt_gs_tail;   // linalg.hip
extern std::atomic<int> g_opt_p1_i8, g_opt_i8_guard_strict;   // p1i8.hip
extern std::atomic<int> g_opt_gs_i8;                          // gsi8.hip
extern std::atomic<int> g_opt_p2_rem;                         // p2_rem.hip: 0 off, 1 on where the remainder rule admits it, 2 on wherever it fits (measurements)
extern std::atomic<int> g_opt_pred_rows, g_opt_inf_rows, g_opt_km_rows;   // predict.hip, infer.hip, kmeans.hip (and pca.hip: the same switch)
extern std::atomic<int> g_opt_nn_rows;                        // nearest.hip
extern std::atomic<int> g_opt_knn_rows;                       // knn.hip
extern std::atomic<int> g_opt_paths_rows;                     // paths.hip: rows per chunk of gp_paths_eval (gp_paths_grad: k / Q points)
extern std::atomic<int> g_opt_sel_rows;                       // select.hip: host rows per upload chunk of gp_select_begin
extern std::atomic<int> g_opt_curve_curves;                   // curve.hip: curves per chunk of gp_curve_energy
extern std::atomic<int> g_opt_inf_patterns;                   // infer.hip: distinct patterns per chunk of gp_infer_*_rows
// layout of the free-embedding LE table (csrc/psi2.hip, b_le_kernel): four points interleaved up to the 16-wide latent tables, point-major beyond
__host__ __device__ constexpr bool le_interleaved(int QT) { return QT <= 16; }
__host__ __device__ inline long le_index(bool il, long n, long m, long Mp) { return il ? ((((n >> 2) * Mp + m) << 2) + (n & 3)) : n * Mp + m; }


// Calls f(std::integral_constant<int, W>) for the W among Ws that equals w and returns its status: the one place a run-time latent width picks a
// compile-time instantiation.  A width outside the list is GP_ERR_UNSUPPORTED, never the nearest kernel.  (A left fold: the compiler then emits the
// kernels in the order of the list, as a switch did.)
template <int... Ws, typename F>
int for_width(gp_ctx* c, const char* what, int w, F&& f) {
  int rc = GP_OK;
  const bool found = (... || (w == Ws && ((rc = f(std::integral_constant<int, Ws>{})), true)));
  return found ? rc : fail(c, GP_ERR_UNSUPPORTED, "%s: no instantiation for the latent table width %d", what, w);
}

}  // namespace gp

// event i of the context's timing set, if the timing level asks for it (levels: gp_ctx::timing)
#define GP_EV(c, i) do { if ((c)->timing >= 2 || ((c)->timing == 1 && ((i) == 0 || (i) == 6))) (void)hipEventRecord((c)->ev[i], (c)->stream); } while (0)
#define GP_TRY_RC(x) do { int rc__ = (x); if (rc__ != GP_OK) return rc__; } while (0)
#define GP_HIP(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) return gp::fail(ctx, GP_ERR_HIP, "%s failed: %s (%s:%d)", #call,      \
                                            hipGetErrorString(e__), __FILE__, __LINE__);           \
  } while (0)
// The one way to launch a kernel: the launch is checked where it is made, and a refused one is reported by the kernel's name before anything else is
// enqueued.  `kernel` may be a parenthesised template name, (psi1_kernel<QP, true>); ctx may be NULL.  Returns from the enclosing function on failure.
#define GP_LAUNCH(ctx, stream, kernel, grid, block, lds_bytes, ...)                                \
  do {                                                                                            \
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, __VA_ARGS__);                      \
    hipError_t e__ = hipGetLastError();                                                           \
    if (e__ != hipSuccess) return gp::fail(ctx, GP_ERR_HIP, "launch of %s failed: %s (%s:%d)", #kernel, \
                                            hipGetErrorString(e__), __FILE__, __LINE__);           \
  } while (0)
