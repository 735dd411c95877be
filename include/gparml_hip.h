/*
 * gparml_hip.h -- C ABI of the MI355X (gfx950) implementation of GParML's per-shard
 * `partial_terms` hot path.  Plain C: opaque context, plain pointers and sizes, int status codes.
 *
 * The reference (markvdw/GParML) has no FFI; the hot path sits behind a Python class and a Python
 * MapReduce backend module.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  The Python host side (gparml_amd/) binds this library
 * with ctypes and mirrors the reference's class/module surface; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - all host arrays are C-contiguous float64, owned by the caller, copied during the call;
 *   - one context per GPU/shard; calls on one context are serialised by the caller;
 *   - every function returns GP_OK (0) or an error code; gp_last_error(ctx) gives the message;
 *   - alpha is the inverse squared lengthscale (ard**-2), sf2 the signal variance, beta the noise
 *     precision -- the argument meaning of partial_terms.__init__ (partial_terms.py:16-36).
 *
 * One evaluation (parallel_GPLVM.py:222-279) is
 *   gp_set_globals -> gp_phase1 -> [gp_stats_pack, all-reduce gp_stats_packed_buffer, gp_stats_unpack] -> gp_global_step
 *                  -> gp_phase2 -> [all-reduce gp_grads_buffer] -> gp_finish
 */
#ifndef GPARML_HIP_H
#define GPARML_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gp_ctx gp_ctx;

/* status codes; the Python wrapper maps them to the exception classes the reference raises
 * (scg_adapted.py:55 catches LinAlgError / ZeroDivisionError / ValueError / AssertionError) */
enum {
  GP_OK = 0,
  GP_ERR_BAD_ARG = 1,      /* -> AssertionError / ValueError (kernel_exp.py:30-34 input assertions)        */
  GP_ERR_NOT_PD = 2,       /* -> numpy.linalg.LinAlgError (linalg.inv / slogdet sign, partial_terms.py:459) */
  GP_ERR_NON_FINITE = 3,   /* -> FloatingPointError (nputil.py:9 np.seterr(all='raise'))                    */
  GP_ERR_HIP = 4,          /* -> RuntimeError                                                               */
  GP_ERR_STATE = 5,        /* call sequence violated (e.g. phase2 before global_step) -> RuntimeError       */
  GP_ERR_UNSUPPORTED = 6,
  GP_RETRY_JITTER = 7,     /* a Cholesky factorisation failed for the first time: repeat the global step with gp_global_step_jitter */
  GP_ERR_RCCL = 8          /* RCCL missing (dlopen) or a collective failed -> RuntimeError                                        */
};

/* what gp_download can fetch (every array the reference exposes on the path) */
enum {
  GP_ARR_KMM = 0,            /* (M,M)   partial_terms.Kmm                 partial_terms.py:94  */
  GP_ARR_KMM_INV = 1,        /* (M,M)   partial_terms.Kmm_inv             partial_terms.py:95  */
  GP_ARR_PSI1 = 2,           /* (N_s,M) partial_terms.exp_K_mi            partial_terms.py:49  */
  GP_ARR_PSI2_SUM = 3,       /* (M,M)   sum_exp_K_mi_K_im                 partial_terms.py:79  */
  GP_ARR_PSI1TY = 4,         /* (M,D)   exp_K_miY                         partial_terms.py:80  */
  GP_ARR_KMM_PLUS_OP_INV = 5,/* (M,M)   Kmm_plus_op_inv                   partial_terms.py:82  */
  GP_ARR_DF_DKMM = 6,        /* (M,M)   dF_dKmm()                         partial_terms.py:102 */
  GP_ARR_DF_DPSI1TY = 7,     /* (M,D)   dF_dexp_K_miY()                   partial_terms.py:115 */
  GP_ARR_DF_DPSI2 = 8,       /* (M,M)   dF_dexp_K_mi_K_im()               partial_terms.py:123 */
  GP_ARR_GRAD_X_MU = 9,      /* (N_s,Q) grad_X_mu()                       partial_terms.py:367 */
  GP_ARR_GRAD_X_S = 10,      /* (N_s,Q) grad_X_S()                        partial_terms.py:400 */
  GP_ARR_SCALARS = 11,       /* 8 doubles: sum_YYT, sum_exp_K_ii, KL, logdet Kmm, logdet A, F, grad_beta, grad_sf2 */
  GP_ARR_PSI2_POINTS = 12,   /* (N_s,M,M) exp_K_mi_K_im, compat only      partial_terms.py:45  */
  GP_ARR_DKMM_DZ = 13,       /* (M,Q,M) dKmm_dZ()                         partial_terms.py:146 */
  GP_ARR_DPSI1TY_DZ = 14,    /* (M,Q,D) dexp_K_miY_dZ()                   partial_terms.py:162 */
  GP_ARR_DPSI2_DZ = 15,      /* (M,Q,M) dexp_K_mi_K_im_dZ()               partial_terms.py:190 */
  GP_ARR_DKMM_DALPHA = 16,   /* (Q,M,M) dKmm_dalpha()                     partial_terms.py:247 */
  GP_ARR_DPSI1TY_DALPHA = 17,/* (Q,M,D) dexp_K_miY_dalpha()               partial_terms.py:256 */
  GP_ARR_DPSI2_DALPHA = 18,  /* (Q,M,M) dexp_K_mi_K_im_dalpha()           partial_terms.py:273 */
  GP_ARR_X_MU_TRIAL = 19,    /* (N_s,Q) X_mu + step*d_mu                  local_MapReduce.py:205-211 */
  GP_ARR_X_S_TRIAL = 20,     /* (N_s,Q) softplus(X_S_raw + step*d_S)      local_MapReduce.py:214 */
  GP_ARR_GRAD_LATEST = 21,   /* (2,N_s,Q) -[grad_X_mu, grad_X_S * softplus'(raw trial)], the .grad_latest.npy of local_MapReduce.py:357-360 */
  GP_ARR_X_MU = 22           /* (N_s,Q) the resident embedding means as uploaded / last updated (the rows gp_kmeans_accumulate clusters with X == NULL) */
};

/* ---- lifetime -------------------------------------------------------------------------------- */
/* partial_terms.__init__ sizes (partial_terms.py:16-30): local shard rows N_s, outputs D, inducing M, latent Q */
int gp_create(gp_ctx** out, int device, int64_t N_s, int D, int M, int Q);
int gp_destroy(gp_ctx* ctx);
const char* gp_last_error(const gp_ctx* ctx);   /* ctx may be NULL: returns the last creation error */
const char* gp_version(void);
/* hipStream_t to launch on (NULL = default stream); lets the host order RCCL collectives with kernels */
int gp_set_stream(gp_ctx* ctx, void* hip_stream);

/* ---- data ------------------------------------------------------------------------------------ */
/* partial_terms.set_data inputs (partial_terms.py:38-43) == what statistics_mapper loads
 * (local_MapReduce.py:197-201).  xs_is_raw != 0: X_S is in softplus-inverse space and is transformed
 * on the device (supporting_functions.py:153-156, local_MapReduce.py:214). */
int gp_upload_shard(gp_ctx* ctx, const double* Y, const double* X_mu, const double* X_S, int xs_is_raw);
/* replace only the embeddings (Y stays resident) */
int gp_upload_embeddings(gp_ctx* ctx, const double* X_mu, const double* X_S, int xs_is_raw);
/* search direction (2,N_s,Q) = [d_mu, d_S] of the optimiser, the .grad_d.npy of
 * local_MapReduce.py:204-211; NULL clears it */
int gp_set_direction(gp_ctx* ctx, const double* d);

/* ---- one evaluation ------------------------------------------------------------------------- */
/* global_statistics Z,sf2,alpha,beta (parallel_GPLVM.py:236-238), global N (options['N']) and the
 * trial step size (options['step_size'], parallel_GPLVM.py:228).
 * Z and the latent means may carry any common offset: the library subtracts an origin (the column mean of Z, kept from call to call while it
 * stays among the inducing points) before it multiplies coordinates; results are translation invariant to the suite's bounds for offsets up to
 * 2^16.  KL and every gradient refer to the caller's coordinates. */
int gp_set_globals(gp_ctx* ctx, const double* Z, double sf2, const double* alpha, double beta,
                   int64_t N_global, double step_size);
/* statistics_mapper body (local_MapReduce.py:224-240 -> partial_terms.set_data / update_local_statistics,
 * partial_terms.py:38-52,74-87): local Psi-statistics into the packed stats buffer */
int gp_phase1(gp_ctx* ctx);
/* packed device buffer the host all-reduces (sum) across shards: the statistics_reducer
 * (local_MapReduce.py:250-277).  Layout: Psi2 (Mp*Mp) | C (Mp*Dp) | sum_YYT, Psi0, KL, n_local, pad(4) */
int gp_stats_buffer(gp_ctx* ctx, void** dev_ptr, int64_t* n_doubles);
/* The same statistics without padding and without the lower triangle, for the all-reduce across processes (what the reducer's twelve
 * accumulated_statistics files carry, local_MapReduce.py:250-277): Psi2 upper triangle, row-major (M(M+1)/2) | C (M*D) | the 8 scalars.
 * gp_stats_pack(ctx) fills it from the statistics buffer (after gp_phase1 and any drop-out scaling), gp_stats_unpack(ctx) writes the
 * reduced values back (both triangles) before gp_global_step.  1.46 MB instead of 2.6 MB at M=512, D=100. */
int gp_stats_packed_buffer(gp_ctx* ctx, void** dev_ptr, int64_t* n_doubles);
int gp_stats_pack(gp_ctx* ctx);
int gp_stats_unpack(gp_ctx* ctx);
/* device-side reduce for several shards in one process (statistics_reducer, local_MapReduce.py:250-277), on one GPU or
 * across GPUs (peer copy into a staging buffer of dst): which=0 statistics buffer, which=1 phase-2 gradient-sum buffer;
 * op=0 dst += src, op=1 dst = src */
int gp_buffer_combine(gp_ctx* dst, const gp_ctx* src, int which, int op);
/* node drop-out (local_MapReduce.py:119-129, 263-264): the reference sums every statistic over the kept nodes only and divides
 * by kept/(kept+dropped).  A dropped shard's contribution is excluded by the caller (factor 0 before the reduction), the reduced
 * buffers are scaled by (kept+dropped)/kept after it: which=0 statistics (before gp_global_step), which=1 gradient sums (after
 * gp_phase2; they are the contracted form of the reference's sum_d_*_d_Z / d_alpha statistics). */
int gp_scale_buffer(gp_ctx* ctx, int which, double factor);
int gp_scale_stats(gp_ctx* ctx, double factor);   /* = gp_scale_buffer(ctx, 0, factor) */
/* ---- the reduce across GPUs inside the library (`allreduce(ctx, phase)`) ------------------------
 * statistics_reducer (local_MapReduce.py:250-277) as an RCCL all-reduce(sum, float64) on the context's stream, one rank per GPU.
 * RCCL is resolved with dlopen at the first of these calls (GP_ERR_RCCL if it cannot be found; GPARML_RCCL_LIB names a specific
 * library), so a single-GPU user never needs it.  Rank 0 obtains the 128-byte ncclUniqueId with gp_comm_unique_id and distributes it;
 * every rank then calls gp_comm_init(ctx, id, nranks, rank) (collective: all ranks must call it).  gp_allreduce(ctx, 0) packs the
 * statistics (gp_stats_pack), all-reduces the packed buffer and unpacks it -- call it between gp_phase1 (and any drop-out scaling)
 * and gp_global_step; gp_allreduce(ctx, 1) all-reduces the gradient sums between gp_phase2 and gp_finish.  Nothing synchronises
 * the host.  A host that prefers its own communicator all-reduces gp_stats_packed_buffer / gp_grads_buffer itself. */
#define GP_COMM_ID_BYTES 128
int gp_comm_unique_id(void* id_out_128_bytes);
int gp_comm_init(gp_ctx* ctx, const void* unique_id_128_bytes, int nranks, int rank);
int gp_allreduce(gp_ctx* ctx, int which);
int gp_comm_destroy(gp_ctx* ctx);
/* Diagnostics for the first multi-GPU run.  gp_comm_available() = GP_OK when RCCL can be resolved in this process (nothing collective
 * happens: every rank can ask before any rank calls gp_comm_init, and a host agrees on the answer over its own channel -- one rank
 * without RCCL would otherwise leave the others waiting inside ncclCommInitRank).  gp_comm_info reports what the communicator of this
 * context saw: nranks / rank as given to ncclCommInitRank (0 / -1 without a communicator), the payload of the two all-reduces in
 * bytes, and -- when probe_sum is not NULL, COLLECTIVE, synchronises the context's stream -- the all-reduced sum of one double 1.0 per
 * rank: it equals nranks exactly when RCCL really connected that many ranks. */
int gp_comm_available(void);
int gp_comm_info(gp_ctx* ctx, int* nranks, int* rank, int64_t* stats_payload_bytes, int64_t* grads_payload_bytes, double* probe_sum);
/* calculate_global_statistics + Kmm parts of calculate_global_derivatives (parallel_GPLVM.py:302-369):
 * Kmm, Cholesky of Kmm and Kmm+beta*Psi2, F, dF_d*, grad_beta.  Asynchronous: the launches are enqueued and nothing is
 * read back; the outcome is reported by the first of gp_global_status / gp_finish / gp_download that follows (one host
 * synchronisation per evaluation). */
int gp_global_step(gp_ctx* ctx);
/* The reference adds 1e-7*I to Kmm (bit 0) and / or Kmm+beta*Psi2 (bit 1) when slogdet reports a negative sign and carries on
 * (partial_terms.logmarglik, partial_terms.py:452-456); if that does not help it asserts (:459-461).  Here a failed Cholesky is
 * reported once as GP_RETRY_JITTER (with the mask to use); the caller repeats the global step -- and phase 2 and its reduction --
 * through this entry.  A second failure of the same matrix is GP_ERR_NOT_PD.  The jittered matrix is used for the log-determinant
 * AND the inverse (the reference keeps the un-jittered LU inverse of the indefinite matrix for the traces and gradients). */
int gp_global_step_jitter(gp_ctx* ctx, int jitter_mask);
/* synchronise and report the outcome of the last global step: GP_OK, GP_RETRY_JITTER (*retry_mask = mask to pass on),
 * GP_ERR_NOT_PD, GP_ERR_NON_FINITE.  retry_mask may be NULL. */
int gp_global_status(gp_ctx* ctx, int* retry_mask);
/* embeddings_mapper body + data-dependent sums of the Z/alpha gradients
 * (local_MapReduce.py:348-358; partial_terms.py:162-205, 256-284, 367-431) */
int gp_phase2(gp_ctx* ctx, int want_embedding_grads);
/* packed device buffer of the phase-2 sums the host all-reduces: grad_Z data part (M*Q) | grad_alpha data part (Q) */
int gp_grads_buffer(gp_ctx* ctx, void** dev_ptr, int64_t* n_doubles);
/* contraction into the final gradients (partial_terms.grad_Z/grad_alpha/grad_sf2/grad_beta,
 * partial_terms.py:207-240, 286-299, 322-333, 340-360).  Any output pointer may be NULL. */
int gp_finish(gp_ctx* ctx, double* F, double* grad_Z, double* grad_sf2, double* grad_alpha, double* grad_beta);

/* ---- prediction ------------------------------------------------------------------------------- */
/* posterior predictive at n new inputs, after a successful global step on this context (the reduced statistics of the whole model; also after
 * gp_set_local_statistics or gp_buffer_combine).  With W = beta (Kmm + beta Psi2)^-1 Psi1^T Y and B = Kmm^-1 - (Kmm + beta Psi2)^-1:
 * X_S == NULL (deterministic inputs): mean = psi1(x)^T W, var = sf2 - psi1(x)^T B psi1(x) (one value per point);
 * X_S != NULL (x ~ N(X_mu, diag X_S)): mean_d = psi1^T W_d, var_d = sf2 - tr(B psi2) + W_d^T psi2 W_d - mean_d^2.
 * X_mu (n,Q); X_S (n,Q) or NULL (xs_is_raw as gp_upload_shard); flags bit 0: add 1/beta (predict y, not f).
 * mean (n,D) or NULL; var (n,D) when X_S != NULL, (n) when X_S == NULL, or NULL.  Synchronous.  Leaves the evaluation state untouched:
 * phase 2 / gp_finish after it give bit-identical results.  GP_ERR_STATE before a global step, after one that failed or asked for a jitter
 * retry, and when the statistics or globals changed since the last global step (gp_phase1, gp_set_globals, gp_set_local_statistics,
 * gp_buffer_combine / gp_scale_buffer of the statistics, gp_stats_unpack, gp_allreduce(ctx, 0), uploads, gp_cg_update moving the embeddings);
 * GP_ERR_BAD_ARG for n < 0 or a non-finite mean / negative or non-finite variance; n = 0 writes nothing. */
int gp_predict(gp_ctx* ctx, int64_t n, const double* X_mu, const double* X_S, int xs_is_raw, int flags, double* mean, double* var);

/* Held-out scoring: how well the model predicts given outputs Y (n,D) at the inputs of gp_predict, reduced on the device to one value per row and
 * five sums per output column (csrc/score.hip).  With m_id and v_id gp_predict's mean and variance at the same inputs and flags
 * bit 0 (v_id: one value per row for X_S == NULL, one per entry otherwise; bit 0 adds 1/beta exactly as in gp_predict) and e = y_id - m_id, for every
 * OBSERVED entry:
 *   logp_id     = -1/2 ln(2 pi v_id) - e^2 / (2 v_id)      computed as e2 = e e, q = e2 / v, logp = -1/2 (ln(2 pi v) + q), each operation rounded once
 *   row_logp[i] = sum_d logp_id     row_sse[i] = sum_d e^2     row_chi2[i] = sum_d e^2 / v_id                                          (n) each
 *   cols[d]     = [count_d, sum_i e, sum_i e^2, sum_i e^2 / v_id, sum_i logp_id]                                                       (D,5)
 * With uncertain inputs this is the density of the MOMENT-MATCHED Gaussian N(m_id, v_id), not of the (non-Gaussian) predictive distribution itself.
 * observed (n,D) row-major, non-zero = observed, NULL = every entry: an entry of Y with observed == 0 is never read, on the host or on the device,
 * and may hold NaN; a row with no observed entry is allowed and scores 0.  Any output pointer may be NULL; a subset gives the bits of the full call.
 * Resident rows: X_mu == NULL scores the context's own rows, as gp_kmeans_accumulate does with X == NULL: n must equal N_s, the inputs are the
 * resident base means (GP_ARR_X_MU), deterministic unless flags bit 1 is set, which takes the resident base variances as well (in the form they were
 * uploaded in); X_S must then be NULL and xs_is_raw 0 either way.  Y == NULL then means the resident Y; a host Y (N_s,D) is allowed too.  Nothing of
 * size n x D crosses the bus in either direction (an optional mask apart).  GP_ERR_STATE when no shard has been uploaded (an engine built from
 * gp_set_local_statistics alone); flags bit 1 with a non-NULL X_mu is GP_ERR_BAD_ARG.
 * Everything else is word for word gp_predict's contract: GP_ERR_STATE unless the last global step succeeded on the statistics and globals as they
 * are now; synchronous; the evaluation state is left untouched, so gp_phase2 / gp_finish / gp_predict* after it give bit-identical results.  n = 0
 * (host inputs; for the resident rows n = N_s holds first) writes zeros to cols and nothing else.  GP_ERR_BAD_ARG, decided before anything is launched: n < 0, unknown flags, a NULL Y with host inputs and
 * n > 0, a non-finite observed entry of Y, non-finite X_mu, X_S that is not finite and >= 0 (as gp_predict), resident rows with n != N_s.
 * A scored entry whose v_id is not > 0 -- var_f at a training input of a nearly noise-free model can round to zero or below, and 1/beta is then
 * too small to lift it -- gives GP_ERR_NON_FINITE when the call returns: the message names the first such row, that row's three outputs and all
 * five sums of the columns it is scored in are NaN, every other row's outputs are valid (a device flag written by plain stores: no second pass).
 * The mean and the variance a row is scored on are gp_predict's bits for that row in a call of the same rows: the same kernels on the same buffers in
 * the same chunks (rows per chunk: 64 MB / (8 (Dp + 2 Mp)) rounded down to a multiple of 128, at least 128 and at most 16384), so logp formed on the
 * host from gp_predict's output differs only by the rounding of the division, the logarithm and the sums.  Bit-identical from run to run, no
 * floating-point atomics.
 * Row invariance, and its limit.  Keeping gp_predict's bits means keeping gp_predict's choice of matrix-product kernel, which depends on the size of
 * the launch: a chunk of r rows (rounded up to 128) forms the mean with (r / 128)(Dp / 128) tiles and, for deterministic inputs, the variance's
 * factors with (r / 128)(2 Mp / 128) tiles; a product of at most 256 tiles runs on the 32 x 32-tile kernel, a larger one on the 128 x 128-tile kernel,
 * and the two add over the inducing points in different orders.  A row's three outputs are therefore the same bits -- alone, in any batch, in any
 * row order, on either side of a chunk boundary -- in any two calls that put each of the row's products on the same kernel: always when every
 * chunk has at most 256 * 128 * 128 / max(Dp, 2 Mp) rows (deterministic; Dp alone for uncertain inputs; 4096 rows at M = 512), and among chunks
 * beyond that.  Between a small and a large chunk the row's mean and variance agree to the rounding of the products (gp_predict's accuracy), not bit
 * for bit -- for instance a row alone against the same row in a full chunk of 7168 rows at M = 512, or a short last chunk.  A batch-independent row,
 * which the other prediction entries obtain by fixing the kernel, and gp_predict's bits cannot both be had; this entry keeps gp_predict's bits.
 * Summation order (csrc/score_pass.h, one definition for this entry and gp_loo_score).  Rows: a function of D alone -- lane l of a 64-lane wave adds the observed d = l, l + 64, .. in ascending order,
 * then the lanes are added pairwise at distance 32, 16, .. 1.  Columns: the ORDER is a function of the global row index alone and never of the chunk
 * size -- the rows are cut into segments of 128 (a chunk is a whole number of them); inside a segment the rows 0 .. 63 and 64 .. 127 are each added
 * in ascending order and the two halves are added; the segments are then added one by one, in ascending order, into the running total, which starts
 * at zero.  cols is thus the same bits at every chunk size under which the rows' terms are (the rule above).  Not covered: non-Gaussian or quadrature densities for uncertain inputs, scores of joint (n x n)
 * predictions, results kept on the device. */
int gp_predict_score(gp_ctx* ctx, int64_t n, const double* X_mu, const double* X_S, int xs_is_raw, const double* Y /*(n,D)*/,
                     const uint8_t* observed /*(n,D) or NULL = all*/, int flags, double* row_logp /*(n)*/, double* row_sse /*(n)*/,
                     double* row_chi2 /*(n)*/, double* cols /*(D,5)*/);

/* Exact leave-one-out and leave-block-out cross-validation of the context's resident rows (X_mu and Y as uploaded, n = N_s), reduced on the device as
 * gp_predict_score reduces (csrc/loo.hip).  Fixed embeddings and fixed Z, sf2, alpha, beta: with k_i = psi1(x_i), a_i = Lk^-1 k_i,
 * b_i = La^-1 k_i, m_i = k_i^T W and e_i = y_i - m_i as in gp_predict_joint, row i contributes beta k_i k_i^T to A = Kmm + beta Psi2 and k_i y_i^T to
 * Psi1^T Y, so Titsias' optimal q(u) of "all data minus the rows of block G" is a rank-g downdate.  Rows [j block, (j + 1) block) form block j (the last
 * one may be short), 1 <= block <= 128.  With B_G (g,M) the block's rows b_i, H = beta B_G B_G^T and S = I - H:
 *   E'_G  = S^-1 E_G                                      (g,D) y minus the mean of the model that never saw G
 *   v'_i  = sf2 - |a_i|^2 + ([S^-1]_ii - 1) / beta        the variance of f at x_i under that model; flags bit 0 adds 1/beta          var_loo (N_s)
 *   lev_i = H_ii = beta |b_i|^2                           the leverage of row i                                                       lev (N_s)
 * (block = 1: e' = e / (1 - h), v' = sf2 - |a|^2 + |b|^2 / (1 - h), h = lev).  A jitter the global step added is part of A and Kmm: the identities
 * hold for the model as factored.  Every OBSERVED entry (i,d) is scored under its own marginal Gaussian N(., v'_i) exactly as gp_predict_score scores:
 * logp = -1/2 (ln(2 pi v') + e'^2 / v'), each operation rounded once; row_logp, row_sse, row_chi2 (N_s) and cols (D,5) = [count, sum e', sum e'^2,
 * sum e'^2 / v', sum logp] are gp_predict_score's.  This is the marginal density per entry, not the joint density of a block.
 * observed (N_s,D) or NULL selects the entries that are summed; it is never an input to H (the model was trained on every entry).  A row with no
 * observed entry scores 0.  Any output pointer may be NULL; a subset gives the bits of the full call.  Nothing of size N_s x D crosses the bus apart
 * from the mask.
 * THE STATISTICS MUST CONTAIN THESE ROWS.  The library cannot tell whether they do: statistics set from elsewhere (gp_set_local_statistics) or a
 * reduce that left this shard out make the downdate meaningless.  That is the caller's obligation.
 * State rule, gp_predict_score's word for word: GP_ERR_STATE unless the last global step succeeded on the statistics and globals as they are now;
 * synchronous; the evaluation state is left untouched, so gp_phase2 / gp_finish / gp_predict* after it give bit-identical results.  In addition
 * GP_ERR_STATE when no shard is uploaded, GP_ERR_UNSUPPORTED when the shard is not in the fixed-embedding regime (a row whose q(x) has non-zero
 * variance contributes a full-rank psi2: the downdate is not rank one), GP_ERR_BAD_ARG, before anything is launched, for block outside 1 .. 128 or
 * unknown flags.
 * A block whose S does not factorise (the model without it is not proper: GP_ERR_NOT_PD) or a row with v' not > 0 (GP_ERR_NON_FINITE): the message
 * names the first such row, its outputs (lev excepted, which stays valid) and the column sums it enters are NaN, every other row is valid; device
 * flags written by plain stores, no second pass.  Blocks of at most 64 rows are factorised several at a time (128 / block whole blocks per 128 x 128
 * tile, by global row index): a block that fails takes the other blocks of its tile with it.
 * Determinism: bit-identical from run to run, no floating-point atomics; a row's outputs and cols are the same bits whatever the chunk length (chunks
 * hold whole tiles; the matrix products run on the 128 x 128-tile kernel whatever the chunk's size).  cols adds in gp_predict_score's order: segments
 * of 128 rows by global row index, ascending.
 * Not covered: uncertain inputs / free embeddings; blocks of more than 128 rows or non-contiguous blocks (order the rows before the upload); joint
 * block densities; per-entry residuals returned to the host; re-optimising the hyper-parameters per fold. */
int gp_loo_score(gp_ctx* ctx, int block, const uint8_t* observed /*(N_s,D) or NULL = all*/, int flags, double* row_logp /*(N_s)*/,
                 double* row_sse /*(N_s)*/, double* row_chi2 /*(N_s)*/, double* lev /*(N_s)*/, double* var_loo /*(N_s)*/, double* cols /*(D,5)*/);

/* Joint posterior at n new deterministic inputs X (n,Q), after a successful global step as gp_predict.  With k_i = psi1(x_i), a_i = Lk^-1 k_i and
 * b_i = La^-1 k_i (Lk, La the Cholesky factors of Kmm and Kmm + beta Psi2):
 *   mean[i][d] = k_i^T W_d (as gp_predict),   cov[i][j] = k(x_i, x_j) - a_i . a_j + b_i . b_j   (one n x n matrix, shared by all D outputs),
 * the inverse-factor form of gp_predict's variance: diag(cov) is that variance.  flags bit 0 adds 1/beta to the diagonal (y, not f).
 * gp_predict_joint: mean (n,D) or NULL, cov (n,n) row-major or NULL; cov[i][j] and cov[j][i] carry the same bits.  n <= 16384.
 * gp_predict_sample: out[s][i][d] = mean[i][d] + sum_j Lc[i][j] eps[s][j][d] for s < n_draws, where Lc Lc^T = cov + (noise + jitter sf2) I, Lc lower
 * with a positive diagonal (noise = 1/beta with flags bit 0, else 0; jitter >= 0 is relative to sf2).  eps (n_draws,n,D): standard normals from the
 * caller (there is no device generator); out (n_draws,n,D); mean (n,D) or NULL.  n <= 8192.  GP_ERR_NOT_PD when the factorisation fails (raise jitter).
 * Both: preconditions, state rule and argument errors are gp_predict's (GP_ERR_STATE unless the last global step succeeded on the statistics and
 * globals as they are now; GP_ERR_BAD_ARG for n < 0, unknown flags, non-finite X or eps, jitter < 0 or non-finite, n_draws < 0, NULL eps / out with
 * n_draws > 0); GP_ERR_UNSUPPORTED beyond the limits on n; n = 0 or n_draws = 0 writes nothing.  Synchronous, bit-identical from run to run (fixed
 * summation order, no floating-point atomics).  The evaluation state is left untouched: gp_phase2 / gp_finish / gp_predict after them give
 * bit-identical results. */
int gp_predict_joint(gp_ctx* ctx, int64_t n, const double* X, int flags, double* mean, double* cov);
int gp_predict_sample(gp_ctx* ctx, int64_t n, const double* X, int flags, double jitter, int n_draws, const double* eps, double* out, double* mean);

/* Derivatives of the prediction with respect to the input, at n new deterministic inputs X (n,Q), after a successful global step as gp_predict.
 * With k = psi1(x), a = Lk^-1 k, b = La^-1 k as above, dk_q = d k / d x_q = -alpha_q (x_q - z_q) o k (difference first, on the centred coordinates),
 * a'_q = Lk^-1 dk_q and b'_q = La^-1 dk_q:
 *   jac[i][d][q]    = dk_q^T W_d                                         (n,D,Q)   d mean_d / d x_q
 *   dvar[i][q]      = -2 (a . a'_q - b . b'_q)                           (n,Q)     d var_f / d x_q
 *   metric[i][q][r] = sum_d jac_dq jac_dr + D (sf2 alpha_q [q == r] - a'_q . a'_r + b'_q . b'_r)   (n,Q,Q)
 *   logdet[i]       = ln det metric[i]                                   (n)       the magnification factor is exp(logdet / 2)
 * metric is the expected metric tensor E[J^T J] = E[J]^T E[J] + D Cov(J) of the mapping x -> f(x); Cov(J) is the mixed second derivative of
 * gp_predict_joint's cov at x = x'.  The noise enters none of them: flags is reserved and must be 0.  Any output may be NULL; a subset gives the bits
 * of the full call.  metric[i] is symmetric bit for bit.  A point's outputs are the same bits alone and in any batch.  jac, dvar and metric work
 * for any Q; logdet is computed on the device for Q <= 64 (beyond: GP_ERR_UNSUPPORTED when logdet is not NULL -- take slogdet of the metric).
 * GP_ERR_NOT_PD when a point's metric does not factorise (not expected for finite inputs; the message names the first such point, its logdet is
 * NaN, every other output of the call is valid).  Preconditions, state rule and argument errors are gp_predict_joint's (GP_ERR_STATE unless the last
 * global step succeeded on the statistics and globals as they are now; GP_ERR_BAD_ARG for n < 0, flags != 0, non-finite X); n = 0 writes nothing.
 * Synchronous, bit-identical from run to run (fixed summation order, no floating-point atomics).  The evaluation state is left untouched: gp_phase2 /
 * gp_finish / gp_predict / gp_predict_joint after it give bit-identical results.  Not covered: uncertain inputs, second derivatives. */
int gp_predict_grad(gp_ctx* ctx, int64_t n, const double* X, int flags, double* jac, double* dvar, double* metric, double* logdet);

/* Expected energy of discrete curves through latent space under the posterior of f, its per-segment terms and its gradient with respect to the
 * curve's points, at deterministic inputs, after a successful global step as gp_predict (csrc/curve.hip).  X (n_curves,T,Q):
 * n_curves curves of T >= 2 points x_0 .. x_{T-1} each.  With k_s = psi1(x_s), dk_s = k_{s+1} - k_s, dx_s = x_{s+1} - x_s, kappa_s = k(x_s, x_{s+1}),
 * [dmu_s | da_s | db_s] = [dk_s^T W | Lk^-1 dk_s | La^-1 dk_s] and the D outputs independent with gp_predict_joint's covariance:
 *   seg[c][s]     = E|f(x_{s+1}) - f(x_s)|^2 = |dmu_s|^2 + D (|db_s|^2 - |da_s|^2) + 2 D (sf2 - kappa_s)            (n_curves,T-1)
 *   energy[c]     = 1/2 (T - 1) sum_s seg[c][s], s ascending  (1/2 int |c'|^2 dt on [0,1] with step 1/(T-1))            (n_curves)
 *   grad[c][t][q] = d energy[c] / d x_tq = (T - 1) [(g_{t-1} - g_t) . dk_t,q + D alpha_q (kappa_{t-1} dx_{t-1,q} - kappa_t dx_{t,q})]   (n_curves,T,Q)
 * with g_s = W dmu_s - D (Lk^-T da_s - La^-T db_s), g_{-1} = g_{T-1} = 0, and dk_t,q = -alpha_q (x_tq - z_q) o k_t as in gp_predict_grad.  The
 * expected length of a curve is sum_s sqrt(max(seg[c][s], 0)).  dk_s and sf2 - kappa_s are formed through expm1 of the exponents' difference, never
 * as a difference of two exponentials, and dx_s from the inputs as given: a curve of any fineness keeps its digits and a repeated point gives
 * seg = 0 exactly.  The noise enters nowhere: flags is reserved and must be 0.  Any output may be NULL; a subset gives the bits of the full call.
 * A curve's outputs are the same bits alone, in any batch, in any curve order and wherever a chunk boundary falls; bit-identical from run to run
 * (fixed summation order that depends on M, Q, D and T alone, no floating-point atomics).  Chunks hold whole curves, max(1, R / T) of them with R
 * the points of gp_predict's chunk (64 MB / (8 (Dp + 2 Mp)) rounded down to a multiple of 128, at least 128 and at most 16384; Mp, Dp = M, D rounded
 * up to 128): GP_ERR_UNSUPPORTED for T > R (M = 512, D = 100: T <= 7168) -- split the curve.  Preconditions, state rule and argument errors are
 * gp_predict_grad's: GP_ERR_STATE unless the last global step succeeded on the statistics and globals as they are now; GP_ERR_BAD_ARG, decided before
 * anything is launched, for n_curves < 0, T < 2, flags != 0, a NULL X with n_curves > 0 or a non-finite X; n_curves = 0 writes nothing.  Synchronous.
 * The evaluation state is left untouched: gp_phase2 / gp_finish / gp_predict* after it give bit-identical results.  Not covered: uncertain inputs,
 * second derivatives, an optimiser on the device (the geodesic solve is host-side: gparml_amd.predict.Predictor.geodesic). */
int gp_curve_energy(gp_ctx* ctx, int64_t n_curves, int T, const double* X /*(n_curves,T,Q)*/, int flags, double* energy /*(n_curves)*/,
                    double* seg /*(n_curves,T-1)*/, double* grad /*(n_curves,T,Q)*/);

/* Pathwise posterior function draws: n_draws sampled functions that can be evaluated at any number of new deterministic inputs, in any number of
 * calls, each call evaluating the SAME functions (Matheron's rule on a random Fourier prior; csrc/paths.hip).  The work of an
 * evaluation is linear in n, O(n (F + M) n_draws D); no n x n matrix is formed and n has no limit.
 * The ARD-RBF prior in F frequency pairs: with frequencies omega (F,Q) and a centre (Q; NULL = 0) the phase of x is
 *   theta_f(x) = sum_q omega[f][q] (x_q - centre_q)       (difference first, q ascending, one fused multiply-add per term)
 * and the 2F features are phi(x) = sqrt(sf2 / F) [cos theta_0 .. cos theta_{F-1}, sin theta_0 .. sin theta_{F-1}].  The caller draws
 * omega[f][q] ~ N(0, alpha_q); phi(x) . phi(x') is then an unbiased estimate of k(x, x') whose diagonal is exactly sf2.  With a = Lk^-1 k(x),
 * b = La^-1 k(x) as above and Phi_Z (M,2F) the features of the inducing points,
 *   G_s = Lk^-1 Phi_Z w_s                                   (M,D) once per draw, in gp_paths_set
 *   out[s][i][d] = mean[i][d] + phi(x_i) . w_s[:,d] - a_i . G_s[:,d] + b_i . eps_u[s][:,d]
 * w (n_draws,2F,D) and eps_u (n_draws,M,D): standard normals from the caller (there is no device generator).  With an exact prior the draws have
 * gp_predict_joint's mean and cov (f, not y: the noise enters nowhere); with F pairs the implied covariance differs from it by exactly
 * P (K_F - K) P^T, K_F = phi phi^T on (X, Z) jointly, P = [I, -k(X,Z) Kmm^-1]: every element of K_F - K has a standard deviation <= sf2 / sqrt(2F).
 * The coordinates enter through the library's centred frame: x - shift and centre - shift, each rounded once, then their difference.
 * gp_paths_set: builds the context's plan of the draws (replacing an earlier one): omega, the centre and the packed operand [Wt ; -G ; E] of
 * (2F rounded up to 16) + 2 Mp rows and n_draws D (rounded up to 128) columns of doubles, Mp = M rounded up to 128.  GP_ERR_UNSUPPORTED when that
 * operand would exceed 2 GiB (set fewer draws at a time).  Needs gp_predict's preconditions.
 * gp_paths_eval: X (n,Q); out (n_draws,n,D); mean (n,D) or NULL: gp_predict's mean.  flags is reserved and must be 0.  GP_ERR_STATE without a plan,
 * and after anything that makes gp_predict return GP_ERR_STATE (new globals, new statistics, a phase 1, a global step): that event also drops the
 * plan -- the draws belonged to the model of the global step gp_paths_set saw.  gp_paths_clear drops the plan and frees its memory.
 * A context holds ONE plan: gp_paths_set frees the earlier one before it builds the new one, so a call that fails part way leaves none.  A plan
 * that such an event has made stale keeps its device memory (up to 2 GiB) until the next gp_paths_eval, gp_paths_set or gp_paths_clear (or
 * gp_destroy): a caller that is done with its draws calls gp_paths_clear.
 * GP_ERR_BAD_ARG, decided before anything is launched: n < 0, n_draws < 1, F < 1, flags != 0, a NULL omega, w, eps_u, or X / out with n > 0,
 * non-finite omega, centre, w, eps_u or X.  n = 0 writes nothing.  All synchronous.  The evaluation state is left untouched: gp_phase2 / gp_finish /
 * gp_predict / gp_predict_joint after them give bit-identical results.
 * Determinism: results are bit-identical from run to run, and a point's outputs depend on that point, the plan and the model only -- the same bits
 * alone, in any batch, in any row order and wherever a chunk boundary falls, so one draw evaluated on two grids agrees exactly at shared points
 * (every matrix product of this path runs on one fixed GEMM kernel without split-k, whatever the launch size; fixed summation order, no
 * floating-point atomics).  Rows are taken in chunks of about 64 MB of left operand [phi | a | b].
 * Not covered: uncertain inputs, noise draws, results kept on the device. */
int gp_paths_set(gp_ctx* ctx, int n_draws, int F, const double* omega /*(F,Q)*/, const double* centre /*(Q) or NULL = 0*/,
                 const double* w /*(n_draws,2F,D)*/, const double* eps_u /*(n_draws,M,D)*/);
int gp_paths_eval(gp_ctx* ctx, int64_t n, const double* X /*(n,Q)*/, int flags, double* out /*(n_draws,n,D)*/, double* mean /*(n,D) or NULL*/);
int gp_paths_clear(gp_ctx* ctx);

/* Derivatives of the draws of gp_paths_set with respect to the input (csrc/paths.hip).  With a'_q = Lk^-1 dk_q,
 * b'_q = La^-1 dk_q and the mean's Jacobian of gp_predict_grad,
 *   jac[s][i][d][q] = d out[s][i][d] / d x_q = jac_mean[i][d][q] + dphi_q(x_i) . w_s[:,d] - a'_q(x_i) . G_s[:,d] + b'_q(x_i) . eps_u[s][:,d]
 *   dphi_q(x) = [ -(scale sin theta_f) omega[f][q]  (f < F) ;  (scale cos theta_f) omega[f][q] ],    scale = sqrt(sf2 / F)
 *   grad[s][i][q]      = sum_d weights[..][d] jac[s][i][d][q]        (d ascending; weights (D), or (n_draws,n,D) with GP_PATHS_WEIGHTS_PER_ROW)
 *   metric[s][i][q][r] = sum_d jac[s][i][d][q] jac[s][i][d][r]       (d ascending; written for q <= r and mirrored from the same value)
 *   mean_jac[i][d][q]  = the mean's Jacobian as this path computes it (what every draw's jac is with zero normals, bit for bit)
 * Each output may be NULL; weights is NULL exactly when grad is.  Needs a current plan: GP_ERR_STATE exactly where gp_paths_eval returns it (and the
 * stale plan is dropped).  GP_ERR_BAD_ARG, decided before anything is launched: n < 1, a NULL or non-finite X, a flag bit other than
 * GP_PATHS_WEIGHTS_PER_ROW, all four outputs NULL, grad without weights or weights without grad, non-finite weights.  Synchronous; the evaluation
 * state, the plan and the results of gp_predict / gp_predict_grad / gp_paths_eval are left untouched.  gp_paths_eval's determinism contract holds:
 * a point's outputs depend on the point, the plan, the model and (grad) its weights only -- the same bits alone, in any batch, in any order,
 * wherever a chunk boundary falls and for any subset of requested outputs.  Points are taken in chunks of about 64 MB of left operand, one row per
 * (point, q).  Not covered: uncertain inputs, second derivatives, results kept on the device. */
#define GP_PATHS_WEIGHTS_PER_ROW 1
int gp_paths_grad(gp_ctx* ctx, int64_t n, const double* X /*(n,Q)*/, int flags,
                  const double* weights /* (D), or (n_draws,n,D) with GP_PATHS_WEIGHTS_PER_ROW; NULL iff grad is NULL */,
                  double* jac      /*(n_draws,n,D,Q) or NULL*/,
                  double* grad     /*(n_draws,n,Q)   or NULL*/,
                  double* metric   /*(n_draws,n,Q,Q) or NULL*/,
                  double* mean_jac /*(n,D,Q) or NULL*/);

/* The posterior conditioned on m extra observed rows (Xc, Yc), without a refit: a rank-m update of the model of the last global step, the mirror
 * image of gp_loo_score's downdate (csrc/condition.hip).  Fixed Z, sf2, alpha, beta; the trained model may have fixed or
 * free embeddings, the conditioning rows and the queries have deterministic inputs.  With a = Lk^-1 k(x), b = La^-1 k(x), mean and var as
 * gp_predict has them, B_c (m,M) the rows b of the conditioning inputs and M_c (m,D) their means under the model as it is,
 *   S = I + beta B_c B_c^T = L L^T,   V = L^-1 B_c,   T = L^-1 (Yc - M_c),   u(x) = V b(x)
 *   mean'(x)_d = mean(x)_d + beta u(x) . T[:,d]          var'(x) = var(x) - beta |u(x)|^2   (flags bit 0 adds 1/beta, as gp_predict)
 * which is exactly the prediction of the model whose statistics are Psi2 + K_c^T K_c, Psi1^T Y + K_c^T Yc, sum_YYT + |Yc|^2: what gp_predict
 * returns after a refit on the shard with these rows appended, embeddings fixed.  S >= I always factorises and |S^-1| <= 1: nothing is amplified.
 * gp_condition_set: 1 <= m <= 1024; builds the context's set (replacing an earlier one whole): V and T, (m rounded up to 128) x (Mp + Dp) doubles.
 * One m x m Cholesky factorisation (the global step's own routines) and a few thin products.  GP_ERR_UNSUPPORTED for m > 1024; GP_ERR_NOT_PD only
 * if the factorisation reports failure, which cannot happen in exact arithmetic.  A call that fails part way leaves the context without a set.
 * gp_condition_predict: X (n,Q); mean (n,D), var (n), reduction (n) = var - var' = beta |u|^2 >= 0: any may be NULL, and the others keep the bits of
 * the full call.  The reduction is the difference of the two variances as they are rounded: var - reduction gives the bits of var'.  Variances are
 * returned unclamped, as gp_predict returns them.  Only X goes to the device and mean, var, reduction come back.
 * Preconditions and state rule are gp_predict's: GP_ERR_STATE unless the last global step succeeded on the statistics and globals as they are now.
 * A set made before the statistics or globals changed (new globals, new statistics, a phase 1, a global step) is stale, as a stale draw set of
 * gp_paths_eval is: gp_condition_predict then answers GP_ERR_STATE, and drops the set, until gp_condition_set is called again; it answers
 * GP_ERR_STATE without a set too.  gp_condition_clear frees the set and succeeds without one; gp_destroy frees it.
 * GP_ERR_BAD_ARG, decided before anything is launched: m < 1, a NULL Xc or Yc, non-finite Xc or Yc; n < 0, unknown flags, a NULL X with n > 0,
 * non-finite X.  n = 0 writes nothing.  All synchronous.  The evaluation state is left untouched: gp_phase2 / gp_finish / gp_predict* after any
 * of the three give bit-identical results.
 * Determinism: results are bit-identical from run to run, and a point's outputs depend on that point, the set and the model only -- the same bits
 * alone, in any batch and at every chunk length (every product runs on one fixed GEMM kernel without split-k; fixed summation order, no
 * floating-point atomics).
 * Not covered: uncertain conditioning or query inputs; per-entry masks on Yc; the joint covariance and draws under the conditioning
 * (cov' = cov - beta U U^T); making the conditioning permanent in the statistics; m > 1024. */
int gp_condition_set(gp_ctx* ctx, int64_t m, const double* Xc /*(m,Q)*/, const double* Yc /*(m,D)*/);
int gp_condition_predict(gp_ctx* ctx, int64_t n, const double* X /*(n,Q)*/, int flags, double* mean /*(n,D) or NULL*/, double* var /*(n) or NULL*/,
                         double* reduction /*(n) or NULL: beta |u|^2 = var - var'*/);
int gp_condition_clear(gp_ctx* ctx);

/* ---- latent inference for new rows ---------------------------------------------------------------- */
/* The bound of n NEW rows y (n,D) under q(x) = N(X_mu, diag X_S), with q(u) frozen at the optimum of the trained model (the statistics of the last
 * global step): per row, with O the observed columns (D_o of them), W and B as for gp_predict, v = W_O y_O and G = W_O W_O^T - D_o B,
 *   L = -D_o/2 ln(2 pi / beta) - beta/2 [ |y_O|^2 - 2 psi1^T v + sum(G o psi2) + D_o sf2 ] - 1/2 sum_q (mu_q^2 + S_q - ln S_q - 1)
 *     = -D_o/2 ln(2 pi / beta) - beta/2 sum_{d in O} [(y_d - mean_d)^2 + var_d] - KL,   mean, var = gp_predict at (X_mu, X_S) without the noise flag.
 * cols: int32 list of the observed output columns, strictly increasing, shared by the call (NULL, 0: all D); the other columns of Y are never read.
 * X_S (n,Q) > 0, or its softplus-inverse with xs_is_raw (as gp_upload_shard); grad_S is then the derivative with respect to the raw value.
 * L (n), grad_mu (n,Q), grad_S (n,Q): any may be NULL.  Rows are independent: a row's outputs are bit-identical whatever other rows share the call.
 * Preconditions, state rule and error codes are gp_predict's (GP_ERR_STATE unless the last global step succeeded on the statistics and globals as
 * they are now; GP_ERR_BAD_ARG for n < 0, a bad column list, non-finite inputs in what is read, variances that are not > 0); n = 0 writes
 * nothing.  Synchronous.  Leaves the evaluation state untouched: phase 2 / gp_finish after it give bit-identical results. */
int gp_infer_objective(gp_ctx* ctx, int64_t n, const double* Y, const int32_t* cols, int n_cols, const double* X_mu, const double* X_S, int xs_is_raw,
                       double* L, double* grad_mu, double* grad_S);
/* Maximises that L for every row over (X_mu, softplus-raw X_S), starting at the given values, which are overwritten with the result (X_S in the form
 * it came in).  Per-row scaled conjugate gradients (Moller), entirely on the device.  A row stops when the largest absolute gradient component in the
 * optimised variables is <= gtol (also at the start) or after max_iters iterations; iters (n, or NULL) reports the iterations taken, so
 * iters < max_iters means the gradient criterion.  Only steps that do not lower L are accepted: L (n, or NULL) is gp_infer_objective's value at the
 * returned point, bit for bit, and never below the value at the start.  Restarts are the caller's rows. */
int gp_infer_latent(gp_ctx* ctx, int64_t n, const double* Y, const int32_t* cols, int n_cols, double* X_mu, double* X_S, int xs_is_raw, int max_iters,
                    double gtol, double* L, int32_t* iters);
/* The same two for rows that each observe their OWN columns, in one call.  observed (n,D), row-major: a non-zero entry means Y[i][d] is observed; an
 * entry of Y with observed == 0 is never read and may be NaN.  Each row's L is gp_infer_objective's formula with O that row's own observed set:
 * v = W_O y_O, |y_O|^2 and D_o are per-row values, and G = W_O W_O^T - D_o B is built once per distinct pattern (row of observed) on the device,
 * never per evaluation.  Everything else is word for word the contract of the two entries above: X_S and xs_is_raw, the outputs and which may be
 * NULL, the optimiser (only steps that do not lower L are accepted; L is gp_infer_objective_rows' value at the returned point, bit for bit, and
 * never below the value at the start; iters per row), the state rule (GP_ERR_STATE unless the last global step succeeded on the statistics and
 * globals as they are now), n = 0 writes nothing, synchronous, and the evaluation state is left untouched: phase 2 / gp_finish / gp_predict after
 * it give bit-identical results.  GP_ERR_BAD_ARG, decided before anything is launched, for n < 0, a NULL observed or Y with n > 0, a row with no
 * observed column (the message names the first such row), a non-finite observed entry of Y, non-finite X_mu, variances that are not > 0,
 * max_iters < 0 or a gtol that is not >= 0.
 * Ordering (csrc/infer.hip): the distinct patterns are numbered in order of first occurrence, the rows are processed in the (stable) order of their
 * pattern's number and the results are scattered back to the caller's order.  A chunk is a run of that order of at most R rows (the chunk length
 * of the two entries above at D observed columns) and at most P_cap = max(1, 2 GiB / (Mp^2 * 8 bytes)) distinct patterns (Mp = M rounded up to
 * 128: 1024 patterns at M = 512), a function of M alone and never of the device; a pattern whose rows straddle a chunk boundary is rebuilt in the
 * next chunk.  Rows of one pattern share its G through the cache; a call whose rows all differ reads Mp^2 * 4 bytes of G per row and evaluation.
 * Determinism: a row's outputs depend on that row's y, pattern and start and on the model only, bit for bit -- the same alone, in any batch, in
 * any row order, and wherever a chunk or pattern-table boundary falls (every matrix product of this path runs on one fixed GEMM kernel without
 * split-k, whatever the launch size; fixed summation order, no floating-point atomics).  They agree with the shared-pattern entries to rounding,
 * not bit for bit. */
int gp_infer_objective_rows(gp_ctx* ctx, int64_t n, const double* Y, const uint8_t* observed, const double* X_mu, const double* X_S, int xs_is_raw,
                            double* L, double* grad_mu, double* grad_S);
int gp_infer_latent_rows(gp_ctx* ctx, int64_t n, const double* Y, const uint8_t* observed, double* X_mu, double* X_S, int xs_is_raw, int max_iters,
                         double gtol, double* L, int32_t* iters);

/* ---- initialisation of the inducing points ---------------------------------------------------------- */
/* One Lloyd assignment pass of k-means: the scipy.cluster.vq.vq + update_cluster_means pair inside scipy.cluster.vq.kmeans, which
 * parallel_GPLVM.init_statistics runs on the host over the first shards' embeddings to place Z (parallel_GPLVM.py:179-186).  Every row of X (n,Q)
 * is assigned to the nearest of the K rows of centres (K,Q) in squared Euclidean distance, computed in the direct form sum_q (x_q - z_q)^2, q
 * ascending (never |x|^2 - 2 x.z + |z|^2, whose cancellation decides near-ties); ties go to the lowest index.  K >= 1 is free of the context's M.
 * X == NULL: the context's resident X_mu (n must equal N_s; GP_ERR_STATE before an upload).  Outputs, any may be NULL:
 *   labels (n) the index of the chosen centre; sums (K,Q) per-centre sum of the rows assigned to it; counts (K);
 *   dist2 (2) = [sum d^2, sum d], d the Euclidean distance to the chosen centre (scipy's stopping rule is on the mean of d).
 * The shards' results add: a host (or an all-reduce) sums them over shards and divides (gparml_amd/init.py).  Results are bit-identical from run to
 * run and a row's label never depends on the other rows.  Summation order (csrc/kmeans.hip): rows are taken in chunks, a chunk in segments of 4096
 * rows; lane l of 64 adds its rows l, l + 64, .. of a segment in ascending order, the lanes are added pairwise (distance 32, 16, .. 1), the
 * segments and then the chunks in ascending order.  Synchronous.  Leaves the evaluation state untouched: gp_phase2 / gp_finish / gp_predict after
 * it give bit-identical results.  GP_ERR_BAD_ARG for n < 0, K < 1, NULL centres, non-finite X or centres; n = 0 writes zeros to sums, counts, dist2. */
int gp_kmeans_accumulate(gp_ctx* ctx, int64_t n, const double* X, int K, const double* centres,
                         double* sums, int64_t* counts, double* dist2, int32_t* labels);

/* Greedy conditional-variance selection of the inducing points: the pivoted Cholesky factorisation of K_nn (Burt, Rasmussen and van der Wilk 2019),
 * the kernel-aware alternative to k-means: one deterministic pass of K steps, every selected point a data row, and after every step the Nystrom
 * residual tr(K_nn - K_nm K_mm^-1 K_mn) of the points chosen so far -- the quantity the collapsed bound is penalised by.
 *   k(x, z) = sf2 exp(-1/2 sum_q alpha_q (x_q - z_q)^2), the difference first, q ascending with one fused multiply-add per term, the library's exp.
 *   Start: d_n = sf2.  Step j: the pivot p is the unselected row of largest d, of equal ones the lowest (shard, row); stop before the step when
 *   d_p <= tol sf2 or j = K.  c_n = (k(x_n, x_p) - sum_{i<j} L_ni L_pi) / sqrt(d_p), i ascending from 0 with one fused multiply-add per term;
 *   L_nj = c_n; d_n <- d_n - c_n^2 in one fused multiply-add; p is marked and never chosen again; trace_j = sum max(d_n, 0) over the unselected rows.
 * gp_select_begin builds the context's selection state (an earlier one is freed first): rows X (n,Q) from the host, uploaded in chunks, or
 *   X == NULL: the resident X_mu (n must equal N_s; GP_ERR_STATE before an upload; it must not be replaced before gp_select_end); sf2 and alpha (Q)
 *   are arguments because no gp_set_globals can have happened yet.  The factor L is kept on the device, n K doubles: GP_ERR_UNSUPPORTED, naming the
 *   size, when that exceeds the free bytes gp_memory_info reports -- decided before anything is allocated.
 * gp_select_run, the one-shard path: enqueues up to `steps` steps (never beyond K in total) with the pivot passed from kernel to kernel on the
 *   device -- no host round trip per step; the stopping rule raises a device flag that the later steps respect -- and reads back once.
 *   *n_done steps were made; rows[0 .. n_done) are their pivots, trace[0 .. n_done) the trace after each (both have `steps` entries; trace may be
 *   NULL).  It may be called again and continues.
 * gp_select_candidate: what a shard offers to the others: the local best unselected row, its d, its coordinates x (Q) and its row of the factor
 *   l (steps done so far); x and l may be NULL.  Without an unselected row: *row = -1, *d = -infinity, x and l are not written.
 * gp_select_apply: one step with the pivot (x_p (Q), l_p (steps done so far), d_p) supplied by the caller; own_row >= 0 marks that local row as
 *   selected (-1: the pivot is another shard's).  *trace (may be NULL): the local trace after the step.  It runs the update kernel of
 *   gp_select_run on the same record: the same bits.  The stopping rule is the caller's.
 * gp_select_end frees the state.
 * Determinism: a row's L and d depend on that row and on the pivots' data only -- not on the other rows, on the chunking of host rows or on how
 * the rows are split over shards: the same rows in one context or in several give the same pivots and the same bits of L and d.  Only trace has a
 * summation order (csrc/select.hip): workgroups of 512 rows, each an LDS tree over its 256 pairs of rows; then thread t of 256 adds the
 * workgroups t, t + 256, .. in ascending order and a tree adds the threads.  No floating-point atomics.
 * All five are synchronous at their return and leave the evaluation state untouched: gp_phase2 / gp_finish / gp_predict after them give
 * bit-identical results.  GP_ERR_STATE for run / candidate / apply / end without a begin, and for an apply after K steps; GP_ERR_BAD_ARG for
 * n < 0, K < 1, a tol that is negative or not finite, an sf2 that is not positive and finite, a negative or non-finite alpha, non-finite rows,
 * X == NULL with n != N_s, steps < 0, a d_p that is not positive and finite, an own_row outside -1 .. n - 1.  n = 0 is legal: it finds nothing. */
int gp_select_begin(gp_ctx* ctx, int64_t n, const double* X /* NULL: the resident X_mu, n == N_s */, int K, double sf2, const double* alpha, double tol);
int gp_select_run(gp_ctx* ctx, int steps, int32_t* n_done, int64_t* rows, double* trace);
int gp_select_candidate(gp_ctx* ctx, double* d, int64_t* row, double* x /* (Q) */, double* l /* (steps done) */);
int gp_select_apply(gp_ctx* ctx, const double* x_p, const double* l_p, double d_p, int64_t own_row /* -1: another shard's */, double* trace);
int gp_select_end(gp_ctx* ctx);

/* ---- initialisation of the embeddings --------------------------------------------------------------- */
/* The two device passes of the PCA that turns Y into the starting X_mu: supporting_functions.PCA (supporting_functions.py:102-121) over ALL data
 * (local_MapReduce.py:50-65) in its streaming form -- per shard the column sums and the Gram matrix of the rows shifted by a centre, which add
 * over shards and ranks; the eigen part is the host's (gparml_amd/init.py: pca_axes, pca); then every row is projected on the axes.
 *
 * gp_scatter_accumulate: for the rows y_r (r < n) of width D (the context's D)
 *   sum (D)     sum[d]     = sum_r (y_rd - centre_d)
 *   gram (D,D)  gram[i][j] = sum_r (y_ri - centre_i)(y_rj - centre_j), the full row-major matrix.
 * Y == NULL: the context's resident Y (n must equal N_s; GP_ERR_STATE before an upload); otherwise host rows (n,D), taken in chunks through the
 * library's own buffers.  Either output may be NULL; gram == NULL skips the D^2 work (the sum-only pass with centre 0 finds the true mean), and
 * sum carries the same bits with and without gram.  The centre (D) is subtracted from every element BEFORE the product (never Y^T Y - n c c^T:
 * its cancellation is why there is a centre); padding rows and columns of the resident layout contribute exact zeros.  gram[i][j] and gram[j][i]
 * carry the same bits: one triangle of 128 x 128 tiles is computed (FP64 matrix-core instructions) and mirrored.  Results are bit-identical from
 * run to run, and host rows and resident rows give the same bits.  Summation order (csrc/pca.hip), a function of the row index, n and D alone:
 * the rows are cut into slices of L = max(512, ceil(n / S) rounded up to 64) rows, S = min(512, 64 MB / (T x 128 KB)) with T the number of tile
 * pairs ceil(D / 128) (ceil(D / 128) + 1) / 2; host chunks are multiples of L.  gram: inside a slice the rows go through the 4x4x4 FP64 MFMA in
 * ascending order, four rows per instruction; sum: wave p of four adds the slice's rows p, p + 4, .. in ascending order and the four are added as
 * (0 + 1) + (2 + 3).  Slices, then chunks, are added in ascending order.  No floating-point atomics.
 *
 * gp_project_rows: X[r][q] = sum_d (y_rd - mean_d) P[d][q], d ascending with one fused multiply-add per term; mean (D), P (D,Q_out) row-major
 * (the caller folds 1/std into P), X host (n,Q_out); Q_out >= 1 is free of the context's Q.  A row's output never depends on the other rows: it
 * is bit-identical alone, in a batch and across a chunk boundary.  Y as above.  The resident X_mu is not written (gp_upload_embeddings commits).
 *
 * Both: synchronous; the evaluation state is left untouched (gp_phase2 / gp_finish / gp_predict after them give bit-identical results).
 * GP_ERR_BAD_ARG for n < 0, a NULL centre / mean / P, Q_out < 1, non-finite Y, centre, mean or P, a NULL X with n > 0, and Y == NULL with
 * n != N_s; n = 0 writes zeros to sum and gram, nothing to X. */
int gp_scatter_accumulate(gp_ctx* ctx, int64_t n, const double* Y, const double* centre, double* sum, double* gram);
int gp_project_rows(gp_ctx* ctx, int64_t n, const double* Y, const double* mean, const double* P, int Q_out, double* X);

/* ---- the start of latent inference ------------------------------------------------------------------ */
/* predict.test starts every new point at the trained embedding of the training output nearest to it (predict.py:44-66).  For each of the n rows
 * of Y_test (n,D) this finds, among a set of training rows, the row of least squared Euclidean distance over the observed columns
 * cols[0 .. n_cols) (each in 0 .. D - 1; cols == NULL: all D columns, n_cols is ignored), computed in the direct form
 * sum_j (y[cols[j]] - t[cols[j]])^2, j ascending with one fused multiply-add per term (never |y|^2 - 2 y.t + |t|^2, whose cancellation decides
 * near-ties).  Columns of Y_test outside cols may hold NaN and are never read.  Training rows: Y_train == NULL: the context's resident rows
 * (n_train is ignored; GP_ERR_STATE before an upload) -- the padding of the resident layout never contributes or wins; otherwise host rows
 * (n_train,D), taken in chunks through the library's own buffers.  Outputs, any may be NULL: dist2 (n) the least squared distance; index (n) the
 * row that has it -- of equally near rows the lowest; x_near (n,Q) the base mean X_mu[index] of that row, resident rows only.  No training rows:
 * every index is -1 and every dist2 +inf.  The minimum over shards is the caller's (gparml_amd/init.py: nearest_start, with the reference's cut-off).
 * A row replaces the best one only when strictly nearer, or equally near with a lower index, at every level (csrc/nearest.hip); there are no
 * atomics: results are bit-identical from run to run, between host rows and resident rows, and for every chunking of either side.  A new row's
 * result never depends on the other new rows.  Synchronous.  Leaves the evaluation state untouched: gp_phase2 / gp_finish / gp_predict after it
 * give bit-identical results.  GP_ERR_BAD_ARG for n < 0, n_train < 0, a column outside 0 .. D - 1, n_cols < 1 with a column list, x_near together
 * with host rows, a NULL Y_test with n > 0, and a non-finite Y_train or observed element of Y_test; n = 0 writes nothing. */
int gp_nearest_rows(gp_ctx* ctx, int64_t n_train, const double* Y_train,   /* NULL: the resident rows, n_train ignored */
                    int64_t n, const double* Y_test, const int32_t* cols, int n_cols, /* cols NULL: all D columns */
                    double* dist2, int64_t* index, double* x_near);        /* (n,), (n,), (n,Q) or NULL; x_near needs resident rows */
/* gp_nearest_rows for new rows that each observe their own columns (rows with holes in different places: the start of one gp_infer_latent_rows
 * call).  observed (n,D), nonzero = observed: the squared distance of new row i to a training row is sum over the observed d of row i, d ascending,
 * of (y[i][d] - t[d])^2, in the same direct form with one fused multiply-add per term; an unobserved element of Y_test may hold NaN and is never
 * read, on the host or on the device.  Everything else is gp_nearest_rows' contract: Y_train == NULL: the resident rows (n_train ignored;
 * GP_ERR_STATE before an upload), whose padding never contributes or wins; otherwise host rows (n_train,D) taken in chunks; any output may be
 * NULL; x_near resident rows only; no training rows: every index -1 and every dist2 +inf; of equally near rows the lowest index at every level, no
 * atomics.  Determinism: a new row's result depends on that row, its mask and the training rows only -- it is bit-identical alone, in any batch,
 * in any chunking of either side and between host rows and resident rows; rows that share one pattern get the bits of gp_nearest_rows with cols =
 * that pattern.  Synchronous.  Leaves the evaluation state untouched.  GP_ERR_BAD_ARG as gp_nearest_rows (less the column list), and for a NULL
 * observed with n > 0, a row with no observed column and a non-finite observed element of Y_test; n = 0 writes nothing. */
int gp_nearest_rows_masked(gp_ctx* ctx, int64_t n_train, const double* Y_train,   /* NULL: the resident rows, n_train ignored */
                           int64_t n, const double* Y_test, const uint8_t* observed,   /* (n,D), nonzero = observed */
                           double* dist2, int64_t* index, double* x_near);

/* ---- k nearest rows in latent space -------------------------------------------------------------------- */
/* The neighbours of points in latent space: for each of the n query rows X (n,Q) the k training rows of least weighted squared distance
 * d2(i,t) = sum_q w_q e_q^2, e_q = x_iq - t_q -- the leave-one-out nearest-neighbour figure of a trained embedding, restarts of the latent inference,
 * geodesic graphs, local subsets.  Either side may be the context's resident embedding means: X_train == NULL: the resident X_mu (n_train is
 * ignored); X == NULL: the resident X_mu as queries (n must equal N_s); they are read exactly as gp_kmeans_accumulate reads them with X == NULL,
 * and the same rows passed as host arrays (the download of GP_ARR_X_MU) give the same bits.  Host rows are taken in chunks through the library's
 * own buffers.  weight (Q), finite and >= 0 (NULL: all 1): with the ARD alpha the distance is the kernel's own metric.
 * Distance: the direct form, difference first, q ascending: acc = fma(e, e, acc) without weights; with them p = w_q * e rounded once, then
 * acc = fma(p, e, acc) (never |x|^2 - 2 x.t + |t|^2, whose cancellation decides near-ties).
 * Order: a query's list is the k training rows that are least in the pair (d2, row), compared lexicographically, ascending: an equal distance
 * goes to the lower row index at every level (csrc/knn.hip).  skip (n) or NULL: per query one training row that is left out, -1 = none; bit 0 of
 * flags (both sides resident): every query leaves out its own row.  Outputs dist2 (n,k) and rows (n,k), either may be NULL; where fewer than k
 * rows are available (n_train small, a row left out) the remaining slots hold rows = -1 and dist2 = +inf.  1 <= k <= 32 (beyond:
 * GP_ERR_UNSUPPORTED); any Q.
 * Determinism: a query's outputs depend on that query, the training rows, the weights and its skip entry only: the same bits alone, in any batch,
 * in any query order, wherever a chunk or slice boundary of either side falls, and from run to run; there are no atomics.  Synchronous.  Needs an
 * uploaded shard only when a side is NULL (GP_ERR_STATE before), no global step.  Leaves the evaluation state untouched: gp_phase2 / gp_finish /
 * gp_predict after it give bit-identical results.  GP_ERR_BAD_ARG, decided before anything is launched, for n < 0, n_train < 0, k < 1, unknown
 * flags, bit 0 without both sides NULL or together with skip, a resident query side with n != N_s, a non-finite X or X_train, a weight that is
 * not finite and >= 0, and a skip entry outside [-1, n_train).  n = 0 writes nothing; n_train = 0 writes the padding.  The merge over shards is
 * the caller's (gparml_amd/init.py: knn). */
int gp_knn_rows(gp_ctx* ctx, int64_t n_train, const double* X_train,   /* (n_train,Q); NULL: the resident X_mu, n_train ignored */
                int64_t n, const double* X,                            /* (n,Q); NULL: the resident X_mu as queries, n must equal N_s */
                const double* weight,                                  /* (Q) finite and >= 0; NULL = all 1 */
                int k, const int64_t* skip,                            /* (n) or NULL: per query one training row to leave out, -1 = none */
                int flags,                                             /* bit 0: both sides resident -> every query leaves out its own row */
                double* dist2, int64_t* rows);                         /* (n,k), (n,k) */

/* ---- results ---------------------------------------------------------------------------------- */
int gp_download(gp_ctx* ctx, int which, double* dst, int64_t n_doubles);
/* set the reduced statistics from the host (partial_terms.set_local_statistics, partial_terms.py:54-61) */
int gp_set_local_statistics(gp_ctx* ctx, double sum_YYT, const double* Psi2, const double* C,
                            double sum_exp_K_ii, double KL);
/* device time of the last evaluation in milliseconds (HIP events on ctx's stream, recorded around each stage):
 * out[0]=prep+Psi1 generation, [1]=phase-1 contraction+reduce, [2]=global step, [3]=phase 2, [4]=sum of [0..3],
 * out[5]=psi1_kernel alone, [6]=p1_kernel alone, [7]=p2_kernel alone */
int gp_last_timings(gp_ctx* ctx, double* out8);
/* How many timing events an evaluation records: 2 (default) = around every stage and the dominant kernels (all of gp_last_timings), 1 = only the
 * first and the last one (gp_last_timings fills out[4], the whole evaluation, alone), 0 = none.  Every event is a signal packet the stream waits
 * on (~4-7 us of idle stream each, thirteen per evaluation): nothing at configs[2]'s size, 15 % of an evaluation at configs[1]'s.  An optimiser
 * that does not read the timings switches them off. */
int gp_set_timing(gp_ctx* ctx, int level);
/* The opt-in int8 phase 1 (GPARML_P1_I8=1; csrc/p1i8.hip: Psi2 / Psi1^T Y of partial_terms.py:45-52, 79-80 from exact integer digit products) guards
 * itself: the first int8 evaluation after an upload and every 64th one run both phase-1 paths, compare the statistics on the device and use the
 * float64 ones; the context is taken off the int8 path (until the next upload) when cond_lower_bound * max(rel_psi2, rel_c) exceeds the library's
 * threshold.  state: -1 the path does not apply to this context's shape / regime, 0 not checked yet, 1 accepted, 2 rejected (float64 kernels run);
 * rel_*: relative Frobenius distance of the int8 statistics from the float64 ones at the last check; checks: how many were made. */
int gp_i8_status(gp_ctx* ctx, int* state, double* rel_psi2, double* rel_c, double* cond_lower_bound, int64_t* checks);
/* hipMemGetInfo of ctx's device: bytes free / total right now (the footprint of a shard at BASELINE configs[4]'s per-GPU size is
 * OBSERVED with this; the reference has no counterpart -- its shard lives in the mapper process' numpy arrays,
 * local_MapReduce.py:197-201) */
int gp_memory_info(gp_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);

/* partial_terms.grad_Z (which=0, partial_terms.py:207-240) / grad_alpha (which=1, :286-299) from explicitly given parts --
 * the signature an unmodified parallel_GPLVM.calculate_global_derivatives (:340-351) calls.  Shapes as in the reference:
 * which=0: dKmm_dX (M,Q,M), dC_dX (M,Q,D), dPsi2_dX (M,Q,M) -> out (M,Q); which=1: (Q,M,M), (Q,M,D), (Q,M,M) -> out (Q) */
int gp_grad_from_parts(gp_ctx* ctx, int which, const double* dF_dKmm, const double* dKmm_dX, const double* dF_dC, const double* dC_dX,
                       const double* dF_dPsi2, const double* dPsi2_dX, double* out);

/* ---- resident CG vectors (scg_adapted_local_MapReduce.py:29-243), SURVEY.md section 8(f)-1 ----------------------------
 * grad_latest / grad_new / grad_old / d are (2,N_s,Q) device arrays; gp_phase2(ctx,1) refreshes grad_latest. */
int gp_cg_set_grads(gp_ctx* ctx);                              /* embeddings_set_grads :29-55: new = old = latest, d = -latest */
/* out6 = [mu = new.d (:59-74), kappa = d.d (:76-90), theta = d.(latest-new) (:92-110), |new|^2 (:112-126),
 *         new.old (:128-140; the caller forms Gamma), max|d|] -- local sums, the host all-reduces them across shards */
int gp_cg_dots(gp_ctx* ctx, double* out6);
int gp_cg_max_d(gp_ctx* ctx, double alpha, double* out);       /* max |alpha*d| :142-155 */
/* the gradient-descent optimiser's two reductions on grad_now (= grad_new here): out2 = [sum |grad_now|, max |grad_now|]
 * (gd_local_MapReduce.py:38-61); its updates are gp_cg_update: set_grads -> 5, update_d(gamma) -> 1 with a = -gamma
 * (d = -(grad_now + gamma d), :63-74), update_X -> 2 (:76-94), update_grad_now -> 4 (:96-105) */
int gp_cg_abs(gp_ctx* ctx, double* out2);
/* which: 0 reset_d :160-173 | 1 update_d(a=Gamma) :175-189 | 2 update_X(a=alpha) :191-214 | 3 update_grad_old :216-229 |
 *        4 update_grad_new :231-243 | 5 set_grads */
int gp_cg_update(gp_ctx* ctx, int which, double a);

/* ---- resident L-BFGS history (csrc/lbfgs.hip) -----------------------------------------------------
 * The vector-free L-BFGS of Chen, Wang and Zhou ("Large-scale L-BFGS using MapReduce", NIPS 2014) on the resident vectors: the context keeps
 * the basis b = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g] of 2m + 1 device vectors of 2 N_s Q doubles, laid out like grad_latest.  The two-loop
 * recursion runs on the host on the (2m+1) x (2m+1) Gram matrix b_i . b_j, whose new rows one gp_lbfgs_dots returns; the new direction is one
 * linear combination of the basis (gp_lbfgs_direction).  The trial mechanism is the existing one: the direction array of gp_set_direction,
 * step_size of gp_set_globals, the grad_latest of gp_phase2(ctx, 1), and gp_cg_update(ctx, 2, a) to move the embeddings.  Free embeddings
 * only (the gp_cg_* rule); the evaluation state is never touched.  An EMPTY slot is a zero vector by definition: it is never read, a dot
 * against it is exactly 0.0 and its coefficient is ignored (as is a coefficient of exactly 0.0 on a filled slot).
 *   gp_lbfgs_begin: 1 <= m <= 32; allocates (2m+1) * 16 N_s Q bytes and marks every slot empty and g unset.  A second call clears the
 *     history: with the same m every slot becomes empty, nothing is reallocated and g stays as it is (a restart); with another m the
 *     vectors are replaced and g is unset.
 *   gp_lbfgs_grad: g = grad_latest (the start, and after a restart).
 *   gp_lbfgs_push, one pass: s[slot] = step * direction, y[slot] = grad_latest - g, g = grad_latest; the slot becomes filled (a filled one is
 *     overwritten: the ring is the caller's).  Needs g (gp_lbfgs_grad), a direction and a finite step.  The embeddings do not move.
 *   gp_lbfgs_dots: out (3, 2m+1) = the LOCAL inner products of s[slot], y[slot] and g with every basis vector, in the order above; slot = -1:
 *     the g row only, the other two rows are zeros.  The caller adds shards and ranks.  Each product is summed in an order that depends on
 *     2 N_s Q alone (segments of 8192 elements, their partials added in ascending order): the same bits from run to run, on any device, for
 *     any m.  GP_ERR_STATE for an empty slot, or before g is set.
 *   gp_lbfgs_direction: direction = sum_j coef[j] * b_j, j ascending over the filled slots and g with coef[j] != 0 (the first term a product,
 *     each further one a fused multiply-add); all-zero: zeros.  The direction counts as rewritten, as after gp_cg_update(ctx, 0 / 1 / 5).
 *   gp_lbfgs_end: frees the vectors.
 * GP_ERR_STATE / GP_ERR_BAD_ARG with a gp_last_error text, before anything is launched: no gp_lbfgs_begin, fixed embeddings, no shard data,
 * no grad_latest, slot outside 0 .. m-1 (-1 .. m-1 for the dots), a non-finite step or coefficient. */
int gp_lbfgs_begin(gp_ctx* ctx, int m);
int gp_lbfgs_grad(gp_ctx* ctx);
int gp_lbfgs_push(gp_ctx* ctx, int slot, double step);
int gp_lbfgs_dots(gp_ctx* ctx, int slot, double* out /* (3, 2m+1) */);
int gp_lbfgs_direction(gp_ctx* ctx, const double* coef /* (2m+1) */);
int gp_lbfgs_end(gp_ctx* ctx);

/* ---- explicit q(u) and minibatch training: the whitened uncollapsed bound (gp_svi_*, csrc/svi.hip) -------------------
 * The collapsed bound solves for q(u) in every global step, so every step needs the statistics of all N rows.  These entries hold q(u) as state
 * instead: u = L_k v with L_k L_k^T = K_mm, q(v_d) = N(Mv[:, d], Sv) with one Sv for all D columns, kept in natural parameters
 * Lam = Sv^-1 (M, M) and H = Lam Mv (M, D); the prior is Lam = I, H = 0.  With a = L_k^-1, Psi2w = a Psi2 a^T, Cw = a C, N = N_global and the
 * statistics as the buffer holds them (a batch's statistics scaled by N / |B| with gp_scale_buffer first):
 *   L     = -1/2 N D ln 2pi + 1/2 N D ln beta - 1/2 beta sum_YYT + beta tr(Mv^T Cw) - 1/2 beta tr(Psi2w (D Sv + Mv Mv^T))
 *           - 1/2 beta D (Psi0 - tr Psi2w) - KL - KLu,      KLu = 1/2 D (tr Sv - M + ln|Lam|) + 1/2 tr(Mv^T Mv)
 *   gp_svi_natural_step(rho):  Lam <- (1 - rho) Lam + rho (I + beta Psi2w),  H <- (1 - rho) H + rho beta Cw      (Psi2w symmetrised: Lam stays
 *           exactly symmetric).  rho = 1 on full statistics is Titsias' optimum, where L equals the collapsed F and every gradient the collapsed one.
 *   gp_svi_step: L and its partials with q(v) held fixed, where gp_global_step leaves its own -- with G2 = 1/2 beta D I - 1/2 beta (D Sv + Mv Mv^T),
 *           Gc = beta Mv, R = 2 G2 Psi2w + Gc Cw^T and Phi(R) = R's strictly lower triangle + half its diagonal:
 *           dF/dPsi2 = a^T G2 a, dF/dPsi1tY = a^T Gc, dF/dKmm = -a^T 1/2 (Phi(R) + Phi(R)^T) a, the phase-2 operand, F = L,
 *           grad_beta = 1/2 N D / beta - 1/2 sum_YYT + tr(Mv^T Cw) - 1/2 tr(Psi2w (D Sv + Mv Mv^T)) - 1/2 D (Psi0 - tr Psi2w), grad_sf2 and the
 *           K_mm parts of grad_Z / grad_alpha by the global step's own formulas on these matrices.  GP_ARR_SCALARS' two log-determinants are
 *           ln|K_mm| and ln|K_mm| + ln|Lam|.  gp_phase2 and gp_finish follow unchanged (fixed or free embeddings, either want_embedding_grads).
 *           Asynchronous; the outcome comes through gp_global_status / gp_finish: K_mm not positive definite is GP_RETRY_JITTER with bit 0 (repeat
 *           gp_svi_step with jitter_mask 1), then GP_ERR_NOT_PD; a Lam that does not factorise is GP_ERR_NOT_PD at once (the caller's state: no
 *           jitter is added to it).  jitter_mask: 0 or 1; the mask is kept for the natural steps and the publish that follow.
 *   gp_svi_publish: writes the pseudo-statistics Psi2_eff = L_k (Lam - I) L_k^T / beta and C_eff = L_k H / beta into the statistics buffer (an
 *           injection of statistics, as gp_set_local_statistics is).  K_mm + beta Psi2_eff = L_k Lam L_k^T, so the ordinary gp_global_step that the
 *           caller runs next leaves Inv, Linv and E describing q(u) exactly: gp_predict and every other new-input entry then work on the SVI-trained
 *           model.  The F (and the gradients) of THAT step mean nothing.  Until then the new-input entries refuse (GP_ERR_STATE): gp_svi_step
 *           leaves no model.
 *   gp_svi_begin: q(v) := prior; a second call without gp_svi_end is GP_ERR_STATE.  gp_svi_set: Lam symmetric, both finite, else GP_ERR_BAD_ARG
 *           (not positive definite is reported by the next step).  gp_svi_get: any pointer may be NULL; Mv / Sv factorise Lam (GP_ERR_NOT_PD when that
 *           fails); synchronous.  gp_svi_natural_step and gp_svi_step need statistics and globals (GP_ERR_STATE), rho in (0, 1] (GP_ERR_BAD_ARG).
 *           a, Psi2w and Cw are computed once and kept until an entry point changes the statistics or the globals (writes through the raw pointer of
 *           gp_stats_buffer between a natural step and its gp_svi_step are not seen).  Every gp_svi_* entry before gp_svi_begin: GP_ERR_STATE.
 *           A natural step on a K_mm that does not factorise leaves the state as it is; the gp_svi_step that follows reports K_mm, and the caller
 *           repeats the natural step after the gp_svi_step with jitter_mask 1 (ShardEngine.svi_step does).
 *           gp_svi_end frees the state; the context evaluates as before.  All products are plain float64; results are bit-identical from run to run. */
int gp_svi_begin(gp_ctx* ctx);
int gp_svi_set(gp_ctx* ctx, const double* Lam /* (M, M) */, const double* H /* (M, D) */);
int gp_svi_get(gp_ctx* ctx, double* Lam /* (M, M) */, double* H /* (M, D) */, double* Mv /* (M, D) */, double* Sv /* (M, M) */);
int gp_svi_natural_step(gp_ctx* ctx, double rho);
int gp_svi_step(gp_ctx* ctx, int jitter_mask);
int gp_svi_publish(gp_ctx* ctx);
int gp_svi_end(gp_ctx* ctx);

/* ---- rows of a resident shard into a batch context, and the embeddings back (csrc/gather.hip) ----
 * Minibatch training from the shard that is already on the device: nothing of size n x D crosses the bus.
 *   gp_gather_shard: dst holds exactly what gp_upload_shard(dst, Y[rows], X_mu[rows], X_S[rows], xs_is_raw) would leave, with the arrays and the
 *           xs_is_raw / fixed-embedding flags src was uploaded with or has since moved to (gp_cg_update, gp_upload_embeddings): Y with its zero
 *           padding written, the embeddings copied in their stored form (no softplus round trip), sum_YYT bit-identical to that upload's, the
 *           upload's lifecycle.  n must be dst's N_s; rows (n) host, each in [0, src's N_s), in any order, repeats allowed.  Synchronous.
 *   gp_scatter_embeddings: src's X_mu / X_S rows 0 .. n-1 into dst's rows rows[i]; dst then stands as after gp_upload_embeddings.  n must be
 *           src's N_s; rows strictly ascending in [0, dst's N_s) (no row is written twice).  Both contexts hold data and store their variances
 *           the same way (xs_is_raw, fixed or free).  Y is never written back.  Synchronous.
 *   Both: D and Q must match, M need not; dst and src are two contexts on one device (another device: GP_ERR_UNSUPPORTED).  Bad indices or counts
 *           and NULL arguments are GP_ERR_BAD_ARG, a source without data GP_ERR_STATE; every check comes before anything is launched or any
 *           state changes.  When the streams differ, the read context's stream is finished first and the work runs on the written context's
 *           (as gp_buffer_combine).  The index list goes through a buffer of the written context that is kept and grown: no allocation per call. */
int gp_gather_shard(gp_ctx* dst, const gp_ctx* src, int64_t n, const int64_t* rows);
int gp_scatter_embeddings(gp_ctx* dst, const gp_ctx* src, int64_t n, const int64_t* rows);

/* ---- shard ingest ------------------------------------------------------
 * numpy.genfromtxt(file, delimiter=',') as statistics_mapper / embeddings_mapper call it on every evaluation
 * (local_MapReduce.py:197-199, 325-327): comma-separated floating-point text -> row-major (rows, cols) doubles.
 * Blank lines and '#' comment lines are skipped, empty or unparsable fields become NaN; a ragged file is GP_ERR_BAD_ARG
 * (genfromtxt raises ValueError).  Host only, parsed in parallel (threads <= 0: all cores); the caller parses a shard once
 * and keeps Y resident (gp_upload_shard). */
int gp_csv_shape(const char* path, int64_t* rows, int64_t* cols);
int gp_csv_read(const char* path, double* out, int64_t rows, int64_t cols, int threads);

/* ---- test hooks (used by tests/ only) --------------------------------------------------------- */
/* C = alpha*op(A)op(B) + beta*C through the library's FP64 MFMA GEMM core; A (m,k) or (k,m) if ta,
 * B (k,n) or (n,k) if tb; any sizes (padded internally) */
int gp_debug_gemm(int device, int ta, int tb, int m, int n, int k, double alpha, const double* A, const double* B,
                  double beta, double* C);
/* make gp_buffer_combine take its cross-device path (peer copy through the staging buffer) even on one device */
int gp_debug_force_staging(int on);
/* process-wide switches of the global step's extended-precision pieces (both on by default): "dd_kipsi2" -- K_mm^-1 Psi2 accumulated in
 * double-double (the product whose float64 rounding is grad_Z's whole error at cond ~1e10), "refine_E" -- one refinement
 * step of E with a double-double residual.  bench.py times the global step with and without to print their cost.
 * "poison_alloc" (also GPARML_POISON=1 at load time): every allocation without a documented zero contract is filled with NaN bytes and
 * gp_set_globals refills the per-evaluation buffers with them -- a kernel that reads what this evaluation did not write fails
 * deterministically (tests/test_gpu_poison.py).  "nearest_rows", k: gp_nearest_rows and gp_nearest_rows_masked take their new rows k at a time (rounded up to 16) and host
 * training rows k at a time (rounded up to 256), so that a small call spans chunks; 0 restores the defaults.  "infer_patterns", k: a chunk of
 * gp_infer_objective_rows / gp_infer_latent_rows holds at most k distinct patterns (P_cap = k); 0 restores the default.  "paths_rows", k: gp_paths_eval
 * takes its rows k at a time (any k >= 1: the chunk's buffers are padded to 128 rows, the chunk is not; never more than gp_predict's chunk), so that a
 * small call spans chunks; 0 restores the default.  "select_rows", k: gp_select_begin uploads its host rows k at a time (any k >= 1); 0 restores the
 * default. */
int gp_debug_set_option(const char* name, int value);
/* in-place lower Cholesky + inverse of an SPD (n,n) matrix; logdet out; returns GP_ERR_NOT_PD on failure */
int gp_debug_potrf_inverse(int device, int n, const double* A, double* L, double* Ainv, double* logdet);
/* device-resident timing of the FP64 MFMA GEMM core: `iters` products of the given shape, milliseconds per product (tools/dev_gemm_bench.py) */
int gp_debug_gemm_bench(int device, int ta, int tb, int m, int n, int k, int iters, double* ms_out);
/* raw copy of one of the global step's internal buffers ("Linv", "Inv", "E", "PsiE", "T1", "T2", "dFdK", "Bbar", "Abar", "Bm", "gK", "gs") after a
 * stream synchronisation; n = capacity of out in doubles (tests/devtools/dev_tail_diff.py).  Between gp_select_begin and gp_select_end also
 * "select_L", the written columns of the factor [steps done][n rounded up to 64], and "select_d" [n rounded up to 64] (GP_ERR_STATE outside).
 * "dir": the search direction [2 N_s Q].  Between gp_lbfgs_begin and gp_lbfgs_end also "lbfgs_s<k>", "lbfgs_y<k>" (k = 0 .. m-1, a filled slot)
 * and "lbfgs_g" (once set), [2 N_s Q] each (GP_ERR_STATE outside, or for a vector that holds nothing). */
int gp_debug_peek(gp_ctx* ctx, const char* name, double* out, long n);
/* the rule the internal matrix products are launched under (csrc/gemm.hip, launch_gemm aborts when it fails: the blocked Cholesky's in-place panel solve raced until
 * round 6): does an operand stored as rows x cols doubles with leading dimension ld, starting at element offset x_off of a buffer, share an element with the result
 * m x n, leading dimension ldc, at offset c_off of the SAME buffer?  Host arithmetic only (no device needed); returns 0 or 1. */
int gp_debug_operands_overlap(long x_off, long rows, long cols, long ld, long c_off, long m, long n, long ldc);
/* ONE internal matrix product with every field of its descriptor (csrc/gp_common.h, GemmP) chosen by the caller: C = alpha op(A) op(B) + beta C on
 * windows of parent buffers, batched as inner x outer entries.  la / lb: 1 = the operand is stored [free][k] (k contiguous), 0 = [k][free]; m, n
 * multiples of 128, k of 16.  geom = 15 longs: lda ldb ldc | inner strides sA sB sC | outer strides oA oB oC | element offset of the first window
 * in its parent, A B C | length of each parent in doubles, A B C.  mode = 5 ints: tri (0 all tiles, 1 lower, 2 upper) | klow | mirror | splits | big.
 * A, B, C are whole parents (host); equal pointers share one device buffer.  The split-k workspace (batch * tiles * splits * 128^2 doubles) is the
 * hook's own; the whole C parent is copied back.  GP_ERR_BAD_ARG, without a launch, for unaligned sizes, a window past its parent, a splits that
 * does not divide a tile's k-chunks, mirror with beta != 0, and any C window that shares an element with an operand or another C window. */
int gp_debug_gemm_modes(int device, int la, int lb, int m, int n, int k, int batch_inner, int batch_outer, const long* geom, double alpha,
                        double beta, const int* mode, const double* A, const double* B, double* C);
/* gp_debug_potrf_inverse for `batch` SPD (n,n) matrices at once, as the global step runs it: A, L, Ainv are [batch][n][n], logdet [batch];
 * *fail_mask gets bit b for a batch entry b that is not positive definite (then GP_ERR_NOT_PD is returned; all outputs are still written).
 * with_workspace: hand the factorisation a split-k workspace, which moves X^T X to the 128 x 128-tile kernel for n > 896. */
int gp_debug_potrf_inverse_batched(int device, int n, int batch, int with_workspace, const double* A, double* L, double* Ainv, double* logdet,
                                   int* fail_mask);
/* ONE of the global step's two extended-precision products on the caller's operands, through the step's own dispatch (csrc/linalg.hip, form_G /
 * form_residual).  product: 0 = G = A B, 1 = the residual R = Csub - A B.  form: 0 = what the step chooses for (Mp, Dp) under the current options,
 * 1 = dd-gemm, 2 = dd-residual, 3 = row-residual, 4 = int8; *form_ran gets the form that ran.  dims = 6 ints: M Mp Dp nA nB K.  Forms 0 and 3 take
 * the step's shapes (nA = K = Mp, nB = Mp for G, Dp for the residual; pass nA = nB = K = 0); forms 1, 2, 4 take nA, nB, K as given.  Operands,
 * dense row-major: forms 1, 2 read A [nA][K]; form 4 reads A [K][nA] (out[i][j] = sum_k A[k][i] B[k][j]; the step's A is symmetric); B [K][nB];
 * Csub [nA][nB].  Form 3 ignores A and rebuilds it as the step does from Keep and Psi2 ([Mp][Mp] each): fma(beta, Psi2, Keep) + jitA on the
 * diagonal, leading M x M block; B = E and Csub = C are [Mp][Dp]; rows M .. Mp of the result are zeros.  out = [nA + 2][nB]: the result and two
 * sentinel rows; the device buffer behind it, the digit planes and the column scales start as 0xFF bytes, so the sentinel rows come back as they
 * were.  GP_ERR_BAD_ARG, before any HIP call, for sizes the kernels cannot take (ddacc_block: nA % 8, nB % 64, K % 8; int8: nA % 64, nB % 64, K % 32,
 * K > 2048, ten digit planes beyond the largest workspace a context allocates), a form that does not compute the product, and form 0 where the
 * step would not run these functions (Mp = Dp = 128 with the fused tail; dd_kipsi2 or refine_E switched off). */
int gp_debug_dd_product(int device, int product, int form, const int* dims, double beta, double jitA, const double* A, const double* B,
                        const double* Csub, const double* Keep, const double* Psi2, double* out, int* form_ran);

#ifdef __cplusplus
}
#endif
#endif /* GPARML_HIP_H */
