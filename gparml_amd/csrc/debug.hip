// The developer hooks that take names (test tools, same-box A/B): the run-time switches and the raw copy of an internal buffer, each one table.
// The harnesses that run file-static code (gp_debug_gemm*, gp_debug_potrf_inverse*, gp_debug_dd_product, gp_debug_operands_overlap) stay in its file.
#include "pred_chunk.h"
#include <cstring>

using namespace gp;

bool gp::g_force_staging = false;
extern "C" int gp_debug_force_staging(int on) { g_force_staging = on != 0; return GP_OK; }

// Every run-time switch by name; each atomic is defined next to the code it switches (gp_common.h declares them).  A flag stores value != 0, a count
// max(0, value) (a chunk length or a countdown, 0 = the default), p2_rem's range clamp(value, 0, 2) (p2_rem.hip: 0 whole tiles only, 1 the rule, 2
// wherever it fits).  The message for an unknown name lists the table; tests/test_gemm_overlap_rule.py pins it name by name.
extern "C" int gp_debug_set_option(const char* name, int value) {
  enum Kind { FLAG, COUNT, RANGE2 };
  static const struct { const char* name; std::atomic<int>* opt; Kind kind; } options[] = {
      {"dd_kipsi2", &g_opt_dd_kipsi2, FLAG},     {"refine_E", &g_opt_refine_E, FLAG},       {"p1_i8", &g_opt_p1_i8, FLAG},
      {"gs_tail", &g_opt_gs_tail, FLAG},         {"i8_guard_strict", &g_opt_i8_guard_strict, FLAG}, {"xtx_tri", &g_opt_xtx_tri, FLAG},
      {"residual_dd", &g_opt_residual_dd, FLAG}, {"gemm_big", &g_opt_gemm_big, FLAG},       {"trtri_rec", &g_opt_trtri_rec, FLAG},
      {"gs_i8", &g_opt_gs_i8, FLAG},             {"poison_alloc", &g_opt_poison, FLAG},     {"predict_rows", &g_opt_pred_rows, COUNT},
      {"infer_rows", &g_opt_inf_rows, COUNT},    {"kmeans_rows", &g_opt_km_rows, COUNT},    {"alloc_fail_after", &g_alloc_fail_after, COUNT},
      {"p2_rem", &g_opt_p2_rem, RANGE2},         {"nearest_rows", &g_opt_nn_rows, COUNT},   {"infer_patterns", &g_opt_inf_patterns, COUNT},
      {"paths_rows", &g_opt_paths_rows, COUNT},  {"curve_curves", &g_opt_curve_curves, COUNT}, {"knn_rows", &g_opt_knn_rows, COUNT},
      {"select_rows", &g_opt_sel_rows, COUNT}};
  if (!name) return fail(nullptr, GP_ERR_BAD_ARG, "gp_debug_set_option: NULL name");
  std::string known;
  for (const auto& o : options) {
    const int stored = o.kind == FLAG ? (value ? 1 : 0) : std::max(0, o.kind == RANGE2 ? std::min(value, 2) : value);
    if (!std::strcmp(name, o.name)) { o.opt->store(stored); return GP_OK; }
    known += (known.empty() ? "" : ", ") + std::string(o.name);
  }
  return fail(nullptr, GP_ERR_BAD_ARG, "gp_debug_set_option: unknown option '%s' (%s)", name, known.c_str());
}

// gp_debug_peek's plain buffers, which every context holds from gp_create on: the name, the buffer, its doubles as it lies in memory (padding included)
#define PEEK_BUF(name, buf, count) {name, [](const gp_ctx* c) -> const double* { return c->buf; }, [](const gp_ctx* c) -> long { return count; }}
static long peek_mm(const gp_ctx* c) { return (long)c->Mp * c->Mp; }
static long peek_md(const gp_ctx* c) { return (long)c->Mp * c->Dp; }
static const struct { const char* name; const double* (*ptr)(const gp_ctx*); long (*count)(const gp_ctx*); } peek_bufs[] = {
    PEEK_BUF("Linv", gstep.Linv, 2 * peek_mm(c)), PEEK_BUF("Inv", gstep.Inv, 2 * peek_mm(c)), PEEK_BUF("E", gstep.E, peek_md(c)),
    PEEK_BUF("PsiE", gstep.PsiE, peek_md(c)), PEEK_BUF("T1", gstep.T1, peek_mm(c)), PEEK_BUF("T2", gstep.T2, peek_mm(c)),
    PEEK_BUF("dFdK", gstep.dFdK, peek_mm(c)), PEEK_BUF("Bbar", gstep.Bbar, peek_mm(c)), PEEK_BUF("Abar", gstep.Abar, peek_md(c)),
    PEEK_BUF("Bm", gstep.Bm, (long)c->LDK * c->Mp), PEEK_BUF("gK", gstep.gK, (long)grads_doubles(c)), PEEK_BUF("gs", gstep.gs, (long)c->gstep.gs.size()),
    PEEK_BUF("Kmm", gstep.Kmm, 2 * peek_mm(c)), PEEK_BUF("KmmKeep", gstep.KmmKeep, peek_mm(c)),
    // the evaluation's other buffers (r06, the poison probe: tests/devtools/dev_poison_probe.py)
    PEEK_BUF("stats", stats, (long)stats_doubles(c)), PEEK_BUF("Kaug", Kaug, (long)c->Np * c->LDK), PEEK_BUF("Z", Z, (long)c->Mp * c->Q),
    PEEK_BUF("Zaug", Zaug, (long)c->Mp * c->CZp), PEEK_BUF("mu", mu, (long)c->Np * c->Q), PEEK_BUF("S", S, (long)c->Np * c->Q),
    PEEK_BUF("Xa", Xa, (long)c->Np * c->CXp), PEEK_BUF("grads", grads, (long)grads_doubles(c)), PEEK_BUF("Rpart", p2.Rpart, (long)c->p2.Rpart.size()),
    PEEK_BUF("dir", dir, 2L * c->N * c->Q)};
#undef PEEK_BUF

// The names a feature or a precondition stands behind, tried in this order ("infer_LEA" before the prefix "infer_").  resolve: the source (NULL:
// nothing to read) and *cnt (-1: no such name); *ints: the source holds ints.  With `refusal`, a NULL source is GP_ERR_STATE "'<name>' <refusal>".
static const void* cg_vector(const gp_ctx* c, const double* v, long* cnt) { *cnt = 2L * c->N * c->Q; return c->life.has_data() && c->xs_raw ? v : nullptr; }
static const void* base_rows(const gp_ctx* c, const double* x, long* cnt) { *cnt = (long)c->N * c->Q; return c->life.has_data() ? x : nullptr; }
static const char kNoCg[] = "exists only with shard data and free embeddings (raw variances)", kNoSelect[] = "outside gp_select_begin .. gp_select_end";
#define PEEK_FN [](const gp_ctx* c, const char* name, long* n, bool*) -> const void*
static const struct { const char* name; bool prefix; const void* (*resolve)(const gp_ctx*, const char*, long*, bool*); const char* refusal; } peek_features[] = {
    {"LE", false, PEEK_FN { return b_debug_table(c, false, n); }, nullptr},
    {"LEA", false, PEEK_FN { return b_debug_table(c, true, n); }, nullptr},
    {"pred_LEA", false, PEEK_FN { return pred_debug_lea(c, n); }, nullptr},
    {"infer_LEA", false, PEEK_FN { return infer_debug_lea(c, n); }, nullptr},
    {"infer_", true, infer_debug_scg, "before gp_infer_latent has built the optimiser's state"},      // the per-row SCG: tests/test_gpu_infer_scg.py
    {"select_L", false, PEEK_FN { return select_debug(c, true, n); }, kNoSelect},
    {"select_d", false, PEEK_FN { return select_debug(c, false, n); }, kNoSelect},
    // the resident CG vectors and the base embeddings as stored (Xs raw when uploaded raw): tests/test_gpu_resident_vectors.py
    {"cg_g_new", false, PEEK_FN { return cg_vector(c, c->cg.g_new, n); }, kNoCg},
    {"cg_g_old", false, PEEK_FN { return cg_vector(c, c->cg.g_old, n); }, kNoCg},
    {"cg_g_latest", false, PEEK_FN { return cg_vector(c, c->cg.g_latest, n); }, kNoCg},
    {"Xmu", false, PEEK_FN { return base_rows(c, c->Xmu, n); }, "before gp_upload_shard"},
    {"Xs", false, PEEK_FN { return base_rows(c, c->Xs, n); }, "before gp_upload_shard"},
    {"lbfgs_", true, PEEK_FN { return lbfgs_debug(c, name, n); }, "outside gp_lbfgs_begin .. gp_lbfgs_end, or not a vector that holds anything"}};
#undef PEEK_FN

// raw copy of an internal buffer (developer and test tool, ShardEngine.peek): out receives the buffer's cnt doubles; GP_ERR_BAD_ARG when n < cnt
extern "C" int gp_debug_peek(gp_ctx* c, const char* name, double* out, long n) {
  if (!c || !name || !out) return GP_ERR_BAD_ARG;
  GP_HIP(c, hipSetDevice(c->device));
  const void* src = nullptr; long cnt = -1; bool ints = false;
  for (const auto& b : peek_bufs) if (!std::strcmp(name, b.name)) { src = b.ptr(c); cnt = b.count(c); break; }
  for (const auto& f : peek_features) {
    if (cnt >= 0 || (f.prefix ? std::strncmp(name, f.name, std::strlen(f.name)) : std::strcmp(name, f.name))) continue;      // a plain buffer; another name
    src = f.resolve(c, name, &cnt, &ints);
    if (!src && cnt >= 0 && f.refusal) return fail(c, GP_ERR_STATE, "gp_debug_peek: '%s' %s", name, f.refusal);
    break;
  }
  if (cnt < 0) return fail(c, GP_ERR_BAD_ARG, "gp_debug_peek: unknown buffer '%s'", name);
  if (n < cnt) return fail(c, GP_ERR_BAD_ARG, "gp_debug_peek: %ld doubles needed", cnt);
  GP_HIP(c, hipStreamSynchronize(c->stream));
  if (ints) {                                  // widened on the host after the copy
    std::vector<int> h((size_t)cnt);
    GP_HIP(c, hipMemcpy(h.data(), src, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost));
    std::copy(h.begin(), h.end(), out);
  } else GP_HIP(c, hipMemcpy(out, src, cnt * 8, hipMemcpyDeviceToHost));
  return GP_OK;
}
