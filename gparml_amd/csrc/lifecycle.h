// Where a gp_ctx is in its evaluation, and what each thing that happens to it resets ("Lifecycle").
//
//   gp_upload_shard -> gp_set_globals -> gp_phase1 -> [reduce / scale / pack / inject the statistics] -> gp_global_step -> gp_phase2 -> gp_finish
//
// Plain C++17, no HIP: tests/lifecycle_table.cpp drives it alone on the CPU.  Nothing outside this header writes a field.  EVENTS (past tense) are one
// call per thing that happens and do every reset and lift that belongs to it; QUERIES answer what the entry points ask before they act.  The
// entry points keep their own fail(...) texts.  Rules marked "as found" are kept from the time when every entry point reset its own subset of
// ten loose flags: they disagree with their neighbours, are pinned by tests/test_gpu_lifecycle.py, and are listed in DESIGN.md for a later change.
#pragma once

namespace gp {

struct Lifecycle {
  // How far the statistics and the step built on them have come.  Events ASSIGN it (a step on a finished context goes back to STEP), except the
  // lift of statistics that arrive from outside, which only raises NONE to STATS.
  enum Progress { NONE = 0, STATS = 1 /* the statistics buffer holds sums */, STEP = 2 /* a global step on them is enqueued */, PHASE2 = 3 };

  // ---- events ------------------------------------------------------------------------------------------------------------------------
  void data_uploaded() { has_data_ = true; direction_ = false; prep_fixa_ = false; }     // gp_upload_shard, after embeddings_changed()
  // gp_upload_shard, gp_upload_embeddings, gp_cg_update(2): new base means or variances
  void embeddings_changed() { prep_fixa_ = false; start_over(); }
  // gp_set_direction.  As found: a direction starts the evaluation over, dropping it (NULL) does not, although both change the trial point
  void direction_set(bool present) { direction_ = present; psi1_current_ = false; if (present) start_over(); }
  // gp_cg_update(0, 1, 5) rewrites the direction on the device.  As found: nothing is reset (gp_set_direction with the same values resets)
  void direction_rewritten() { direction_ = true; psi1_current_ = false; }
  void origin_moved() { prep_fixa_ = false; }           // gp_set_globals chose a new origin: the centred means are stale
  void globals_set() { has_globals_ = true; start_over(); }
  void prep_ran(bool fixa) { prep_fixa_ = fixa; }       // run_prep_and_generate: the trial point is built (fixa: in the form that outlives the globals)
  void phase1_ran() { ++inputs_; progress_ = STATS; psi1_current_ = true; packed_ = false; model_ = false; }
  // gp_set_local_statistics.  The lift: statistics from outside admit the global step without a phase 1 -- and, as found, gp_phase2 after it
  // on whatever Psi1 the context holds (psi1_is_current() says which; no entry point asks)
  void stats_injected() { ++inputs_; lift(); packed_ = false; model_ = false; }
  void stats_combined() { ++inputs_; lift(); model_ = false; }     // gp_buffer_combine(statistics).  As found: the packed copy stays "current"
  void stats_scaled() { ++inputs_; packed_ = false; model_ = false; }        // gp_scale_buffer(statistics): the padded buffer is the source of truth
  void stats_unpacked() { ++inputs_; model_ = false; }             // gp_stats_unpack.  As found: raised before the refusal of an unpack without a pack
  void stats_packed() { packed_ = true; }
  void step_started() { model_ = false; }
  void step_enqueued() { progress_ = STEP; model_ = true; outcome_pending_ = true; ++steps_; }     // its outcome is still checked (check_global)
  void step_read_back() { outcome_pending_ = false; }
  // gp_svi_step stands where the global step stands: gp_phase2 and gp_finish follow it, its outcome is checked the same way -- but Inv / Linv / E do
  // not describe its q(u), so the model stays down until gp_svi_publish (stats_injected) and an ordinary global step
  void svi_step_enqueued() { progress_ = STEP; model_ = false; outcome_pending_ = true; }
  void phase2_mode(bool embedding_grads) { embedding_mode_ = embedding_grads; }          // the feature layout of the trial point follows it
  void grad_latest_written() { grad_latest_ = true; }   // the resident CG vector; never cleared (as found: it outlives an upload)
  void phase2_ran() { progress_ = PHASE2; }

  // ---- queries -----------------------------------------------------------------------------------------------------------------------
  bool has_data() const { return has_data_; }
  bool has_globals() const { return has_globals_; }
  bool has_direction() const { return direction_; }
  bool embedding_mode() const { return embedding_mode_; }
  bool can_phase1() const { return has_data_ && has_globals_; }
  bool has_stats() const { return progress_ >= STATS; }
  bool step_done() const { return progress_ >= STEP; }
  bool phase2_done() const { return progress_ >= PHASE2; }
  bool psi1_available() const { return has_data_ && has_stats(); }                      // the compat arrays made from Psi1 (as found: has_stats stands for it)
  bool psi1_is_current() const { return psi1_current_; }
  bool step_outcome_pending() const { return outcome_pending_; }
  // Inv / Linv / E describe the statistics and the globals as they are now: gp_predict, gp_infer_*
  bool model_current() const { return step_done() && has_globals_ && model_; }
  // Which global step the model is of: a plan built from Inv / Linv / E (gp_paths_set) keeps the number and is stale once it differs -- model_
  // rises again only through step_enqueued, so "model_current() and the same number" is "nothing has happened to the model since"
  long model_serial() const { return steps_; }
  // Counts everything that changes the statistics buffer or the globals through an entry point: what gp_svi_* derives from both (the whitened
  // statistics) is kept with the number and is stale once it differs
  long inputs_serial() const { return inputs_; }
  bool grad_latest_ready() const { return phase2_done() && embedding_mode_; }           // GP_ARR_GRAD_LATEST, rebuilt from this evaluation's gradients
  bool has_grad_latest() const { return grad_latest_; }                                 // gp_cg_update(4, 5): the resident copy
  bool prep_is_current(bool fixa) const { return fixa && prep_fixa_; }
  bool packed_is_current() const { return packed_; }
  // gp_last_timings: which pairs of events an evaluation has recorded.  As found: the level, so injected statistics report phase 1's events too
  bool phase1_timed() const { return has_stats(); }
  bool step_timed() const { return step_done(); }
  bool phase2_timed() const { return phase2_done(); }

 private:
  // Data, embeddings, direction or globals changed: the statistics, Psi1 and the step are stale.  progress_ carries two meanings that cannot be
  // parted without changing an outcome -- gp_phase2 and the compat downloads are admitted on the level alone, so after injected statistics they
  // run on a Psi1 the level says nothing about.  psi1_current_ is the second meaning on its own, kept for the table and the later change.
  void start_over() { ++inputs_; progress_ = NONE; psi1_current_ = false; model_ = false; }
  void lift() { if (progress_ < STATS) progress_ = STATS; }

  Progress progress_ = NONE;
  bool psi1_current_ = false;     // the trial point and Psi1 in Kaug belong to the data, embeddings, direction and globals as they are now
  bool has_data_ = false, has_globals_ = false;
  bool direction_ = false;        // the dir buffer takes part in the trial point
  bool embedding_mode_ = false;   // the last gp_phase2 asked for embedding gradients
  bool prep_fixa_ = false;        // fixed embeddings: the prep kernels' outputs (mu, features, records) are current
  bool packed_ = false;           // gp_stats_pack has run since the statistics last changed (gp_stats_unpack refuses to run before it)
  bool model_ = false;            // the last global step saw the statistics and globals as they are now
  bool outcome_pending_ = false;  // a global step was enqueued and its scalars / failure flags have not been read back yet
  bool grad_latest_ = false;
  long steps_ = 0;                // global steps enqueued so far (model_serial)
  long inputs_ = 0;               // changes of the statistics or the globals so far (inputs_serial)
};

}  // namespace gp
