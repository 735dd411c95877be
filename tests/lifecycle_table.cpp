// Stand-alone driver of gparml_amd/csrc/lifecycle.h (no HIP, no library): from every point of the canonical evaluation it raises every event on a
// copy of the state and prints every query's answer, one line per (point, event).  tests/test_lifecycle_cpu.py compiles it with the host
// compiler (once more under -fsanitize=address,undefined), runs it and compares the lines with the rules written down from the entry points as
// they were before this header existed.
#include <cstdio>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../gparml_amd/csrc/lifecycle.h"

using gp::Lifecycle;
using Event = std::pair<std::string, std::function<void(Lifecycle&)>>;
using Query = std::pair<std::string, std::function<bool(const Lifecycle&)>>;

#define EV(name, call) Event{name, [](Lifecycle& l) { l.call; }}
#define QU(name, call) Query{name, [](const Lifecycle& l) { return l.call; }}

int main() {
  const std::vector<Event> events = {
      EV("data_uploaded", data_uploaded()), EV("embeddings_changed", embeddings_changed()), EV("direction_set(0)", direction_set(false)),
      EV("direction_set(1)", direction_set(true)), EV("direction_rewritten", direction_rewritten()), EV("origin_moved", origin_moved()),
      EV("globals_set", globals_set()), EV("prep_ran(0)", prep_ran(false)), EV("prep_ran(1)", prep_ran(true)), EV("phase1_ran", phase1_ran()),
      EV("stats_injected", stats_injected()), EV("stats_combined", stats_combined()), EV("stats_scaled", stats_scaled()),
      EV("stats_unpacked", stats_unpacked()), EV("stats_packed", stats_packed()), EV("step_started", step_started()),
      EV("step_enqueued", step_enqueued()), EV("step_read_back", step_read_back()), EV("phase2_mode(0)", phase2_mode(false)),
      EV("phase2_mode(1)", phase2_mode(true)), EV("grad_latest_written", grad_latest_written()), EV("phase2_ran", phase2_ran())};
  const std::vector<Query> queries = {
      QU("has_data", has_data()), QU("has_globals", has_globals()), QU("has_direction", has_direction()), QU("embedding_mode", embedding_mode()),
      QU("can_phase1", can_phase1()), QU("has_stats", has_stats()), QU("step_done", step_done()), QU("phase2_done", phase2_done()),
      QU("psi1_available", psi1_available()), QU("step_outcome_pending", step_outcome_pending()), QU("model_current", model_current()),
      QU("grad_latest_ready", grad_latest_ready()), QU("has_grad_latest", has_grad_latest()), QU("prep_is_current(0)", prep_is_current(false)),
      QU("prep_is_current(1)", prep_is_current(true)), QU("packed_is_current", packed_is_current()), QU("phase1_timed", phase1_timed()),
      QU("step_timed", step_timed()), QU("phase2_timed", phase2_timed()), QU("psi1_is_current", psi1_is_current())};
  // the canonical evaluation: the events each entry point raises, in its order (fixed embeddings in phase 1, embedding gradients in phase 2)
  const std::vector<std::pair<std::string, std::vector<std::string>>> points = {
      {"new", {}},
      {"gp_upload_shard", {"embeddings_changed", "data_uploaded"}},
      {"gp_set_globals", {"origin_moved", "globals_set"}},
      {"gp_phase1", {"prep_ran(1)", "phase1_ran"}},
      {"gp_stats_pack", {"stats_packed"}},
      {"gp_global_step", {"step_started", "step_enqueued"}},
      {"gp_phase2", {"phase2_mode(1)", "prep_ran(0)", "grad_latest_written", "phase2_ran"}},
      {"gp_finish", {"step_read_back"}}};
  auto raise = [&](Lifecycle& l, const std::string& name) {
    for (const Event& e : events)
      if (e.first == name) { e.second(l); return true; }
    return false;
  };
  auto answers = [&](const Lifecycle& l) {
    std::string s;
    for (const Query& q : queries) s += q.second(l) ? '1' : '0';
    return s;
  };
  std::string names = "queries:";
  for (const Query& q : queries) names += " " + q.first;
  std::puts(names.c_str());
  Lifecycle at;
  for (const auto& p : points) {
    for (const std::string& name : p.second)
      if (!raise(at, name)) { std::fprintf(stderr, "unknown event %s\n", name.c_str()); return 2; }
    std::printf("%s | - | %s\n", p.first.c_str(), answers(at).c_str());
    for (const Event& e : events) {
      Lifecycle l = at;
      e.second(l);
      std::printf("%s | %s | %s\n", p.first.c_str(), e.first.c_str(), answers(l).c_str());
    }
  }
  return 0;
}
