// pba_lm.cpp -- the solve drivers: replaces ceres::Solve at reference src/photobundle.cc:829.
//
// ONE rule set, four schedulers.  The trust-region rules (Ceres TrustRegionMinimizer + LevenbergMarquardtStrategy) are pba_lm_rules.h:
// an LmState and one lm_decide per step on the step's scalar block.  The drivers of this file only differ in WHERE that decision runs
// and how the device work around it is scheduled; all heavy work is behind the engine (pba_engine.hip):
//   host-stepped  solve_host_stepped   one step per round trip, lm_decide on the host.  Everything the others do not cover: wide windows,
//                                      pose-only solves, PBA_FUSE=0 / PBA_ASYNC=0, the precision-sweep flags, profiling, iteration limits
//                                      beyond the device log, the callback transport without peer exchange
//   pipelined     solve_async          lm_decide in the last workgroup of every candidate pass; the host enqueues steps back to back
//   batched       pba_solve_batch      the pipelined schedule for n independent windows in shared launches
//   resident      solve_resident       the whole solve as one cooperative launch, lm_decide in its serial workgroup
// All of them report through summarize_solve, which holds every termination message.
//
// One deviation from Ceres in scheduling (not in results), common to all drivers: the gradient norms of a freshly accepted point come
// out of the same device pass that computes the NEXT trust-region step, so that step is computed speculatively right after an
// acceptance; if the iteration then terminates the solve (gradient tolerance / iteration limit) the speculative step is simply
// dropped (at the iteration limit only the gradient part is run).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pba.h"

#include "pba_internal.h"
#include "pba_device.h"

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}

static int summarize_solve(pba_engine* e, const pba_solver_options* o, const pba::LmState* st, const pba_iteration_summary* device_log,
                           pba_solver_summary* sum, pba_iteration_summary* its, int32_t max_out, double t_start, bool verbose,
                           int64_t jac_passes);
// the state a device driver left in the engine's host mirror
static const pba::LmState* mirror(const pba_engine* e) { return static_cast<const pba::LmState*>(pba_internal_async_state(e)); }

// Resident variant (pba_resident.h): the whole solve is ONE cooperative launch -- every workgroup keeps its tiles' state in registers
// across the iterations, the serial workgroup takes the same decisions (lm_decide) -- and the host only waits for the flush.
static int solve_async(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum, pba_iteration_summary* its,
                       int32_t max_out, double t_start, bool verbose);

static int solve_resident(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum, pba_iteration_summary* its,
                          int32_t max_out, double t_start, bool verbose) {
  unsigned long long seq = 0;
  int rc = pba_internal_resident_launch(e, o, &seq);
  if (rc == PBA_INTERNAL_RESIDENT_REFUSED) return solve_async(e, o, sum, its, max_out, t_start, verbose);
  if (rc) return rc;
  if ((rc = pba_internal_async_wait(e, seq))) { pba_internal_resident_failed(e); return rc; }
  if ((rc = pba_internal_async_end(e))) return rc;
  const pba::LmState* st = mirror(e);
  pba_internal_resident_done(e, st->iteration);
  pba_internal_resident_trace(e, st->iteration);
  // one Jacobian pass at the initial point + one (speculative) Jacobian pass per step taken
  return summarize_solve(e, o, st, pba_internal_async_log(e), sum, its, max_out, t_start, verbose, 1 + (int64_t)st->iteration);
}

// Asynchronous variant: the same trust-region rules are evaluated on the device by the last workgroup of every
// candidate pass (lm_decide), so the host enqueues iterations back to back (at most kAhead in flight
// beyond the last one it has seen finish) instead of paying a launch + completion round trip per step.
static int solve_async(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum, pba_iteration_summary* its,
                       int32_t max_out, double t_start, bool verbose) {
  using pba::LmState;
  constexpr int kAhead = 3;
  static const bool tr = getenv("PBA_TRACE_SOLVE") != nullptr;
  double tt[8] = {0};
  tt[0] = now();
  int rc = pba_internal_async_begin(e, o);
  if (rc) return rc;
  tt[1] = now();
  const volatile LmState* st = static_cast<const volatile LmState*>(pba_internal_async_state(e));
  unsigned long long seq = 0, seqs[kAhead + 1] = {0};
  if ((rc = pba_internal_async_enqueue(e, 0, 0, o, &seq))) return rc;
  tt[2] = now();
  int enq = 0;
  unsigned long long last_seq = 0;
  // Multi-rank: every enqueued step carries collectives, so all ranks must enqueue the SAME number of steps although
  // each sees the termination flag at a different moment: they all stop kAhead steps after the terminating one.
  const bool multi = pba_internal_is_multi(e) != 0;
  while (enq < o->max_num_iterations) {
    // done and done_seq reach the host mirror as independent 32-bit stores: act on `done` in multi-rank mode only once
    // the (non-zero) sequence number of the terminating step is visible too
    {
      const unsigned long long ds = st->done_seq;
      if (st->done && (!multi || (ds != 0 && last_seq >= ds + kAhead))) break;
    }
    if ((rc = pba_internal_async_enqueue(e, 1, enq == 0 ? 1 : 0, o, &seq))) return rc;
    seqs[enq % (kAhead + 1)] = seq;
    last_seq = seq;
    ++enq;
    if (enq > kAhead) { if ((rc = pba_internal_async_wait(e, seqs[(enq - kAhead) % (kAhead + 1)]))) return rc; }
  }
  // Iteration limit (or max_num_iterations <= 0): the gradient norms of the final point may still be missing.  The pass
  // that computes them is enqueued unconditionally and gates itself on the device state (lm_final_pass_needed), which
  // saves a host round trip; then ONE flush brings the last outcome and the iteration log to the host mirror.
  tt[3] = now();
  bool flushed = false;
  if (enq >= o->max_num_iterations) {
    if ((rc = pba_internal_async_enqueue(e, 2, o->max_num_iterations <= 0 ? 1 : 0, o, &seq))) return rc;
    flushed = pba_internal_final_flushes(e) != 0;      // single rank: the final pass flushes in its own last workgroup
  }
  if (!flushed && (rc = pba_internal_async_enqueue(e, 3, 0, o, &seq))) return rc;
  tt[4] = now();
  if ((rc = pba_internal_async_wait(e, seq))) return rc;
  tt[5] = now();
  (void)last_seq;
  if ((rc = pba_internal_async_end(e))) return rc;
  tt[6] = now();
  if (tr) std::fprintf(stderr, "solve_async us: entry->begin %.1f, begin %.1f, enqueue0 %.1f, loop %.1f, final enqueues %.1f, final wait %.1f, end %.1f\n",
                       1e6 * (tt[0] - t_start), 1e6 * (tt[1] - tt[0]), 1e6 * (tt[2] - tt[1]), 1e6 * (tt[3] - tt[2]), 1e6 * (tt[4] - tt[3]), 1e6 * (tt[5] - tt[4]), 1e6 * (tt[6] - tt[5]));
  return summarize_solve(e, o, mirror(e), pba_internal_async_log(e), sum, its, max_out, t_start, verbose, -1);
}

// The final trust-region state and the iteration log -> pba_solver_summary: every driver ends here, and no termination message is
// written anywhere else.  device_log: the engine's host mirror of a device driver's log, copied to `its` with the solve's time spread
// evenly over the entries; nullptr: the driver logged into `its` itself.
// jac_passes < 0: the pass counters of the engine; else the count to report (resident solve).
static int summarize_solve(pba_engine* e, const pba_solver_options* o, const pba::LmState* st, const pba_iteration_summary* device_log,
                           pba_solver_summary* sum, pba_iteration_summary* its, int32_t max_out, double t_start, bool verbose,
                           int64_t jac_passes) {
  const pba::LmState fin = *st;
  const double total = now() - t_start;
  const int n_log = fin.n_log;
  for (int i = 0; i < n_log && i < max_out && its; ++i) {
    if (device_log) {
      its[i] = device_log[i];
      its[i].iteration_time_in_seconds = total / (n_log > 0 ? n_log : 1);
      its[i].cumulative_time_in_seconds = total * (i + 1) / (n_log > 0 ? n_log : 1);
    }
    if (verbose)
      std::printf("%4d  cost % .6e  change % .3e  |grad| %.3e  |step| %.3e  rho % .3e  radius %.3e  %s\n", its[i].iteration, its[i].cost,
                  its[i].cost_change, its[i].gradient_max_norm, its[i].step_norm, its[i].relative_decrease, its[i].trust_region_radius,
                  its[i].step_is_successful ? "ok" : (its[i].step_is_valid ? "rejected" : "invalid"));
  }
  // pose-only mode: the constant camera's residual blocks left the program; Ceres' summary adds their cost back (0 outside the mode)
  sum->fixed_cost = pba_internal_fixed_cost(e);
  sum->initial_cost = fin.initial_cost + sum->fixed_cost;
  sum->final_cost = fin.minimum_cost + sum->fixed_cost;
  sum->num_successful_steps = fin.num_successful;
  sum->num_unsuccessful_steps = fin.num_unsuccessful;
  sum->num_iterations = n_log < max_out ? n_log : max_out;
  sum->num_resolve_passes = fin.num_unsuccessful;
  pba_internal_pass_counts(e, &sum->num_jacobian_passes, &sum->num_cost_passes);
  if (jac_passes >= 0) { sum->num_jacobian_passes = jac_passes; sum->num_cost_passes = 0; }
  switch (fin.done) {
    case pba::kLmGradientTolerance:
      sum->termination_type = 0;
      std::snprintf(sum->message, sizeof(sum->message), "Gradient tolerance reached. Gradient max norm: %e <= %e", fin.last_value[0], o->gradient_tolerance);
      break;
    case pba::kLmMinRadius:
      sum->termination_type = 0;
      std::snprintf(sum->message, sizeof(sum->message), "Minimum trust region radius reached. Trust region radius: %e <= %e", fin.radius, o->min_trust_region_radius);
      break;
    case pba::kLmParameterTolerance:
      sum->termination_type = 0;
      std::snprintf(sum->message, sizeof(sum->message), "Parameter tolerance reached. Relative step_norm: %e <= %e.", fin.last_value[0], o->parameter_tolerance);
      break;
    case pba::kLmFunctionTolerance:
      sum->termination_type = 0;
      std::snprintf(sum->message, sizeof(sum->message), "Function tolerance reached. |cost_change|/cost: %e <= %e", fin.last_value[0], o->function_tolerance);
      break;
    case pba::kLmInvalidSteps:
      sum->termination_type = 2;
      std::snprintf(sum->message, sizeof(sum->message), "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d", o->max_num_consecutive_invalid_steps);
      break;
    case pba::kLmEvalFailure:
      sum->termination_type = 2;
      std::snprintf(sum->message, sizeof(sum->message), fin.n_log == 0 ? "Initial residual and Jacobian evaluation failed." : "Residual and Jacobian evaluation failed.");
      break;
    default:
      sum->termination_type = 1;
      std::snprintf(sum->message, sizeof(sum->message), "Maximum number of iterations reached. Number of iterations: %d.", fin.iteration);
      break;
  }
  sum->total_time_in_seconds = now() - t_start;
  return PBA_OK;
}

// Host-stepped variant: one step per round trip.  Every trip computes one trust-region step with the damping of the state (and, with it,
// cost and gradient norms of the current point), hands the step's scalar block to lm_decide and acts on the outcome: an accepted
// candidate becomes the current point (its Jacobian pass has usually run already: the candidate pass speculates on acceptance as long
// as steps are accepted), a rejected or invalid one makes the next trip re-solve the stored linearisation with the new damping.
// The state lives here and the log is the caller's array, so the iteration limit is not bounded by the device log.
static int solve_host_stepped(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum, pba_iteration_summary* its,
                              int32_t max_out, double t_start, bool verbose) {
  const int max_log = its ? max_out : 0;
  pba::LmState st = pba::lm_initial_state(o, 0);      // (only the FLIPS of the parity are used here: the engine keeps its own)
  pba_internal_reset_pass_counts(e);
  pba_internal_set_speculate(e, 1);
  int rc = pba_linearize(e, nullptr);
  if (rc) return rc;
  int64_t resolves = 0;
  bool resolve = false;      // this trip's step is a re-solve: its predecessor was rejected or invalid
  for (;;) {
    const double t_trip = now();
    // the gradient norms alone: iteration zero of a zero-iteration solve, and the point accepted by the last iteration allowed
    const int grad_only = st.first ? o->max_num_iterations <= 0 : st.iteration >= o->max_num_iterations;
    pba_step_info info;
    double s[pba::kNumScal];
    rc = pba_internal_step(e, st.radius, st.first, o, &info, s, grad_only);
    // a non-finite residual at the linearisation point is lm_decide's to rule on (kEvalFailLin): the solve fails, the call does not
    if (rc && rc != PBA_ERR_NUMERIC) return rc;
    const double t_step = now() - t_trip;
    if (resolve) ++resolves;
    const int cur = st.cur, n0 = st.n_log;
    pba::lm_decide(&st, s, its, max_log, grad_only);
    const bool accepted = st.cur != cur;
    if (accepted) {
      pba_internal_set_speculate(e, 1);   // accepted: keep betting on acceptance
      if ((rc = pba_accept(e))) return rc;
      if ((rc = pba_linearize(e, nullptr))) return rc;   // no-op when the candidate pass was a Jacobian pass
    } else if (!st.done) {
      pba_internal_set_speculate(e, 0);   // rejected or invalid: the retry only needs the cost
    }
    const double t = now();
    for (int i = n0; i < st.n_log && i < max_log; ++i) {
      its[i].iteration_time_in_seconds = t - t_trip;
      its[i].cumulative_time_in_seconds = t - t_start;
      if (resolve) its[i].step_solver_time_in_seconds = t_step;
    }
    resolve = !accepted;
    // the one trip after the end: the iteration limit right after an acceptance still owes that point's gradient norms
    if (st.done && !(st.done == pba::kLmMaxIterations && !grad_only && pba::lm_final_pass_needed(&st))) break;
  }
  rc = summarize_solve(e, o, &st, nullptr, sum, its, max_out, t_start, verbose, -1);
  sum->num_resolve_passes = resolves;      // the re-solves actually run (include/pba.h)
  return rc;
}

extern "C" int pba_solve(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum, pba_iteration_summary* its,
                         int32_t max_out) {
  if (!e || !o || !sum) return PBA_ERR_INVALID;
  { const int rc0 = pba_internal_ready(e); if (rc0) return rc0; }   // solve before set_problem / set_cameras: PBA_ERR_STATE
  const double t_start = now();
  std::memset(sum, 0, sizeof(*sum));
  sum->termination_type = 1;
  std::snprintf(sum->message, sizeof(sum->message), "Maximum number of iterations reached.");
  const bool pose = pba_internal_points_constant(e) != 0;
  double blocks = (double)(pose ? pba_internal_program_blocks(e) : pba_internal_local_blocks(e));
  if (pose && blocks == 0.0) {
    // Ceres' reduced program is empty: every residual block hangs on constant parameter blocks only
    std::snprintf(sum->message, sizeof(sum->message), "No free camera has a residual block: with every point constant the program is empty.");
    return pba_internal_refuse(e, PBA_ERR_INVALID, sum->message);
  }
  if (pba_internal_allreduce_host(e, &blocks, 1, 0)) return PBA_ERR_COMM;
  // ceres::Solver::Summary counts in `int` (the reference's numResiduals too): a window beyond that range is refused up front
  // instead of reporting a wrapped count (3.2 M blocks x 121 pixels x 8 channels would)
  if (blocks * pba_internal_patch_len(e) > 2147483647.0) {
    std::snprintf(sum->message, sizeof(sum->message), "%.0f residual blocks x %d residuals exceed the int32 range of the summary", blocks, pba_internal_patch_len(e));
    return PBA_ERR_INVALID;
  }
  sum->num_residual_blocks = (int32_t)blocks;
  sum->num_residuals = (int32_t)(blocks * pba_internal_patch_len(e));
  const bool verbose = o->verbose && pba_internal_rank(e) == 0;
  if (!pba_internal_async_capable(e, o)) return solve_host_stepped(e, o, sum, its, max_out, t_start, verbose);
  pba_internal_reset_pass_counts(e);
  if (pba_internal_resident_capable(e, o)) return solve_resident(e, o, sum, its, max_out, t_start, verbose);
  return solve_async(e, o, sum, its, max_out, t_start, verbose);
}

// Batch variant of solve_async: n independent windows, one batched launch per phase on ONE stream (pba_batch.h).  Each window follows the
// loop of solve_async step for step -- the same enqueue / wait rule per window, the same final pass through lm_final_pass_needed, the
// same summary -- and all windows still running advance together, so window w's k-th full iteration is in the batch's k-th launch.
extern "C" int pba_solve_batch(pba_engine* const* es, int32_t n, const pba_solver_options* options, pba_solver_summary* sums,
                               pba_iteration_summary* its, int32_t max_out) {
  constexpr int kAhead = 3;     // solve_async's
  if (!es || !sums || n < 1 || n > PBA_MAX_BATCH || (its && max_out < 0)) return PBA_ERR_INVALID;
  std::vector<pba_solver_options> o((size_t)n);
  for (int w = 0; w < n; ++w) {
    if (options) o[w] = options[w];
    else pba_default_solver_options(&o[w]);
  }
  { const int rc = pba_internal_batch_validate(es, n, o.data()); if (rc) return rc; }
  const double t_start = now();
  for (int w = 0; w < n; ++w) {
    pba_solver_summary* sum = &sums[w];
    std::memset(sum, 0, sizeof(*sum));
    sum->termination_type = 1;
    std::snprintf(sum->message, sizeof(sum->message), "Maximum number of iterations reached.");
    sum->num_residual_blocks = (int32_t)pba_internal_local_blocks(es[w]);
    sum->num_residuals = (int32_t)(pba_internal_local_blocks(es[w]) * pba_internal_patch_len(es[w]));
    sum->fixed_cost = 0.0;
    pba_internal_reset_pass_counts(es[w]);
  }
  int rc = pba_internal_batch_begin(es, n, o.data());
  enum { kRunning, kFinished };
  std::vector<int> phase((size_t)n, kRunning), enq((size_t)n, 0);
  std::vector<unsigned long long> final_seq((size_t)n, 0), ring((size_t)n * (kAhead + 1), 0), seq_k((size_t)n, 0);
  std::vector<int32_t> sel, fin;
  sel.reserve(n); fin.reserve(n);
  for (int w = 0; w < n && !rc; ++w) sel.push_back(w);
  if (!rc) rc = pba_internal_batch_enqueue(es, sel.data(), (int32_t)sel.size(), 0, 0, seq_k.data());
  for (int j = 0; !rc; ++j) {
    sel.clear(); fin.clear();
    for (int w = 0; w < n; ++w) {
      if (phase[w] != kRunning) continue;
      const volatile pba::LmState* st = static_cast<const volatile pba::LmState*>(pba_internal_async_state(es[w]));
      if (enq[w] >= o[w].max_num_iterations) { phase[w] = kFinished; fin.push_back(w); continue; }   // the iteration limit: final pass
      if (st->done) {             // terminated: the flush alone (kind 3)
        phase[w] = kFinished;
        if ((rc = pba_internal_async_enqueue(es[w], 3, 0, &o[w], &final_seq[w]))) break;
        continue;
      }
      sel.push_back(w);
    }
    if (rc) break;
    if (!fin.empty()) {
      // gradient norms of the final point, gated on the device (lm_final_pass_needed); single rank, it decides and flushes itself
      std::vector<int32_t> fused;
      for (int32_t w : fin) {
        if (pba_internal_final_flushes(es[w])) { fused.push_back(w); continue; }
        unsigned long long s2 = 0;
        if ((rc = pba_internal_async_enqueue(es[w], 2, o[w].max_num_iterations <= 0 ? 1 : 0, &o[w], &s2))) break;
        if ((rc = pba_internal_async_enqueue(es[w], 3, 0, &o[w], &final_seq[w]))) break;
      }
      if (rc) break;
      if (!fused.empty()) {
        if ((rc = pba_internal_batch_enqueue(es, fused.data(), (int32_t)fused.size(), 2, 0, seq_k.data()))) break;
        for (size_t k = 0; k < fused.size(); ++k) final_seq[fused[k]] = seq_k[k];
      }
    }
    if (sel.empty()) break;
    if ((rc = pba_internal_batch_enqueue(es, sel.data(), (int32_t)sel.size(), 1, j == 0 ? 1 : 0, seq_k.data()))) break;
    for (size_t k = 0; k < sel.size() && !rc; ++k) {
      const int w = sel[k];
      unsigned long long* seqs = &ring[(size_t)w * (kAhead + 1)];
      seqs[enq[w] % (kAhead + 1)] = seq_k[k];
      ++enq[w];
      if (enq[w] > kAhead) rc = pba_internal_async_wait(es[w], seqs[(enq[w] - kAhead) % (kAhead + 1)]);
    }
  }
  for (int w = 0; w < n && !rc; ++w) {
    if ((rc = pba_internal_async_wait(es[w], final_seq[w]))) break;
    rc = pba_internal_async_end(es[w]);
  }
  pba_internal_batch_end(es, n, rc != 0);
  if (rc) return rc;
  for (int w = 0; w < n; ++w) {
    const bool verbose = o[w].verbose != 0;
    const int rcw = summarize_solve(es[w], &o[w], mirror(es[w]), pba_internal_async_log(es[w]), &sums[w],
                                    its ? its + (size_t)w * (size_t)max_out : nullptr, its ? max_out : 0, t_start, verbose, -1);
    if (rcw) return rcw;
  }
  return PBA_OK;
}
