// pba_lm_rules.h -- THE trust-region rules of the solver: Ceres (>= 1.12) TrustRegionMinimizer + LevenbergMarquardtStrategy with the
// settings of GetSolverOptions (reference src/photobundle.cc:738-761) and the Ceres defaults listed in SURVEY.md 8c, restated once as
// a state (LmState) and one decision per step (lm_decide) on the step's scalar block.  Every driver runs this code: the host-stepped
// loop of pba_lm.cpp on the host, the pipelined, batched and resident drivers in a workgroup on the device.  No HIP header is needed:
// plain C++ compiles it (tests/native/host_probe.cpp does).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pba.h"

#if defined(__HIPCC__)
#define PBA_LM_FN __host__ __device__ inline
#else
#define PBA_LM_FN inline
#endif

namespace pba {

// Scalar block of one step (Engine::d_scal), grouped so that the multi-rank transports can reduce slices in place.
enum Scal {
  // --- group B, SUM over ranks after the cost pass -------------------------------------------------
  kCandCost = 0,    // candidate cost (local shard)
  kMccPts,          // point part of the model cost change
  kStep2Pts,        // sum delta_p^2
  kX2Pts,           // sum xyz^2 at the current point
  kSumBCount = 4,
  // --- group M, MAX over ranks ----------------------------------------------------------------------
  kGmaxPts = 8,     // max |g_p|
  kSchurFail,       // > 0: a damped point block was not PD
  kEvalFailLin,     // > 0: non-finite residual block in the Jacobian pass
  kEvalFailCand,    // > 0: non-finite residual block in the cost pass
  kMaxCount = 4,
  // --- replicated (identical on every rank, never reduced) --------------------------------------------
  kMccCams = 16,
  kStep2Cams,
  kX2Cams,
  kGmaxCams,
  kGnorm2Cams,
  kSolveOk,         // reduced-system Cholesky succeeded and the camera step is finite
  kCostLin,         // GLOBAL cost at the linearisation point (copied out of the reduced packed buffer)
  kGnorm2Pts,       // GLOBAL sum g_p^2
  kNumScal = 32
};

enum LmTermination { kLmRunning = 0, kLmMaxIterations, kLmGradientTolerance, kLmMinRadius, kLmParameterTolerance,
                     kLmFunctionTolerance, kLmInvalidSteps, kLmEvalFailure };

// The trust-region state of one solve.  The device drivers keep it in device memory (mirrored to the host at every publish) so that
// the host can enqueue iterations back to back; the host-stepped driver keeps it on its stack.
struct LmState {
  double radius, decrease_factor, x_cost, minimum_cost, initial_cost;
  double last_value[2];        // termination detail (e.g. step norm ratio)
  int32_t cur;                 // parity of the current point
  int32_t iteration;           // iterations completed (log entries written = n_log)
  int32_t done;                // LmTermination
  int32_t num_invalid, num_successful, num_unsuccessful;
  int32_t pending_grad;        // log index still waiting for the gradient norms of its (accepted) point, -1 none
  int32_t n_log;
  int32_t first;               // 1 until iteration 0 has been logged
  int32_t pad;
  // options
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double max_radius, min_radius, min_relative_decrease;
  int32_t max_num_iterations, max_invalid;
  unsigned long long done_seq;   // sequence number of the step that terminated the solve (0 while running)
};

// The state before iteration zero; cur = parity of the current point.
PBA_LM_FN LmState lm_initial_state(const pba_solver_options* o, int cur) {
  LmState st;
  memset(&st, 0, sizeof(st));
  st.radius = o->initial_trust_region_radius; st.decrease_factor = 2.0;
  st.cur = cur; st.pending_grad = -1; st.first = 1;
  st.function_tolerance = o->function_tolerance; st.gradient_tolerance = o->gradient_tolerance;
  st.parameter_tolerance = o->parameter_tolerance; st.max_radius = o->max_trust_region_radius;
  st.min_radius = o->min_trust_region_radius; st.min_relative_decrease = o->min_relative_decrease;
  st.max_num_iterations = o->max_num_iterations; st.max_invalid = o->max_num_consecutive_invalid_steps;
  return st;
}

// The cube of LevenbergMarquardtStrategy::StepAccepted -- the ONE place where the host and the device may round differently, on
// purpose: a device decision multiplies (the bits of the pipelined, batched and resident drivers), a host decision calls pow as Ceres
// does (the bits of the host-stepped driver).  Both are pinned by tests/golden/solve_bits.json; the radii of the two differ by an ulp
// or so per accepted step.  Everything else in this file is the same arithmetic on both sides.
PBA_LM_FN double lm_cube(double t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return t * t * t;
#else
  return pow(t, 3.0);
#endif
}

PBA_LM_FN __attribute__((always_inline)) void lm_step_rejected(LmState* st) {   // LevenbergMarquardtStrategy::StepRejected
  st->radius = st->radius / st->decrease_factor;
  st->decrease_factor *= 2.0;
}

// n_log counts every entry, also those beyond max_log (which are dropped): a short log does not change the solve.
PBA_LM_FN void lm_log(LmState* st, pba_iteration_summary* log, int max_log, const pba_iteration_summary& it) {
  if (st->n_log < max_log) log[st->n_log] = it;
  st->n_log++;
}

// Gate of the final (gradient-only) pass, evaluated where the state lives so that the host can enqueue that pass without first
// reading the state back: it is needed for iteration zero of a zero-iteration solve and when the iteration limit was
// reached right after an accepted step (whose gradient norms are still to be reported).
PBA_LM_FN __attribute__((always_inline)) bool lm_final_pass_needed(const LmState* st) {
  return st->first || (st->pending_grad >= 0 && (st->done == kLmRunning || st->done == kLmMaxIterations));
}

// One decision.  `s` = the step's (fully reduced) scalar block: cost and gradient norms of the current point, the step computed
// there and the cost of its candidate.  grad_only: only the gradient norms of the current point are valid.
// The gradient norms of an accepted point come with the NEXT block (the pass that computes them also computes the next step), so
// the gradient-tolerance and minimum-radius checks of an accepted iteration are deferred to the next decision (pending_grad).
PBA_LM_FN void lm_decide(LmState* st, const double* s, pba_iteration_summary* log, int max_log, int grad_only) {
  const double gmax = fmax(s[kGmaxPts], s[kGmaxCams]);
  const double gnorm = sqrt(s[kGnorm2Pts] + s[kGnorm2Cams]);
  if (st->done) {
    // final pass after the iteration limit: only report the gradient norms of the last accepted point
    if (grad_only && st->done == kLmMaxIterations && st->pending_grad >= 0 && !st->first) {
      if (st->pending_grad < max_log) { log[st->pending_grad].gradient_max_norm = gmax; log[st->pending_grad].gradient_norm = gnorm; }
      st->pending_grad = -1;
    }
    return;
  }
  pba_iteration_summary it;
  memset(&it, 0, sizeof(it));
  it.eta = 1e-1;
  if (st->first) {
    // IterationZero
    if (s[kEvalFailLin] > 0.5) { st->done = kLmEvalFailure; return; }
    st->first = 0;
    st->x_cost = s[kCostLin];
    st->initial_cost = st->x_cost;
    st->minimum_cost = st->x_cost;
    it.iteration = 0; it.cost = st->x_cost; it.gradient_max_norm = gmax; it.gradient_norm = gnorm;
    it.step_is_valid = 1; it.step_is_successful = 1; it.trust_region_radius = st->radius;
    st->num_successful = 1;
    lm_log(st, log, max_log, it);
    if (0 >= st->max_num_iterations) st->done = kLmMaxIterations;
    else if (gmax <= st->gradient_tolerance) { st->done = kLmGradientTolerance; st->last_value[0] = gmax; }
    else if (st->radius <= st->min_radius) st->done = kLmMinRadius;
    if (st->done) return;
    // the record of iteration zero is out; iteration one starts from a clean one (its step_is_successful / step_is_valid
    // flags used to survive into a REJECTED first step's log entry)
    memset(&it, 0, sizeof(it));
    it.eta = 1e-1;
  } else if (st->pending_grad >= 0) {
    // gradient norms of the point accepted by the previous iteration + its deferred termination checks
    if (st->pending_grad < max_log) { log[st->pending_grad].gradient_max_norm = gmax; log[st->pending_grad].gradient_norm = gnorm; }
    st->pending_grad = -1;
    if (s[kEvalFailLin] > 0.5) { st->done = kLmEvalFailure; return; }
    if (gmax <= st->gradient_tolerance) { st->done = kLmGradientTolerance; st->last_value[0] = gmax; return; }
    if (st->radius <= st->min_radius) { st->done = kLmMinRadius; return; }
  }
  if (grad_only) return;

  const int iteration = st->iteration + 1;
  it.iteration = iteration;
  it.gradient_max_norm = gmax; it.gradient_norm = gnorm;
  it.linear_solver_iterations = 1;
  it.model_cost_change = s[kMccPts] + s[kMccCams];
  const bool solver_ok = s[kSolveOk] > 0.5 && s[kSchurFail] < 0.5;
  const bool step_is_valid = solver_ok && it.model_cost_change > 0.0;
  bool successful = false;
  if (!step_is_valid) {
    // HandleInvalidStep
    st->num_invalid++;
    it.cost = st->x_cost;
    if (st->num_invalid >= st->max_invalid) {
      it.trust_region_radius = st->radius;
      lm_log(st, log, max_log, it);
      st->iteration = iteration;
      st->done = kLmInvalidSteps;
      return;
    }
    lm_step_rejected(st);
  } else {
    it.step_is_valid = 1;
    st->num_invalid = 0;
    const bool eval_ok = s[kEvalFailCand] < 0.5 && isfinite(s[kCandCost]);
    const double candidate_cost = eval_ok ? s[kCandCost] : DBL_MAX;
    it.candidate_cost = candidate_cost;
    it.step_norm = sqrt(s[kStep2Pts] + s[kStep2Cams]);
    const double x_norm = sqrt(s[kX2Pts] + s[kX2Cams]);
    if (it.step_norm <= st->parameter_tolerance * (x_norm + st->parameter_tolerance)) {   // ParameterToleranceReached
      st->done = kLmParameterTolerance;
      st->last_value[0] = it.step_norm / (x_norm + st->parameter_tolerance);
      return;
    }
    it.cost_change = st->x_cost - candidate_cost;
    if (fabs(it.cost_change) <= st->function_tolerance * st->x_cost) {                    // FunctionToleranceReached
      st->done = kLmFunctionTolerance;
      st->last_value[0] = fabs(it.cost_change) / st->x_cost;
      return;
    }
    it.relative_decrease = it.cost_change / it.model_cost_change;
    if (it.relative_decrease > st->min_relative_decrease) {
      // HandleSuccessfulStep + LevenbergMarquardtStrategy::StepAccepted
      successful = true;
      st->cur ^= 1;
      st->x_cost = candidate_cost;
      const double t = 2.0 * it.relative_decrease - 1.0;
      st->radius = st->radius / fmax(1.0 / 3.0, 1.0 - lm_cube(t));
      st->radius = fmin(st->max_radius, st->radius);
      st->decrease_factor = 2.0;
      it.step_is_successful = 1;
      it.cost = st->x_cost;
      st->pending_grad = st->n_log;
    } else {
      lm_step_rejected(st);
      it.cost = candidate_cost;
    }
  }
  // FinalizeIterationAndCheckIfMinimizerCanContinue (gradient tolerance deferred to the next decision)
  if (successful) { st->num_successful++; st->minimum_cost = st->x_cost; }
  else st->num_unsuccessful++;
  it.trust_region_radius = st->radius;
  lm_log(st, log, max_log, it);
  st->iteration = iteration;
  if (iteration >= st->max_num_iterations) st->done = kLmMaxIterations;
  else if (!successful && st->radius <= st->min_radius) st->done = kLmMinRadius;
}

}  // namespace pba
