"""The trust-region rules of the solver (photobundle_amd/csrc/pba_lm_rules.h: lm_initial_state, lm_decide, lm_final_pass_needed) without
a device.  The header is plain C++; tests/native/host_probe.cpp includes it and exposes one hook, so what runs here is the HOST form of
the rules -- the form the host-stepped driver runs (the cube of StepAccepted through pow, as Ceres computes it).

Two references, neither derived from the header:
  * hand-made scalar blocks, one per rule and one value on each side of every threshold, against `ceres_rules` below: Ceres'
    TrustRegionMinimizer + LevenbergMarquardtStrategy written down from their documented control flow.  Everything the rules compute is
    compared exactly, the radius included.
  * the CPU oracle (its own, independent loop in oracle/pba_oracle.cpp): its solves of the windows and option sets of
    tests/test_oracle_solver_options.py are replayed -- every iteration's scalar block is built from the oracle's iteration records -- and
    the rules must log the same iterations and end the same way.  The parameter-tolerance case is not replayed: the oracle's records do
    not hold |x|, so that rule is the hand-made table's alone (kX2* = 0 keeps it silent in the replay).

The loop that feeds the rules (`run_rules`) is the schedule of the host-stepped driver: one block per trip, gradient-only where only the
gradient norms of the current point are due, and one more trip after the end when lm_final_pass_needed says so.

Where the project's rule set deliberately differs from Ceres the restatement says so in place: a failed evaluation
at a freshly accepted point leaves that iteration logged and counted."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import _lib

import test_oracle_solver_options as opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = sys.float_info.max

# pba_lm_rules.h: enum Scal / enum LmTermination / struct LmState
K = dict(cand=0, mcc_pts=1, step2_pts=2, x2_pts=3, gmax_pts=8, schur_fail=9, eval_fail_lin=10, eval_fail_cand=11, mcc_cams=16, step2_cams=17,
         x2_cams=18, gmax_cams=19, gnorm2_cams=20, solve_ok=21, cost=22, gnorm2_pts=23)
RUNNING, MAX_IT, GRAD, MIN_RADIUS, PARAM, FUNC, INVALID, EVAL_FAIL = range(8)


class LmState(C.Structure):
    _fields_ = [("radius", C.c_double), ("decrease_factor", C.c_double), ("x_cost", C.c_double), ("minimum_cost", C.c_double),
                ("initial_cost", C.c_double), ("last_value", C.c_double * 2), ("cur", C.c_int32), ("iteration", C.c_int32),
                ("done", C.c_int32), ("num_invalid", C.c_int32), ("num_successful", C.c_int32), ("num_unsuccessful", C.c_int32),
                ("pending_grad", C.c_int32), ("n_log", C.c_int32), ("first", C.c_int32), ("pad", C.c_int32),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("max_num_iterations", C.c_int32), ("max_invalid", C.c_int32), ("done_seq", C.c_ulonglong)]


@functools.lru_cache(None)
def probe():
    L = C.CDLL(os.path.join(ROOT, "tests", "native", "libhost_probe.so"))
    L.pb_lm_rules.restype = C.c_int
    L.pb_lm_rules.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return L


def options(**kw):
    """pba_solver_options: the reference's values (include/pba.h) unless given."""
    o = _lib.SolverOptions(max_num_iterations=500, max_num_consecutive_invalid_steps=5, function_tolerance=1e-6, gradient_tolerance=1e-6,
                           parameter_tolerance=1e-6, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
                           min_trust_region_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                           jacobi_scaling=1, verbose=0)
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def scalars(b, grad_only):
    """The 32-double scalar block of the dict b; a gradient-only block carries NaN wherever a step's figures would be."""
    s = np.zeros(32)
    s[K["cost"]], s[K["eval_fail_lin"]] = b["cost"], b.get("eval_fail_lin", 0.0)
    s[K["gmax_pts"]], s[K["gmax_cams"]] = b["gmax"]
    s[K["gnorm2_pts"]], s[K["gnorm2_cams"]] = b["gnorm2"]
    names = ("cand", "mcc_pts", "mcc_cams", "step2_pts", "step2_cams", "x2_pts", "x2_cams", "schur_fail", "eval_fail_cand", "solve_ok")
    for n in names:
        s[K[n]] = np.nan if grad_only else b["step"][n]
    return s


def run_rules(o, next_block, max_log=64):
    """The host-stepped schedule over the rules.  next_block(state, grad_only) -> block dict.  Returns (final state, log entries as
    dicts, [lm_final_pass_needed after the initial state and after every trip], [grad_only of every trip])."""
    L, st = probe(), LmState()
    log = (_lib.IterationSummary * max(max_log, 1))()
    needed = [L.pb_lm_rules(C.byref(o), C.byref(st), C.sizeof(st), None, 0, None, 0)]
    assert needed[0] >= 0, "LmState above does not mirror the header's"
    flags = []
    while True:
        grad_only = int(o.max_num_iterations <= 0 if st.first else st.iteration >= o.max_num_iterations)
        s = scalars(next_block(st, grad_only), grad_only)
        needed.append(L.pb_lm_rules(C.byref(o), C.byref(st), C.sizeof(st), s.ctypes.data, grad_only, log, max_log))
        flags.append(grad_only)
        assert len(flags) < 5000
        if st.done and not (st.done == MAX_IT and not grad_only and needed[-1]):
            break
    entries = [{f: getattr(log[i], f) for f, _ in _lib.IterationSummary._fields_} for i in range(min(st.n_log, max_log))]
    return st, entries, needed, flags


def message(st, o):
    """The termination message of a final state, as the summary of every driver words it (pba_lm.cpp: summarize_solve)."""
    if st.done == GRAD:
        return "Gradient tolerance reached. Gradient max norm: %e <= %e" % (st.last_value[0], o.gradient_tolerance)
    if st.done == MIN_RADIUS:
        return "Minimum trust region radius reached. Trust region radius: %e <= %e" % (st.radius, o.min_trust_region_radius)
    if st.done == PARAM:
        return "Parameter tolerance reached. Relative step_norm: %e <= %e." % (st.last_value[0], o.parameter_tolerance)
    if st.done == FUNC:
        return "Function tolerance reached. |cost_change|/cost: %e <= %e" % (st.last_value[0], o.function_tolerance)
    if st.done == INVALID:
        return ("Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d"
                % o.max_num_consecutive_invalid_steps)
    if st.done == EVAL_FAIL:
        return "Initial residual and Jacobian evaluation failed." if st.n_log == 0 else "Residual and Jacobian evaluation failed."
    assert st.done == MAX_IT
    return "Maximum number of iterations reached. Number of iterations: %d." % st.iteration


# ---- Ceres' rules, restated ---------------------------------------------------------------------------------------------------------
def ceres_rules(o, blocks):
    """TrustRegionMinimizer::Minimize with LevenbergMarquardtStrategy on a list of blocks.  blocks[k]["step"] is the trust-region step
    computed with the damping in force when block k was made (the step of the next iteration); cost and gradient norms of a block are
    those of the point it was made at, so an accepted iteration reads its new point's gradient from the NEXT block.
    Returns dict(kind, message, radius, log, used, owed, successful, unsuccessful, minimum_cost): used = blocks read; owed[k] = block k's
    step was accepted, so right after block k the gradient norms of the new point are still owed to the log."""
    gmax = lambda b: max(b["gmax"])
    gnorm = lambda b: math.sqrt(b["gnorm2"][0] + b["gnorm2"][1])
    out = dict(log=[], successful=0, unsuccessful=0)
    b = blocks[0]
    if b.get("eval_fail_lin", 0.0) > 0.5:
        # (iteration zero is never logged, which lm_final_pass_needed reports as a pass still due: the drivers stop on the failure)
        return dict(out, kind=EVAL_FAIL, message="Initial residual and Jacobian evaluation failed.", radius=o.initial_trust_region_radius,
                    minimum_cost=0.0, used=1, owed=[True])
    x_cost = minimum_cost = b["cost"]
    radius, decrease_factor, n_invalid = o.initial_trust_region_radius, 2.0, 0
    it = dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=x_cost, gradient_max_norm=gmax(b), gradient_norm=gnorm(b))
    accepted_on = set()

    def finalize(eval_failed=False):
        # FinalizeIterationAndCheckIfMinimizerCanContinue
        nonlocal minimum_cost
        if it["step_is_successful"]:
            out["successful"] += 1
            if x_cost < minimum_cost or it["iteration"] == 0:
                minimum_cost = x_cost
        else:
            out["unsuccessful"] += 1
        it["trust_region_radius"] = radius
        out["log"].append(dict(it))
        if it["iteration"] >= o.max_num_iterations:
            return MAX_IT, "Maximum number of iterations reached. Number of iterations: %d." % it["iteration"]
        if eval_failed:
            # Ceres ends the solve inside HandleSuccessfulStep, before this iteration is logged or counted; the project's rule set logs
            # and counts the accepted iteration first, and at the iteration limit the limit wins
            return EVAL_FAIL, "Residual and Jacobian evaluation failed."
        if it["step_is_successful"] and it["gradient_max_norm"] <= o.gradient_tolerance:
            return GRAD, "Gradient tolerance reached. Gradient max norm: %e <= %e" % (it["gradient_max_norm"], o.gradient_tolerance)
        if radius <= o.min_trust_region_radius:
            return MIN_RADIUS, "Minimum trust region radius reached. Trust region radius: %e <= %e" % (radius, o.min_trust_region_radius)
        return None

    def step_rejected():     # LevenbergMarquardtStrategy::StepRejected
        nonlocal radius, decrease_factor
        radius = radius / decrease_factor
        decrease_factor *= 2.0

    end = finalize()
    k = 0      # the block that holds the step of the next iteration (the highest block read so far)
    while end is None:
        s = blocks[k]["step"]
        it = dict(iteration=it["iteration"] + 1, step_is_valid=0, step_is_successful=0, gradient_max_norm=it["gradient_max_norm"],
                  gradient_norm=it["gradient_norm"])
        it["model_cost_change"] = s["mcc_pts"] + s["mcc_cams"]
        solved = s["solve_ok"] > 0.5 and s["schur_fail"] < 0.5
        if not (solved and it["model_cost_change"] > 0.0):
            # HandleInvalidStep
            n_invalid += 1
            it["cost"] = x_cost
            if n_invalid >= o.max_num_consecutive_invalid_steps:
                it["trust_region_radius"] = radius
                out["log"].append(dict(it))
                end = (INVALID, "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d"
                       % o.max_num_consecutive_invalid_steps)
                break
            step_rejected()
            end = finalize()
            k += 0 if end else 1
            continue
        it["step_is_valid"] = 1
        n_invalid = 0
        candidate_cost = s["cand"] if s["eval_fail_cand"] < 0.5 and math.isfinite(s["cand"]) else DBL_MAX
        it["candidate_cost"] = candidate_cost
        it["step_norm"] = math.sqrt(s["step2_pts"] + s["step2_cams"])
        x_norm = math.sqrt(s["x2_pts"] + s["x2_cams"])
        if it["step_norm"] <= o.parameter_tolerance * (x_norm + o.parameter_tolerance):
            end = (PARAM, "Parameter tolerance reached. Relative step_norm: %e <= %e."
                   % (it["step_norm"] / (x_norm + o.parameter_tolerance), o.parameter_tolerance))
            break
        it["cost_change"] = x_cost - candidate_cost
        if abs(it["cost_change"]) <= o.function_tolerance * x_cost:
            end = (FUNC, "Function tolerance reached. |cost_change|/cost: %e <= %e" % (abs(it["cost_change"]) / x_cost, o.function_tolerance))
            break
        it["relative_decrease"] = it["cost_change"] / it["model_cost_change"]
        if it["relative_decrease"] > o.min_relative_decrease:
            # HandleSuccessfulStep; LevenbergMarquardtStrategy::StepAccepted
            x_cost = candidate_cost
            it["step_is_successful"], it["cost"] = 1, x_cost
            radius = radius / max(1.0 / 3.0, 1.0 - (2.0 * it["relative_decrease"] - 1.0) ** 3)
            radius = min(o.max_trust_region_radius, radius)
            decrease_factor = 2.0
            accepted_on.add(k)
            k += 1
            nb = blocks[k]      # made at the accepted point: its gradient norms, and whether it could be evaluated at all
            it["gradient_max_norm"], it["gradient_norm"] = gmax(nb), gnorm(nb)
            end = finalize(nb.get("eval_fail_lin", 0.0) > 0.5)
        else:
            step_rejected()
            it["cost"] = candidate_cost
            end = finalize()
            k += 0 if end else 1
    return dict(out, kind=end[0], message=end[1], radius=radius, minimum_cost=minimum_cost, used=k + 1,
                owed=[i in accepted_on for i in range(k + 1)])


# ---- hand-made blocks ------------------------------------------------------------------------------------------------------------
def step(cand, mcc=(0.25, 0.75), step2=(0.5, 0.5), x2=(60.0, 40.0), solve_ok=1.0, schur_fail=0.0, eval_fail_cand=0.0):
    return dict(cand=cand, mcc_pts=mcc[0], mcc_cams=mcc[1], step2_pts=step2[0], step2_cams=step2[1], x2_pts=x2[0], x2_cams=x2[1],
                solve_ok=solve_ok, schur_fail=schur_fail, eval_fail_cand=eval_fail_cand)


def blk(cost, st=None, gmax=(3.0, 5.0), gnorm2=(9.0, 16.0), **kw):
    return dict(cost=cost, gmax=gmax, gnorm2=gnorm2, step=st, **kw)


NONE = step(np.nan)      # the step of a block whose step is never read
UP = float(np.nextafter(1.0, 2.0))
# x_cost = 8 and model cost change = 1 throughout, so relative_decrease = 8 - candidate cost, exactly
ACC = lambda cost, cand, **kw: blk(cost, step(cand), **kw)
TOL0 = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)

CASES = {
    # id: (options, blocks, kind, valid/successful flags of the log as a string: S accepted, R rejected, I invalid)
    "zero_iteration_limit": (dict(max_num_iterations=0), [blk(8.0, NONE)], MAX_IT, "S"),
    "zero_gradient_at_tolerance": (dict(gradient_tolerance=5.0), [blk(8.0, step(7.0))], GRAD, "S"),
    "zero_gradient_above_tolerance": (dict(TOL0, gradient_tolerance=5.0 / UP, max_num_iterations=1), [blk(8.0, step(7.0)), blk(7.0, NONE)],
                                      MAX_IT, "SS"),
    "zero_gradient_before_min_radius": (dict(gradient_tolerance=5.0, initial_trust_region_radius=2.0, min_trust_region_radius=2.0),
                                        [blk(8.0, step(7.0))], GRAD, "S"),
    "zero_min_radius_at": (dict(TOL0, initial_trust_region_radius=2.0, min_trust_region_radius=2.0), [blk(8.0, step(7.0))], MIN_RADIUS, "S"),
    "zero_min_radius_below": (dict(TOL0, initial_trust_region_radius=2.0 * UP, min_trust_region_radius=2.0, max_num_iterations=1),
                              [blk(8.0, step(7.0)), blk(7.0, NONE)], MAX_IT, "SS"),
    "zero_eval_failure": (dict(), [blk(8.0, step(7.0), eval_fail_lin=1.0)], EVAL_FAIL, ""),
    "zero_eval_failure_zero_limit": (dict(max_num_iterations=0), [blk(8.0, NONE, eval_fail_lin=1.0)], EVAL_FAIL, ""),
    # invalid steps: solver failure, a point block that is not positive definite, model cost change zero and negative
    "invalid_until_limit": (dict(TOL0, max_num_consecutive_invalid_steps=4),
                            [blk(8.0, step(7.0, solve_ok=0.0)), blk(8.0, step(7.0, schur_fail=1.0)), blk(8.0, step(7.0, mcc=(0.5, -0.5))),
                             blk(8.0, step(7.0, mcc=(-1.0, 0.5)))], INVALID, "SIIII"),
    "invalid_one_below_limit": (dict(TOL0, max_num_consecutive_invalid_steps=4, max_num_iterations=4),
                                [blk(8.0, step(7.0, solve_ok=0.0)), blk(8.0, step(7.0, schur_fail=1.0)), blk(8.0, step(7.0, mcc=(0.5, -0.5))),
                                 blk(8.0, step(7.5)), blk(7.5, NONE)], MAX_IT, "SIIIS"),
    "invalid_count_resets": (dict(TOL0, max_num_consecutive_invalid_steps=2, max_num_iterations=4),
                             [blk(8.0, step(7.0, solve_ok=0.0)), blk(8.0, step(7.5)), blk(7.5, step(7.0, schur_fail=1.0)),
                              blk(7.5, step(7.0, solve_ok=0.0))], INVALID, "SISII"),
    "invalid_limit_zero": (dict(TOL0, max_num_consecutive_invalid_steps=0), [blk(8.0, step(7.0, solve_ok=0.0))], INVALID, "SI"),
    "invalid_then_min_radius": (dict(TOL0, max_num_consecutive_invalid_steps=9, initial_trust_region_radius=4.0, min_trust_region_radius=2.0),
                                [blk(8.0, step(7.0, solve_ok=0.0))], MIN_RADIUS, "SI"),
    # parameter tolerance 0.5 at |x| = 2: the threshold is 1.25; the second step norm is 1.25 + 2^-20, whose square is exact
    "parameter_at_tolerance": (dict(TOL0, parameter_tolerance=0.5), [blk(8.0, step(7.0, step2=(0.5625, 1.0), x2=(1.0, 3.0)))], PARAM, "S"),
    "parameter_above_tolerance": (dict(TOL0, parameter_tolerance=0.5, max_num_iterations=1),
                                  [blk(8.0, step(7.0, step2=((1.25 + 2.0 ** -20) ** 2 - 1.0, 1.0), x2=(1.0, 3.0))), blk(7.0, NONE)], MAX_IT, "SS"),
    # function tolerance 2^-4 at cost 8: the threshold is a change of 0.5, in either direction
    "function_at_tolerance": (dict(TOL0, function_tolerance=2.0 ** -4), [blk(8.0, step(7.5))], FUNC, "S"),
    "function_at_tolerance_uphill": (dict(TOL0, function_tolerance=2.0 ** -4), [blk(8.0, step(8.5))], FUNC, "S"),
    "function_above_tolerance": (dict(TOL0, function_tolerance=2.0 ** -4, max_num_iterations=1),
                                 [blk(8.0, step(7.5 - 2.0 ** -30)), blk(7.5 - 2.0 ** -30, NONE)], MAX_IT, "SS"),
    # acceptance: relative_decrease = 0.25 exactly is not above min_relative_decrease = 0.25; 0.25 + 2^-40 is
    "accept_just_above": (dict(TOL0, min_relative_decrease=0.25, max_num_iterations=1),
                          [blk(8.0, step(7.75 - 2.0 ** -40)), blk(7.75 - 2.0 ** -40, NONE)], MAX_IT, "SS"),
    "accept_at_threshold_rejected": (dict(TOL0, min_relative_decrease=0.25, max_num_iterations=1), [blk(8.0, step(7.75))], MAX_IT, "SR"),
    "candidate_not_finite": (dict(TOL0, max_num_iterations=2), [blk(8.0, step(np.inf)), blk(8.0, step(np.nan))], MAX_IT, "SRR"),
    "candidate_flagged": (dict(TOL0, max_num_iterations=1), [blk(8.0, step(7.0, eval_fail_cand=1.0))], MAX_IT, "SR"),
    # three rejections divide the radius by 2, 4, 8; an acceptance resets the factor, so the next rejection divides by 2 again
    "decrease_factor_doubles_and_resets": (dict(TOL0, max_num_iterations=5, initial_trust_region_radius=64.0),
                                           [blk(8.0, step(9.0)), blk(8.0, step(9.0)), blk(8.0, step(9.0)), blk(8.0, step(7.5)),
                                            blk(7.5, step(9.0))], MAX_IT, "SRRRSR"),
    "rejected_to_min_radius": (dict(TOL0, initial_trust_region_radius=4.0, min_trust_region_radius=2.0), [blk(8.0, step(9.0))], MIN_RADIUS, "SR"),
    "rejected_above_min_radius": (dict(TOL0, initial_trust_region_radius=4.0 * UP, min_trust_region_radius=2.0, max_num_iterations=1),
                                  [blk(8.0, step(9.0))], MAX_IT, "SR"),
    # the checks of an accepted iteration wait for the next block's gradient norms
    "deferred_gradient_at_tolerance": (dict(TOL0, gradient_tolerance=0.5), [blk(8.0, step(7.5)), blk(7.5, step(7.0), gmax=(0.5, 0.25))],
                                       GRAD, "SS"),
    "deferred_gradient_above_tolerance": (dict(TOL0, gradient_tolerance=0.5, max_num_iterations=2),
                                          [blk(8.0, step(7.5)), blk(7.5, step(7.25), gmax=(0.5 * UP, 0.25)), blk(7.25, NONE, gmax=(0.1, 0.1))],
                                          MAX_IT, "SSS"),
    # 1.6 / 1.125 <= 1.5: the acceptance at relative_decrease 0.25 shrinks the radius below the minimum
    "deferred_min_radius_after_acceptance": (dict(TOL0, initial_trust_region_radius=1.6, min_trust_region_radius=1.5),
                                             [blk(8.0, step(7.75)), blk(7.75, step(7.0))], MIN_RADIUS, "SS"),
    "eval_failure_after_acceptance": (dict(TOL0), [blk(8.0, step(7.5)), blk(7.5, step(7.0), eval_fail_lin=1.0)], EVAL_FAIL, "SS"),
    "limit_then_final_gradient": (dict(TOL0, max_num_iterations=2),
                                  [blk(8.0, step(7.5)), blk(7.5, step(7.25), gmax=(2.0, 1.0), gnorm2=(4.0, 5.0)),
                                   blk(7.25, NONE, gmax=(0.5, 0.75), gnorm2=(0.25, 2.0))], MAX_IT, "SSS"),
    # the gradient tolerance is met at the limit: the limit is checked first
    "limit_before_gradient": (dict(TOL0, gradient_tolerance=1.0, max_num_iterations=1), [blk(8.0, step(7.5)), blk(7.5, NONE, gmax=(0.5, 0.5))],
                              MAX_IT, "SS"),
}

def _flags(log):
    return "".join("S" if e["step_is_successful"] else ("R" if e["step_is_valid"] else "I") for e in log)


COMPARED = ("iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm", "gradient_norm", "step_norm",
            "relative_decrease", "trust_region_radius", "model_cost_change", "candidate_cost")


def check_against_restatement(o, blocks, max_log=64):
    want = ceres_rules(o, blocks)
    fed = []

    def feed(st_, g):
        fed.append(g)
        assert len(fed) <= len(blocks), "the rules ask for a block beyond the case's last one"
        return blocks[len(fed) - 1]
    st, log, needed, grad_only = run_rules(o, feed, max_log)
    assert st.done == want["kind"] and message(st, o) == want["message"]
    assert len(fed) == want["used"], "blocks consumed"
    assert st.n_log == len(want["log"])
    for got, ref in zip(log, want["log"][:max_log]):
        for f in COMPARED:
            assert got[f] == ref.get(f, 0.0), (ref["iteration"], f, got[f], ref.get(f, 0.0))
        assert got["eta"] == 0.1 and got["linear_solver_iterations"] == (1 if ref["iteration"] else 0)
    assert st.radius == want["radius"]
    assert (st.num_successful, st.num_unsuccessful) == (want["successful"], want["unsuccessful"])
    if want["log"]:
        assert st.initial_cost == blocks[0]["cost"] and st.minimum_cost == want["minimum_cost"]
    # lm_final_pass_needed: before iteration zero is logged, and while an accepted point's gradient norms are owed to the log
    assert needed[0] == 1
    assert needed[1:] == [int(w) for w in want["owed"]], (needed, want["owed"])
    return st, log, want


@pytest.mark.parametrize("cid", sorted(CASES))
def test_rule_against_the_restatement(cid):
    kw, blocks, kind, flags = CASES[cid]
    st, log, want = check_against_restatement(options(**kw), blocks)
    assert st.done == kind, (st.done, message(st, options(**kw)))
    assert _flags(log) == flags


@pytest.mark.parametrize("rho,factor", [(0.25, 1.125), (0.5, 1.0), (0.75, 0.875), (1.0, 1.0 / 3.0), (2.0, 1.0 / 3.0)])
@pytest.mark.parametrize("cap", [1e16, 100.0])
def test_radius_after_an_acceptance(rho, factor, cap):
    """StepAccepted: radius / max(1/3, 1 - (2 rho - 1)^3), clamped to max_trust_region_radius."""
    o = options(**dict(TOL0, max_num_iterations=1, initial_trust_region_radius=64.0, max_trust_region_radius=cap))
    st, log, _ = check_against_restatement(o, [blk(8.0, step(8.0 - rho)), blk(8.0 - rho, NONE)])
    assert log[1]["relative_decrease"] == rho and log[1]["step_is_successful"] == 1
    assert st.radius == log[1]["trust_region_radius"] == min(cap, 64.0 / factor)
    assert st.decrease_factor == 2.0


def test_decrease_factor_over_three_rejections():
    kw, blocks, _, _ = CASES["decrease_factor_doubles_and_resets"]
    _, log, _ = check_against_restatement(options(**kw), blocks)
    assert [e["trust_region_radius"] for e in log[:4]] == [64.0, 32.0, 8.0, 1.0]
    assert log[5]["trust_region_radius"] == log[4]["trust_region_radius"] / 2.0


def test_final_gradient_goes_to_the_pending_entry():
    kw, blocks, _, _ = CASES["limit_then_final_gradient"]
    _, log, _ = check_against_restatement(options(**kw), blocks)
    assert [e["gradient_max_norm"] for e in log] == [5.0, 2.0, 0.75]
    assert [e["gradient_norm"] for e in log] == [5.0, 3.0, 1.5]


@pytest.mark.parametrize("max_log", [0, 1, 2, 5])
def test_log_shorter_than_the_solve(max_log):
    """n_log keeps counting past the end of the log; nothing is written beyond it and the solve does not change."""
    kw, blocks, _, flags = CASES["decrease_factor_doubles_and_resets"]
    st, log, want = check_against_restatement(options(**kw), blocks, max_log=max_log)
    assert st.n_log == len(flags) == 6 and len(log) == min(max_log, 6)
    assert _flags(log) == flags[:max_log]


# ---- replay of the oracle ----------------------------------------------------------------------------------------------------------
REPLAYED = [c for c in opts.OPTION_IDS if c != "G_parameter"]      # (the oracle's records hold no |x|: see the module docstring)
INVALID_IDS = [c[0] for c in opts.invalid_cases() if c[2] is not None]
RULE_OPTIONS = ("max_num_iterations", "max_num_consecutive_invalid_steps", "function_tolerance", "gradient_tolerance", "parameter_tolerance",
                "initial_trust_region_radius", "max_trust_region_radius", "min_trust_region_radius", "min_relative_decrease")


@functools.lru_cache(None)
def _option_cases(name):
    return opts._window(name), {c[0]: c for c in opts._cases(name)}


@functools.lru_cache(None)
def _flat_window():
    return opts.flat_camera(opts._window("mild"))[0]


def replay(p, kw):
    """Solves p with the oracle at the options kw, feeds the rules blocks built from the oracle's iteration records and compares."""
    oo = oracle.default_options(**kw)
    ref = oracle.solve(p, oo)
    ref_message = ref["message"].decode() if isinstance(ref["message"], bytes) else ref["message"]
    trace = ref["iterations"]
    if ref_message.startswith(opts.FUNC):
        # the oracle (like Ceres) does not log the iteration that met the tolerance: its record comes from the same solve with the
        # tolerance off, stopped right after it
        more = oracle.solve(p, oracle.default_options(**dict(kw, function_tolerance=0.0, max_num_iterations=len(trace))))["iterations"]
        assert len(more) == len(trace) + 1 and [i["cost"] for i in more[:-1]] == [i["cost"] for i in trace]
        trace = more
    o = options(**{f: getattr(oo, f) for f in RULE_OPTIONS})

    def block(st, grad_only):
        at = max(i for i in range(st.iteration + 1) if trace[i]["step_is_successful"])      # the current point: the last one accepted
        b = dict(cost=trace[at]["cost"], gmax=(0.0, trace[at]["gradient_max_norm"]), gnorm2=(0.0, trace[at]["gradient_norm"] ** 2), step=NONE)
        if not grad_only and st.iteration + 1 < len(trace):      # (else: a speculative step the oracle never took -- NaN, not to be used)
            r = trace[st.iteration + 1]
            solved = 1.0 if r["step_is_valid"] or r["model_cost_change"] != 0.0 else 0.0
            b["step"] = step(r["candidate_cost"], mcc=(0.0, r["model_cost_change"]), step2=(0.0, r["step_norm"] ** 2), x2=(0.0, 0.0), solve_ok=solved)
        return b
    st, log, _, _ = run_rules(o, block, max_log=512)
    its = ref["iterations"]
    assert message(st, o) == ref_message
    assert st.n_log == len(log) == len(its)
    for a, b in zip(log, its):
        assert a["iteration"] == b["iteration"]
        assert (a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]), b["iteration"]
        for f in ("cost", "gradient_max_norm", "model_cost_change"):
            assert a[f] == b[f], (b["iteration"], f, a[f], b[f])
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-12 * b["trust_region_radius"], b["iteration"]
    assert (st.num_successful, st.num_unsuccessful) == (ref["num_successful_steps"], ref["num_unsuccessful_steps"])
    assert (st.initial_cost, st.minimum_cost) == (ref["initial_cost"], ref["final_cost"])
    return ref_message


@pytest.mark.parametrize("cid", REPLAYED)
def test_replay_of_the_oracle_option_case(cid):
    p, cases = _option_cases("plain")
    _, kw, kind = cases[cid]
    assert replay(p, kw).startswith(kind)


@pytest.mark.parametrize("cid", INVALID_IDS)
def test_replay_of_the_oracle_invalid_steps(cid):
    _, kw, kind, _ = {c[0]: c for c in opts.invalid_cases()}[cid]
    assert replay(_flat_window(), kw).startswith(kind)


def test_the_replayed_cases_reach_every_termination():
    kinds = {c[2] for c in _option_cases("plain")[1].values() if c[0] in REPLAYED} | {c[2] for c in opts.invalid_cases() if c[0] in INVALID_IDS}
    assert kinds == {opts.MAX_IT, opts.GRAD, opts.FUNC, opts.MIN_RADIUS, opts.INVALID}
