"""The oracle's trust-region loop at NON-default solver options (include/pba.h pba_solver_options) against an independent dense
numpy Levenberg-Marquardt written from Ceres' documented rules (tests/lm_yardstick.py on the explicit Jacobian): Jacobi scaling on/off, the LM diagonal clamp, the trust-region
radius bounds, the step-quality threshold, the three tolerances set to end the solve partway through, and the invalid-step path
(a singular linear solve) up to max_num_consecutive_invalid_steps.

The windows of the invalid-step cases (flat_camera / flat_point) and the option cases themselves (option_cases) are shared with
tests/test_gpu_solver_options.py, which runs the same cases on every device driver."""
import copy

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import oracle
from photobundle_amd import imgproc, synthetic

import lm_yardstick as lm

TOLERANCES_OFF = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
MAX_IT = "Maximum number of iterations"
GRAD = "Gradient tolerance"
MIN_RADIUS = "Minimum trust region radius"
INVALID = "Number of consecutive invalid steps"
PARAM = "Parameter tolerance"
FUNC = "Function tolerance"


# ---- windows whose steps are invalid on purpose ------------------------------------------------------------------------------------
def _copy_frames(p):
    q = copy.copy(p)
    q.images, q.planes = p.images.copy(), p.planes.copy()
    return q


def flat_camera(p):
    """A free camera whose frame is one constant grey: its Jacobian columns are exactly zero, so with min_lm_diagonal = 0 its rows of
    the reduced camera system are zero and the Cholesky factorisation fails.  Returns (window, slot)."""
    k = max(s for s in range(p.n_frames) if s != p.fixed_slot)
    q = _copy_frames(p)
    q.images[k][:] = 128
    q.planes[k] = imgproc.planes_from_u8(q.images[k])
    return q, k


def _projections(p):
    fx, fy, cx, cy = p.K
    uv = np.zeros((p.n_frames, p.n_points, 2))
    for s in range(p.n_frames):
        Xc = p.xyz @ Rotation.from_rotvec(p.cams[s, :3]).as_matrix().T + p.cams[s, 3:]
        uv[s] = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    return uv


def flat_point(p):
    """A point whose patches are flat in every frame: a constant square of half-width radius + 4 around its projection at the
    initial cameras.  Its point block J_p^T J_p is exactly zero (with min_lm_diagonal = 0 the damped block is not positive
    definite: a Schur elimination failure); every other point keeps a positive-definite block.  Returns (window, point)."""
    uv = _projections(p)
    rows, cols = p.images.shape[1:]
    h = p.radius + 4
    for j in range(p.n_points):
        c = np.rint(uv[:, j]).astype(int)
        if not ((c[:, 0] >= h + 1).all() and (c[:, 0] < cols - h - 1).all() and (c[:, 1] >= h + 1).all() and (c[:, 1] < rows - h - 1).all()):
            continue
        q = _copy_frames(p)
        for s in range(p.n_frames):
            q.images[s][c[s, 1] - h:c[s, 1] + h + 1, c[s, 0] - h:c[s, 0] + h + 1] = 128
            q.planes[s] = imgproc.planes_from_u8(q.images[s])
        V = oracle.linearize(q)["V"]
        others = np.delete(V, j, 0)
        if np.all(V[j] == 0) and np.all(np.linalg.eigvalsh(others) > 0):
            return q, j
    raise AssertionError("no point of the window can be flattened alone")


# ---- the option cases ------------------------------------------------------------------------------------------------------------
def _new_minimum(values, first=2, factor=0.5):
    """(index, threshold): the first entry at or after `first` that is below `factor` x the minimum of the earlier entries, and a
    threshold halfway (geometrically) between the two."""
    m = np.inf
    for i, (k, v) in enumerate(values):
        if i >= first and v < factor * m:
            return k, np.sqrt(v * m)
        m = min(m, v)
    raise AssertionError("the default trace has no clear new minimum to end on: %r" % (values,))


def option_cases(p, ref, n_it):
    """[(case id, solver keywords, termination message prefix)] for the window p; ref = its oracle solve with the tolerances off
    and max_num_iterations = n_it (the mid-solve thresholds are read off that trace)."""
    its = ref["iterations"]
    assert len(its) == n_it + 1, ref["message"]
    x_norm = np.sqrt((np.delete(p.cams, p.fixed_slot, 0) ** 2).sum() + (p.xyz ** 2).sum())
    off = dict(TOLERANCES_OFF, max_num_iterations=n_it)
    short = dict(TOLERANCES_OFF, max_num_iterations=min(n_it, 12))      # the diagonal clamps: a dozen steps are plenty
    g_it, g_tol = _new_minimum([(i["iteration"], i["gradient_max_norm"]) for i in its if i["step_is_successful"]])
    valid = [i for i in its[1:] if i["step_is_valid"]]
    _, p_rel = _new_minimum([(i["iteration"], i["step_norm"] / x_norm) for i in valid])
    _, f_rel = _new_minimum([(i["iteration"], abs(i["cost_change"]) / (i["cost"] if i["step_is_successful"] else i["cost"] - i["cost_change"]))
                                for i in valid])
    grad_mid = dict(max_num_iterations=n_it, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=g_tol)
    return [
        ("A_no_jacobi", dict(off, jacobi_scaling=0), MAX_IT),
        ("B_max_diag", dict(short, max_lm_diagonal=1e-3, initial_trust_region_radius=1e-2), MAX_IT),
        ("B_min_diag", dict(short, min_lm_diagonal=0.5), MAX_IT),
        ("B_no_jacobi_max_diag", dict(short, jacobi_scaling=0, max_lm_diagonal=1e3), MAX_IT),
        ("C_small_radius", dict(off, initial_trust_region_radius=1e-3), MAX_IT),
        ("C_radius_cap", dict(off, initial_trust_region_radius=1e-3, max_trust_region_radius=1e-1), MAX_IT),
        ("D_min_decrease", dict(off, max_num_iterations=min(n_it, 15), min_relative_decrease=0.9), MAX_IT),
        ("E_min_radius", dict(off, max_num_iterations=60, min_trust_region_radius=1e3, min_relative_decrease=0.999), MIN_RADIUS),
        ("E_start_at_min_radius", dict(off, initial_trust_region_radius=1e4, min_trust_region_radius=1e4), MIN_RADIUS),
        ("F_grad_at_zero", dict(off, gradient_tolerance=2.0 * its[0]["gradient_max_norm"]), GRAD),
        # both iteration-zero tests pass: the gradient test comes first
        ("F_grad_before_min_radius", dict(off, gradient_tolerance=2.0 * its[0]["gradient_max_norm"], initial_trust_region_radius=1e4,
                                          min_trust_region_radius=1e4), GRAD),
        ("F_grad_mid", grad_mid, GRAD),
        ("F_grad_at_limit", dict(grad_mid, max_num_iterations=g_it), MAX_IT),
        ("G_parameter", dict(off, parameter_tolerance=p_rel), PARAM),
        ("G_function", dict(off, function_tolerance=f_rel), FUNC),
        ("I_long_limit", dict(grad_mid, max_num_iterations=2000), GRAD),
    ]


def invalid_cases():
    """[(case id, solver keywords, termination message prefix, number of invalid steps logged)] of the flat windows."""
    out = [("H_invalid_%d" % m, dict(min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=m), INVALID, max(m, 1)) for m in (0, 1, 3, 5)]
    out.append(("H_min_radius_wins", dict(min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=10, min_trust_region_radius=1e2),
                MIN_RADIUS, 4))
    out.append(("H_control", dict(max_num_iterations=8), None, 0))
    return out


def check_case_shape(cid, ref, kind, n_it):
    """The case ends where it is meant to: message, and -- for the mid-solve thresholds -- partway through."""
    if kind is not None:
        assert ref["message"].startswith(kind), (cid, ref["message"])
    its = ref["iterations"]
    if cid in ("F_grad_at_zero", "F_grad_before_min_radius", "E_start_at_min_radius"):
        assert len(its) == 1
    if cid in ("F_grad_mid", "G_parameter", "G_function", "E_min_radius"):
        assert 2 < len(its) < n_it, (cid, len(its))
    if cid == "D_min_decrease":
        assert ref["num_unsuccessful_steps"] >= 2
    if cid == "C_radius_cap":
        assert max(i["trust_region_radius"] for i in its) == 1e-1
    if cid == "E_min_radius":
        assert not its[-1]["step_is_successful"]


# ---- the independent dense loop: lm_yardstick's loop on the explicit Jacobian --------------------------------------------------------
KINDS = (MAX_IT, GRAD, MIN_RADIUS, INVALID, PARAM, FUNC)


def compare_with_dense_loop(p, o, ref):
    res = lm.ExplicitJacobian(p).solve(**lm.options_of(o))
    log, cams, xyz = res["iterations"], res["cams"], res["xyz"]
    kind = next(k for k in KINDS if res["message"].startswith(k))
    its = ref["iterations"]
    assert ref["message"].startswith(kind), (kind, ref["message"])
    assert len(its) == len(log), (len(its), len(log), ref["message"])
    for a, b in zip(its, log):
        assert a["iteration"] == b["iteration"]
        assert (a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]), a["iteration"]
        # a rejected entry logs the candidate's cost: an overshooting step, where the cost is first-order sensitive to the step (which
        # the Schur path and the dense solve agree on to ~1e-8, test_oracle_solver.py)
        assert np.isclose(a["cost"], b["cost"], rtol=1e-9 if b["step_is_successful"] or not b["step_is_valid"] else 1e-8), \
            (a["iteration"], a["cost"], b["cost"])
        assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-9), \
            (a["iteration"], a["trust_region_radius"], b["trust_region_radius"])
    assert ref["num_successful_steps"] == sum(b["step_is_successful"] for b in log)
    assert ref["termination_type"] == {INVALID: 2, MAX_IT: 1}.get(kind, 0)
    assert np.abs(ref["cams"] - cams).max() <= 1e-7 and np.allclose(ref["xyz"], xyz, rtol=1e-7, atol=1e-7)
    return log


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
WINDOWS = {
    "plain": dict(n_frames=3, n_points=36, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0), seed_offset=3, rot_deg=0.6, trans=0.05),
    # the flat windows: a mild start, so that a flattened point's projection stays inside its flat square through the solve
    "mild": dict(n_frames=3, n_points=36, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0), seed_offset=3),
    "huber": dict(n_frames=3, n_points=36, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0), seed_offset=3, rot_deg=0.6, trans=0.05,
                  huber=0.05),
}
N_IT = 30


def _window(name):
    return synthetic.make_window(**WINDOWS[name])


def _cases(name):
    p = _window(name)
    return option_cases(p, oracle.solve(p, oracle.default_options(max_num_iterations=N_IT, **TOLERANCES_OFF)), N_IT)


OPTION_IDS = ["A_no_jacobi", "B_max_diag", "B_min_diag", "B_no_jacobi_max_diag", "C_small_radius", "C_radius_cap", "D_min_decrease",
              "E_min_radius", "E_start_at_min_radius", "F_grad_at_zero", "F_grad_before_min_radius", "F_grad_mid", "F_grad_at_limit", "G_parameter", "G_function",
              "I_long_limit"]


# the Huber window runs the cases whose path the loss changes
@pytest.mark.parametrize("name,cid", [("plain", c) for c in OPTION_IDS] + [("huber", c) for c in ("A_no_jacobi", "D_min_decrease",
                                                                                               "F_grad_mid", "G_parameter", "G_function")])
def test_option_case_against_the_dense_loop(name, cid):
    p = _window(name)
    cases = {c[0]: c for c in _cases(name)}
    assert sorted(cases) == sorted(OPTION_IDS)
    _, kw, kind = cases[cid]
    o = oracle.default_options(**kw)
    ref = oracle.solve(p, o)
    check_case_shape(cid, ref, kind, kw["max_num_iterations"])
    compare_with_dense_loop(p, o, ref)
    if cid == "I_long_limit":
        short = oracle.solve(p, oracle.default_options(**dict(kw, max_num_iterations=500)))
        assert [i["cost"] for i in short["iterations"]] == [i["cost"] for i in ref["iterations"]] and short["message"] == ref["message"]


@pytest.mark.parametrize("flat", ["camera", "point"])
@pytest.mark.parametrize("k", range(len(invalid_cases())))
def test_invalid_steps_against_the_dense_loop(flat, k):
    cid, kw, kind, n_invalid = invalid_cases()[k]
    q, idx = (flat_camera if flat == "camera" else flat_point)(_window("mild"))
    o = oracle.default_options(**kw)
    ref = oracle.solve(q, o)
    log = compare_with_dense_loop(q, o, ref)
    its = ref["iterations"]
    if kind is not None:
        assert ref["message"].startswith(kind), ref["message"]
        assert len(its) == 1 + n_invalid and all(i["step_is_valid"] == 0 for i in its[1:])
        radii = [1e4 / 2.0 ** (m * (m + 1) // 2) for m in range(n_invalid)]
        if kind == INVALID:
            radii.append(radii[-1])    # the terminating step is logged before any damping change
        else:
            radii = radii[:1] + [1e4 / 2.0 ** (m * (m + 1) // 2) for m in range(1, n_invalid + 1)]
        assert [i["trust_region_radius"] for i in its] == radii
        assert ref["termination_type"] == (2 if kind == INVALID else 0)
        assert ref["final_cost"] == ref["initial_cost"]
        assert np.array_equal(ref["cams"], q.cams) and np.array_equal(ref["xyz"], q.xyz)
    else:
        # the control: the default clamp makes every step valid and the zero-Jacobian block does not move, to the bit
        assert all(i["step_is_valid"] for i in its) and ref["num_successful_steps"] > 2
        moved = ref["cams"][idx] if flat == "camera" else ref["xyz"][idx]
        assert np.array_equal(moved, q.cams[idx] if flat == "camera" else q.xyz[idx])
    assert len(log) == len(its)
