"""Anchor frames (pba_set_cameras_anchored) without a device: the numpy yardstick tests/lm_yardstick.py (Dense) against the oracle's own solver
(one constant slot) and against scipy.optimize.least_squares (two and three), the qualification of the device trace cases on the
yardstick alone, the slot rule of photobundle_amd/csrc/pba_slot_rule.h compiled stand-alone, and the ABI / Python / host plumbing."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic

import anchors_cases as cases
import lm_yardstick as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_IT = "Maximum number of iterations"
INVALID = "Number of consecutive invalid steps"
KINDS = (MAX_IT, INVALID, "Gradient tolerance", "Minimum trust region radius", "Parameter tolerance", "Function tolerance")


# ---- one constant slot: the oracle's own trace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed_slot,huber", [(0, 0.0), (1, 0.05), (2, 0.0)])
def test_one_slot_set_reproduces_the_oracle_trace(fixed_slot, huber):
    """The assertions of test_oracle_solver_options.py::compare_with_dense_loop, with the yardstick in the dense loop's place."""
    p = synthetic.make_window(n_frames=3, n_points=40, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0), huber=huber, seed_offset=1)
    p.fixed_slot = fixed_slot
    n_it = 12
    res_o = oracle.solve(p, oracle.default_options(max_num_iterations=n_it))
    res = lm.Dense(p, (fixed_slot,)).solve(max_num_iterations=n_it)
    its, log = res_o["iterations"], res["iterations"]
    kind = next(k for k in KINDS if res["message"].startswith(k))
    assert res_o["message"].startswith(kind), (res["message"], res_o["message"])
    assert len(its) == len(log), (len(its), len(log), res_o["message"], res["message"])
    for a, b in zip(its, log):
        assert a["iteration"] == b["iteration"]
        assert (a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]), a["iteration"]
        # a rejected entry logs the candidate's cost: an overshooting step, where the cost is first-order sensitive to the step (which
        # the Schur path and the dense solve agree on to ~1e-8, test_oracle_solver.py)
        assert np.isclose(a["cost"], b["cost"], rtol=1e-9 if b["step_is_successful"] or not b["step_is_valid"] else 1e-8), \
            (a["iteration"], a["cost"], b["cost"])
        assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-9), a["iteration"]
    assert res_o["num_successful_steps"] == sum(b["step_is_successful"] for b in log)
    assert res_o["termination_type"] == {INVALID: 2, MAX_IT: 1}.get(kind, 0)
    assert np.abs(res_o["cams"] - res["cams"]).max() <= 1e-7 and np.allclose(res_o["xyz"], res["xyz"], rtol=1e-7, atol=1e-7)
    assert np.array_equal(res["cams"][fixed_slot], p.cams[fixed_slot])


def test_first_step_reduced_system_equals_the_dense_reference_step():
    """first_step()'s Schur elimination against tests/gpu_util.py's reference_step (dense Jacobian from per-block rows), one slot."""
    from gpu_util import dense_system, reference_step
    p = synthetic.make_window(n_frames=3, n_points=40, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0), huber=0.05, seed_offset=1)
    st = lm.Dense(p, (p.fixed_slot,)).first_step()
    J, r, n_cam = dense_system(p)
    rs = reference_step(J, r, n_cam, 1e4)
    assert n_cam == st["n_cam"]
    assert np.abs(st["S"] - rs["S"]).max() <= 1e-9 * np.abs(rs["S"]).max()
    assert np.abs(st["rhs"] - rs["rhs"]).max() <= 1e-9 * np.abs(rs["rhs"]).max()
    assert np.isclose(st["model_cost_change"], rs["model_cost_change"], rtol=1e-8)
    assert np.allclose(np.concatenate([st["delta_c"].ravel(), st["delta_p"].ravel()]), rs["delta"], rtol=1e-6, atol=1e-12)


# ---- two and three anchors: a third-party trust-region loop over the same free columns -----------------------------------------------
@pytest.mark.parametrize("n_frames,slots,seed", [(3, (0, 2), 3), (4, (1, 3), 8), (5, (0, 1, 2), 5)])
def test_end_point_matches_scipy_least_squares_over_the_free_columns(n_frames, slots, seed):
    """The bar of test_pose_only_cpu.py / test_points_only_cpu.py for this comparison: both loops descend, the costs are 5 % apart at
    the most, the median point lands within 0.1 px of the same place in every frame; the anchored cameras do not move.  The 5 % are
    held one-sided, as test_points_only_cpu.py holds them and for its reason: the subject is the yardstick, it must not end more than
    5 % above what the independent loop reaches, and a loop that stops earlier (scipy ends on its xtol after 6-10 Jacobians) says
    nothing against it.  Measured, (scipy - yardstick) / yardstick: +7.8 % (anchors {0, 2}), -0.6 % ({1, 3}), +5.3 % ({0, 1, 2})."""
    pytest.importorskip("scipy")
    from scipy.optimize import least_squares
    from test_oracle_scipy_minimum import _Restatement
    p = synthetic.make_window(n_frames=n_frames, n_points=60, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0),
                              rot_deg=0.05, trans=0.01, depth_noise=0.005, seed_offset=seed)
    rs = _Restatement(p)
    rs.free = lm.free_slots(p, slots)                    # the restatement's camera columns: the slots outside the set
    rs.col = {s: 6 * k for k, s in enumerate(rs.free)}
    rs.n_cam = 6 * len(rs.free)
    theta0 = rs.pack(p.cams, p.xyz)
    res = lm.Dense(p, slots).solve(max_num_iterations=400, function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14)
    sp = least_squares(rs.residuals, theta0, jac=rs.jacobian, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                       max_nfev=2000)
    print("anchors %s: start %.6e  yardstick %.6e  scipy %.6e" % (slots, res["initial_cost"], res["final_cost"], sp.cost))
    assert res["final_cost"] < res["initial_cost"] and sp.cost < res["initial_cost"]
    assert res["final_cost"] <= 1.05 * sp.cost, (sp.cost, res["final_cost"], res["message"])
    cs, xs = rs.unpack(sp.x)
    _, _, _, u1, v1 = rs._geometry(cs, xs)
    _, _, _, u2, v2 = rs._geometry(res["cams"], res["xyz"])
    assert np.median(np.hypot(u1 - u2, v1 - v2)) < 0.1
    for s in slots:
        assert np.array_equal(res["cams"][s], p.cams[s]) and np.array_equal(cs[s], p.cams[s])


# ---- qualification of the device trace cases ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trace_runs():
    """The yardstick on every trace case, on autodiff evaluations: (problem, slots, extras, rays, rho, result, compared iterations)."""
    out = {}
    for name in cases.TRACE_CASES:
        p, slots, extras, rays, rho = cases.trace_case(name)
        res = lm.Dense(p, slots, rays, rho).solve(max_num_iterations=cases.REF_ITERATIONS)
        out[name] = (p, slots, extras, rays, rho, res, lm.compared_iterations(res))
    return out


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_cases_have_four_clear_iterations(trace_runs, name):
    res, n_cmp = trace_runs[name][5:]
    assert n_cmp >= 4, [(i["step_is_successful"], i["relative_decrease"]) for i in res["iterations"]]


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_cases_qualify(trace_runs, name):
    """As test_points_only_cpu.py qualifies its cases: run on analytic evaluations the yardstick takes the same decisions and ends the
    compared iterations within 1e-6 of the run on autodiff evaluations, in the parameters the program optimises."""
    p, slots, extras, rays, rho, res, n_cmp = trace_runs[name]
    ana = lm.Dense(p, slots, rays, rho, autodiff=False).solve(max_num_iterations=n_cmp - 1)
    a, b = res["iterations"][:n_cmp], ana["iterations"]
    assert len(b) == n_cmp
    assert [i["step_is_successful"] for i in a] == [i["step_is_successful"] for i in b]
    assert [i["step_is_valid"] for i in a] == [i["step_is_valid"] for i in b]
    assert np.allclose([i["cost"] for i in a], [i["cost"] for i in b], rtol=1e-9, atol=0.0)
    cams_a, x_a = res["states"][n_cmp - 1]
    diff = max(np.abs(cams_a - ana["cams"]).max(), np.abs(x_a - ana["x"]).max())
    print(name, "autodiff against analytic after %d iterations: %.3e" % (n_cmp - 1, diff))
    assert diff <= cases.QUALIFY_BAR
    for s in slots:
        assert np.array_equal(res["cams"][s], p.cams[s])
    if rays is not None:      # every evaluated candidate stays inside the domain of the parameterisation (inverse depths > 0)
        assert res["min_candidate"] > 0.0 and ana["min_candidate"] > 0.0


def test_traces_hold_both_kinds_of_decision():
    """From the default radius the four windows accept and reject: the device traces are compared on both kinds."""
    kinds = set()
    for name in sorted(cases.TRACE_CASES):
        p, slots, extras, rays, rho = cases.trace_case(name)
        if rays is not None:
            continue
        res = lm.Dense(p, slots).solve(max_num_iterations=40)
        its = res["iterations"][1:]
        print(name, "log entries %d, rejected %d (%s)" % (len(res["iterations"]), sum(not i["step_is_successful"] for i in its), res["message"]))
        kinds |= {bool(i["step_is_successful"]) for i in its}
    assert kinds == {True, False}


def test_two_anchors_close_the_gauge():
    """The undamped reduced camera system: singular with one constant slot (the scale of the window is free), well conditioned with
    two -- the table of DESIGN.md, on the 3 x 40 dense window."""
    p, _, _, _, _ = cases.trace_case("3x40-dense-r1-anchors-0-2")

    def cond(slots):
        prog = lm.Dense(p, slots)
        H, n_cam = prog.linearize((np.array(p.cams), np.array(p.xyz)))["H"], prog.n_cam
        S = H[:n_cam, :n_cam] - H[:n_cam, n_cam:] @ np.linalg.solve(H[n_cam:, n_cam:], H[n_cam:, :n_cam])
        w = np.linalg.eigvalsh(0.5 * (S + S.T))
        return abs(w).max() / max(abs(w).min(), 1e-300)

    c1, c2 = cond((0,)), cond((0, 2))
    print("cond(S) undamped: one constant slot %.3e, two %.3e" % (c1, c2))
    assert c1 > 1e10 and c2 < 1e7


def _pose_costs(p, slots):
    """Pose-only mode: (cost of the anchored cameras' residual blocks, cost of the program = every other block, number of program
    blocks)."""
    st = lm.CameraBlocks(p, slots).first_step()
    return st["fixed_cost"], st["cost"], st["num_residual_blocks"]


def test_pose_only_fixed_cost_sums_the_anchored_blocks():
    p = synthetic.make_window(n_frames=5, n_points=60, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0), huber=0.05)
    fixed, prog, n_prog = _pose_costs(p, (0, 3))
    total = oracle.cost(p)[0]
    assert np.isclose(fixed + prog, total, rtol=1e-13)
    assert n_prog == int(np.sum((p.obs_slot != 0) & (p.obs_slot != 3)))
    f0, _, _ = _pose_costs(p, (0,))
    f3, _, _ = _pose_costs(p, (3,))
    assert fixed == f0 + f3


# ---- the slot rule, compiled stand-alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slot_rule(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("slot_rule")), "slot_rule_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "slot_rule_probe.cpp")])

    def run(lines):
        r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True, timeout=60)
        return r.stdout.splitlines()
    return run


def _python_rule(mask, n):
    """[number of free slots, is_free(0), free_index(0), is_free(1), ...]: free index = slot - popcount of the mask below the slot."""
    out = [n - bin(mask & ((1 << n) - 1)).count("1")]
    for c in range(n):
        anchored = (mask >> c) & 1
        out += [0 if anchored else 1, -1 if anchored else c - bin(mask & ((1 << c) - 1)).count("1")]
    return out


def test_slot_rule_equals_the_popcount_rule(slot_rule):
    cases = [(m, n) for n in range(1, 9) for m in range(1 << n)]
    rng = np.random.default_rng(20240607)
    cases += [(int(m), 32) for m in rng.integers(0, 1 << 32, size=1000, dtype=np.uint64)]
    cases += [(0, 32), (0xffffffff, 32), (0x80000000, 32), (0x7fffffff, 32)]
    got = slot_rule(["%x %d\n" % c for c in cases])
    assert len(got) == len(cases)
    for (m, n), line in zip(cases, got):
        assert [int(v) for v in line.split()] == _python_rule(m, n), (hex(m), n)


def test_slot_rule_equals_the_old_fixed_slot_formula(slot_rule):
    """Every one-bit and empty mask at 2 .. 32 slots against the formula pba_set_cameras(fixed_slot) used to hand the kernels."""
    cases = [(n, f) for n in range(2, 33) for f in range(-1, n)]
    masks = [int(v, 16) for v in slot_rule(["@ %d\n" % f for _, f in cases])]
    assert masks == [0 if f < 0 else 1 << f for _, f in cases]
    got = slot_rule(["%x %d\n" % (m, n) for m, (n, _) in zip(masks, cases)])
    for (n, f), line in zip(cases, got):
        old = [n - (1 if f >= 0 else 0)]
        for c in range(n):
            old += [int(c != f), -1 if c == f else (c - 1 if f >= 0 and c > f else c)]
        assert [int(v) for v in line.split()] == old, (n, f)


# ---- ABI and plumbing without a device ------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_rejects_a_null_engine():
    from photobundle_amd import _lib
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pba_set_cameras_anchored" in _lib.SYMBOLS
    assert " T pba_set_cameras_anchored\n" in nm
    assert L.pba_set_cameras_anchored(None, None, 3, 1) == -1      # PBA_ERR_INVALID


def test_header_declares_the_call():
    with open(os.path.join(ROOT, "include", "pba.h")) as f:
        text = f.read()
    assert "int pba_set_cameras_anchored(pba_engine* e, const double* cams6, int32_t n_frames, uint32_t anchor_mask);" in text


def test_python_wrapper_takes_constant_slots():
    import inspect
    from photobundle_amd.engine import Engine
    sig = inspect.signature(Engine.set_cameras)
    assert list(sig.parameters) == ["self", "cams", "fixed_slot", "constant_slots"]
    assert sig.parameters["fixed_slot"].default == 0 and sig.parameters["constant_slots"].default is None


def test_class_header_has_the_option(tmp_path):
    import host_class_probe
    with open(os.path.join(ROOT, "photobundle_amd", "host", "photobundle.h")) as f:
        assert "int numConstantFrames = 1;" in f.read()
    probe = host_class_probe.HostClassProbe(tmp_path)
    assert probe.default_num_constant() == 1
    assert "numConstantFrames = 3\n" in probe.print_options(num_constant=3)
    # outside 1 .. slidingWindowSize - 1: refused when the class is constructed, before a device is asked for
    for levels in (1, 2):
        for k in (0, 5, 7):
            with pytest.raises(RuntimeError, match="numConstantFrames = %d is outside 1 .. slidingWindowSize - 1 = 4" % k):
                probe.create(levels, (32, 48), (50.0, 50.0, 24.0, 16.0), window=5, radius=1, num_constant=k)


def _run_kitti(args):
    run = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    assert os.path.exists(run), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    # (HIP_VISIBLE_DEVICES hides every device: whatever is refused here is refused before any device call)
    return subprocess.run([run] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def _tiny_sequence(tmp, extra):
    import host_class_probe
    img = np.zeros((32, 48), np.uint8)
    host_class_probe.write_sequence(str(tmp), [img], [np.ones((32, 48), np.float32)], (50.0, 50.0, 24.0, 16.0), [np.eye(4)])
    cfg = os.path.join(str(tmp), "test.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\nslidingWindowSize = 4\n%s" % (tmp, tmp, extra))
    return cfg


@pytest.mark.parametrize("k", [0, 4])
@pytest.mark.parametrize("batch", [False, True])
def test_run_kitti_refuses_a_value_outside_the_window(tmp_path, k, batch):
    cfg = _tiny_sequence(tmp_path, "numConstantFrames = %d\n" % k)
    out = os.path.join(str(tmp_path), "out.txt")
    r = _run_kitti(["-b", "%s:%s" % (cfg, out)] if batch else ["-c", cfg, "-o", out])
    assert r.returncode == 1
    assert "numConstantFrames = %d is outside 1 .. slidingWindowSize - 1 = 3" % k in r.stderr
    assert "pba_create" not in r.stderr


def test_run_kitti_accepts_the_key_up_to_the_device(tmp_path):
    cfg = _tiny_sequence(tmp_path, "numConstantFrames = 2\n")
    r = _run_kitti(["-c", cfg, "-o", os.path.join(str(tmp_path), "out.txt")])
    assert r.returncode == 1 and "pba_create" in r.stderr and "numConstantFrames" not in r.stderr
