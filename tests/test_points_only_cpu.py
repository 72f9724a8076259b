"""Structure-only solves (pba_set_cameras_constant) without a device: the numpy yardstick tests/lm_yardstick.py (PointBlocks) against two
independent routes (dense point-only normal equations from per-block oracle products; scipy.optimize.least_squares over the same 3 n
parameters), the qualification of the device trace cases on the yardstick alone, and the ABI / Python / host plumbing of the mode."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic

import lm_yardstick as lm
import points_only_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("huber", [0.0, 0.05])
def test_first_step_equals_the_dense_point_only_normal_equations(huber):
    p = cases.cameras_to_ground_truth(synthetic.make_window(n_frames=3, n_points=40, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0),
                                                          huber=huber, seed_offset=1))
    st = lm.PointBlocks(p).first_step(radius=1e4)
    # a second route: per-block products of the corrected rows, summed into ONE dense 3 n x 3 n system and solved densely
    bp = oracle.block_products(p, cams=p.cams, xyz=p.xyz)
    n = 3 * p.n_points
    H, g = np.zeros((n, n)), np.zeros(n)
    for o in range(p.n_obs):
        k = 3 * int(p.obs_point[o])
        H[k:k + 3, k:k + 3] += bp["JpJp"][o]
        g[k:k + 3] += bp["Jpr"][o]
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    Hs = H * scale[:, None] * scale[None, :]
    gs = g * scale
    D2 = np.clip(np.diag(Hs), 1e-6, 1e32) / 1e4
    A = Hs + np.diag(D2)
    y = np.linalg.solve(A, gs)
    S = np.zeros((n, n))
    for k in range(p.n_points):
        S[3 * k:3 * k + 3, 3 * k:3 * k + 3] = st["S"][k]
    tol = 1e-10
    assert np.abs(S - A).max() <= tol * np.abs(A).max()
    assert np.abs(st["rhs"].ravel() - gs).max() <= tol * np.abs(gs).max()
    assert np.abs(st["delta"].ravel() + y * scale).max() <= tol * np.abs(y * scale).max()
    assert np.isclose(st["model_cost_change"], float(y @ gs - 0.5 * y @ Hs @ y), rtol=tol)
    assert np.abs(st["gradient"].ravel() - g).max() <= tol * np.abs(g).max()
    assert st["linear_solver_ok"]
    sq = oracle.linearize(p, cams=p.cams, blocks=False)["block_sqnorm"]
    assert np.isclose(st["cost"], lm.block_costs(p, sq).sum(), rtol=1e-14)


def _scipy_problem(seed):
    from test_oracle_scipy_minimum import _Restatement
    p = cases.cameras_to_ground_truth(synthetic.make_window(n_frames=3, n_points=30, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0),
                                                          rot_deg=0.05, trans=0.01, depth_noise=0.005, seed_offset=seed))
    rs = _Restatement(p)
    n_cam = rs.n_cam
    tc = rs.pack(p.cams, p.xyz)[:n_cam]

    def residuals(x):
        return rs.residuals(np.concatenate([tc, x]))

    def jacobian(x):
        return rs.jacobian(np.concatenate([tc, x]))[:, n_cam:]

    res = lm.PointBlocks(p).solve(max_num_iterations=400, function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14)
    return p, rs, residuals, jacobian, res


@pytest.mark.parametrize("seed", [3, 8, 5, 1])
def test_scipy_from_the_common_start_ends_in_the_same_basin(seed):
    """An independent trust-region loop over the same 3 n point parameters (cameras constant), from the same start, in the form of the
    pose-only twin and of test_oracle_scipy_minimum.py: the surface is piecewise (texel cells, float-rounded coordinates), both loops stop
    where their trust region has shrunk below a float ulp of (u, v), so what can be asserted is the same basin.  Here the parameters
    are the points themselves and nothing ties one point to another, so a single point that settles in a neighbouring cell shifts the
    cost by a per cent.  Measured, (scipy - yardstick) / yardstick: +9.1 % (seed 3, where scipy stops early and the yardstick ends LOWER),
    -0.38 % (seed 8), -0.54 % (seed 5), -0.95 % (seed 1).  The bound is the twin's 5 %, held one-sided because the subject is the
    yardstick: it must not end more than 5 % above what the independent loop reaches (a loop that reaches less says nothing against it);
    both loops descend; and the median point lands within 0.1 px of the same place in every frame, the twin's bound."""
    pytest.importorskip("scipy")
    from scipy.optimize import least_squares
    p, rs, residuals, jacobian, res = _scipy_problem(seed)
    sp = least_squares(residuals, p.xyz.ravel(), jac=jacobian, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                       max_nfev=2000)
    rel = (sp.cost - res["final_cost"]) / res["final_cost"]
    _, _, _, u1, v1 = rs._geometry(p.cams, sp.x.reshape(-1, 3))
    _, _, _, u2, v2 = rs._geometry(p.cams, res["xyz"])
    px = float(np.median(np.hypot(u1 - u2, v1 - v2)))
    print("seed %d: start %.6e  yardstick %.6e  scipy %.6e  relative %.2e  median distance %.3f px" % (seed, res["initial_cost"],
                                                                                                        res["final_cost"], sp.cost, rel, px))
    assert res["final_cost"] < res["initial_cost"] and sp.cost < res["initial_cost"]
    assert res["final_cost"] <= 1.05 * sp.cost
    assert px < 0.1


@pytest.mark.parametrize("seed", [5, 1])
def test_yardstick_end_point_is_stationary_for_scipy(seed):
    """Stationarity, not agreement of two loops: least_squares STARTED at the yardstick's end point finds nothing further to gain, to
    1e-6 of the cost (measured 8.7e-9 on seed 5, 5.2e-9 on seed 1).  On seeds 3 and 8 scipy still finds a lower texel cell next to the
    end point (1.6e-5, 3.3e-6), which is the piecewise surface again and why those two are not held to this bar."""
    pytest.importorskip("scipy")
    from scipy.optimize import least_squares
    p, rs, residuals, jacobian, res = _scipy_problem(seed)
    assert res["final_cost"] < res["initial_cost"]
    restated = 0.5 * float(np.sum(residuals(res["xyz"].ravel()) ** 2))
    assert restated == pytest.approx(res["final_cost"], rel=1e-6)
    sp = least_squares(residuals, res["xyz"].ravel(), jac=jacobian, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                       max_nfev=2000)
    print("yardstick %.12e  scipy %.12e  (%s)" % (res["final_cost"], sp.cost, res["message"]))
    assert np.isclose(sp.cost, res["final_cost"], rtol=1e-6)


@pytest.fixture(scope="module")
def trace_runs():
    """The yardstick on every trace case, on autodiff evaluations: (problem, extras, rays, rho, result, compared iterations)."""
    out = {}
    for name in cases.TRACE_CASES:
        p, extras, rays, rho = cases.trace_case(name)
        res = lm.PointBlocks(p, rays, rho).solve(max_num_iterations=cases.REF_ITERATIONS)
        out[name] = (p, extras, rays, rho, res, lm.compared_iterations(res))
    return out


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_cases_have_four_clear_iterations(trace_runs, name):
    """The condition of the device trace test (tests/test_gpu_points_only.py), on the yardstick alone."""
    res, n_cmp = trace_runs[name][4:]
    assert n_cmp >= 4, [(i["step_is_successful"], i["relative_decrease"]) for i in res["iterations"]]


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_cases_qualify(trace_runs, name):
    """A case qualifies for the device comparison when the yardstick itself is insensitive to how the derivatives are evaluated: run
    on analytic evaluations it takes the same decisions and ends the compared iterations within 1e-6 (a tenth of the device bar) of the
    run on autodiff evaluations, in the parameters the program optimises (inverse depths in that case: a far point's world position
    amplifies its inverse depth by depth^2).  The single-observation case is held to cost and decisions only: its rank-2 blocks leave
    one direction per point to the damping alone."""
    p, extras, rays, rho, res, n_cmp = trace_runs[name]
    ana = lm.PointBlocks(p, rays, rho, autodiff=False).solve(max_num_iterations=n_cmp - 1)
    a, b = res["iterations"][:n_cmp], ana["iterations"]
    assert len(b) == n_cmp
    assert [i["step_is_successful"] for i in a] == [i["step_is_successful"] for i in b]
    assert [i["step_is_valid"] for i in a] == [i["step_is_valid"] for i in b]
    assert np.allclose([i["cost"] for i in a], [i["cost"] for i in b], rtol=1e-9, atol=0.0)
    if "single-observation" not in extras:
        diff = np.abs(res["states"][n_cmp - 1] - ana["x"]).max()
        print(name, "autodiff against analytic after %d iterations: %.3e" % (n_cmp - 1, diff))
        assert diff <= 1e-6
    if rays is not None:      # every evaluated candidate stays inside the domain of the parameterisation (inverse depths > 0)
        assert res["min_candidate"] > 0.0 and ana["min_candidate"] > 0.0


def test_the_wide_case_holds_a_point_seen_once_and_one_seen_by_every_frame():
    p, _, _, _ = cases.trace_case("20-frames-r1-causal")
    count = np.bincount(p.obs_point, minlength=p.n_points)
    assert count.min() == 1 and count.max() == 20 and p.n_frames == 20


def test_a_rejecting_start_exists_on_the_yardstick():
    """The device test of rejected steps starts from a radius the yardstick rejects at least once."""
    p, _, rays, rho = cases.trace_case("3-frames-r1-huber")
    res = lm.PointBlocks(p, rays, rho).solve(max_num_iterations=6, initial_trust_region_radius=1e12)
    assert any(i["step_is_valid"] and not i["step_is_successful"] for i in res["iterations"][1:])


# ---- ABI and plumbing without a device ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_reject_a_null_engine():
    import subprocess
    from photobundle_amd import _lib
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("pba_set_cameras_constant", "pba_get_point_system"):
        assert name in _lib.SYMBOLS
        assert (" T " + name + "\n") in nm
    assert L.pba_set_cameras_constant(None, 1) == -1      # PBA_ERR_INVALID
    assert L.pba_get_point_system(None, None, None) == -1


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "pba.h")) as f:
        text = f.read()
    assert "int pba_set_cameras_constant(pba_engine* e, int32_t on);" in text
    assert "int pba_get_point_system(pba_engine* e, double* V9, double* rhs3);" in text


def test_python_wrappers_exist():
    from photobundle_amd.engine import Engine
    assert callable(getattr(Engine, "set_cameras_constant")) and callable(getattr(Engine, "point_system"))


def test_host_header_compiles_with_the_option(tmp_path):
    import host_class_probe
    probe = host_class_probe.HostClassProbe(tmp_path)
    for name in ("probe_create", "probe_add", "probe_print_options", "probe_release"):
        assert hasattr(probe.L, name)
    assert "camerasConstant = 1\n" in probe.print_options(cameras_constant=True)
    assert "camerasConstant = 0\n" in probe.print_options(cameras_constant=False)


def test_run_kitti_accepts_the_key_up_to_the_device(tmp_path):
    import subprocess
    import host_class_probe
    run = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    assert os.path.exists(run), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    img = np.zeros((32, 48), np.uint8)
    host_class_probe.write_sequence(str(tmp_path), [img], [np.ones((32, 48), np.float32)], (50.0, 50.0, 24.0, 16.0), [np.eye(4)])

    def go(extra):
        cfg = os.path.join(str(tmp_path), "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\n%s" % (tmp_path, tmp_path, extra))
        # (HIP_VISIBLE_DEVICES hides every device: the run ends where it first needs one)
        return subprocess.run([run, "-c", cfg, "-o", os.path.join(str(tmp_path), "out.txt")], capture_output=True, text=True, timeout=120,
                              env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))

    with_key, without = go("camerasConstant = 1\n"), go("")
    # the key changes nothing before the device is needed: both runs end at the same place, creating the engine
    assert with_key.returncode == without.returncode == 1
    assert "pba_create" in with_key.stderr and "pba_create" in without.stderr
    assert "camerasConstant" not in with_key.stderr
