"""Pose-only solves (pba_set_points_constant) without a device: the numpy yardstick tests/lm_yardstick.py (CameraBlocks) against two independent
routes (dense camera-only normal equations from per-block oracle rows; scipy.optimize.least_squares over the same 6 k parameters),
the tracking bar on the yardstick itself, and the ABI / Python plumbing of the mode."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic

import lm_yardstick as lm
import pose_only_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense_camera_system(p, cols):
    """Loss-corrected Jacobian over the camera columns of the program + residual, from oracle.eval_block rows (a second route: the
    yardstick takes oracle.linearize's block sums)."""
    P = p.patch_len * p.channels
    col = {c: 6 * i for i, c in enumerate(cols)}
    rows_J, rows_r = [], []
    for o in range(p.n_obs):
        c = int(p.obs_slot[o])
        if c not in col:
            continue
        rb, jc, _ = oracle.eval_block(p, o)
        s = rb @ rb
        k = np.sqrt(p.huber / np.sqrt(s)) if (p.huber > 0 and s > p.huber ** 2) else 1.0
        J = np.zeros((P, 6 * len(cols)))
        J[:, col[c]:col[c] + 6] = k * jc
        rows_J.append(J)
        rows_r.append(k * rb)
    return np.concatenate(rows_J), np.concatenate(rows_r)


@pytest.mark.parametrize("huber,fixed_slot", [(0.0, 0), (0.05, 0), (0.05, -1), (0.05, 1)])
def test_first_step_equals_the_dense_camera_only_normal_equations(huber, fixed_slot):
    p = synthetic.make_window(n_frames=3, n_points=40, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0), huber=huber, seed_offset=1)
    p.fixed_slot = fixed_slot
    st = lm.CameraBlocks(p).first_step(radius=1e4)
    cols = st["cols"]
    assert cols == [c for c in range(3) if c != fixed_slot]
    J, r = _dense_camera_system(p, cols)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    H = Js.T @ Js + np.diag(np.clip((Js * Js).sum(0), 1e-6, 1e32) / 1e4)
    y = np.linalg.solve(H, Js.T @ r)
    model = Js @ (-y)
    n = 6 * len(cols)
    S = np.zeros((n, n))
    for k in range(len(cols)):
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = st["S"][k]
    assert np.allclose(S, H, rtol=1e-8, atol=1e-8 * np.abs(H).max())            # block diagonal: the off-diagonal blocks of H vanish
    assert np.allclose(st["rhs"].ravel(), Js.T @ r, rtol=1e-8, atol=1e-8 * np.abs(Js.T @ r).max())
    assert np.allclose(st["delta"].ravel(), -y * scale, rtol=1e-8, atol=1e-8 * np.abs(y * scale).max())
    assert np.isclose(st["model_cost_change"], -model @ (r + model / 2), rtol=1e-8)
    if huber == 0:
        assert np.isclose(st["cost"], 0.5 * float(r @ r), rtol=1e-12)
    assert np.allclose(st["gradient"].ravel(), J.T @ r, rtol=1e-8, atol=1e-8 * np.abs(J.T @ r).max())
    # fixed cost: the loss-corrected cost of the constant camera's residual blocks
    sq = oracle.linearize(p, blocks=False)["block_sqnorm"]
    c = lm.block_costs(p, sq)
    assert np.isclose(st["fixed_cost"], c[p.obs_slot == fixed_slot].sum(), rtol=1e-14)
    assert np.isclose(st["cost"] + st["fixed_cost"], c.sum(), rtol=1e-13)


def test_end_point_matches_scipy_least_squares_over_the_cameras():
    """The yardstick's end point against a third-party trust-region loop over the same 6 k camera parameters, the way
    test_oracle_scipy_minimum.py compares the full problem: same basin, costs within 5 %, re-projections within 0.1 px (median)."""
    pytest.importorskip("scipy")
    from scipy.optimize import least_squares
    from test_oracle_scipy_minimum import _Restatement, _window
    p = _window(3)
    rs = _Restatement(p)
    n_cam = rs.n_cam
    xyz = p.xyz.ravel()

    def residuals(tc):
        return rs.residuals(np.concatenate([tc, xyz]))

    def jacobian(tc):
        return rs.jacobian(np.concatenate([tc, xyz]))[:, :n_cam]

    theta0 = rs.pack(p.cams, p.xyz)[:n_cam]
    res = lm.CameraBlocks(p).solve(max_num_iterations=400, function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14)
    sp = least_squares(residuals, theta0, jac=jacobian, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    full_sp = sp.cost      # scipy's residual vector holds every block, the constant camera's included (like final_cost)
    assert res["final_cost"] < res["initial_cost"] and full_sp < res["initial_cost"]
    assert abs(full_sp - res["final_cost"]) <= 0.05 * res["final_cost"], (full_sp, res["final_cost"], res["message"])
    cs, _ = rs.unpack(np.concatenate([sp.x, xyz]))
    _, _, _, u1, v1 = rs._geometry(cs, p.xyz)
    _, _, _, u2, v2 = rs._geometry(res["cams"], p.xyz)
    assert np.median(np.hypot(u1 - u2, v1 - v2)) < 0.1
    assert np.array_equal(res["cams"][p.fixed_slot], p.cams[p.fixed_slot])


@pytest.mark.parametrize("start", ["velocity", "zero"])
@pytest.mark.parametrize("shape", sorted(cases.TRACKING_SHAPES))
def test_tracking_bar_on_the_yardstick(shape, start):
    """The last frame of a 5-frame window tracked against the window's points, from the constant-velocity prediction and from zero
    motion: the yardstick ends within 0.02 m and 0.1 degree of the ground truth (one sigma of make_window's trans / rot_deg
    defaults; the bar the device is held to as well)."""
    w = cases.tracking_window(shape)
    p = cases.tracking_problem(w, start)
    slot = p.meta["tracked_slot"]
    gt = w.meta["cams_gt"][slot]
    rot0, tr0 = cases.pose_error(p.cams[slot], gt)
    res = lm.CameraBlocks(p).solve(max_num_iterations=50)
    rot, tr = cases.pose_error(res["cams"][slot], gt)
    print("%s from %s: start %.2e rad %.3f m -> end %.2e rad %.4f m in %d iterations (%s)" % (shape, start, rot0, tr0, rot, tr,
                                                                                           len(res["iterations"]) - 1, res["message"]))
    assert lm.CameraBlocks(p).cols == [slot]
    assert tr <= cases.TRACK_BAR_M and rot <= cases.TRACK_BAR_RAD, (rot, tr)
    others = [c for c in range(p.n_frames) if c != slot]
    assert np.array_equal(res["cams"][others], p.cams[others])


def test_empty_program_is_refused_by_the_yardstick(small_window):
    p = cases.tracking_problem(small_window, "zero", slot=0)      # only the constant camera has residual blocks
    with pytest.raises(ValueError, match="empty program"):
        lm.CameraBlocks(p).solve()


# ---- ABI and plumbing without a device ------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_rejects_a_null_engine():
    from photobundle_amd import _lib
    L = _lib.lib()
    assert "pba_set_points_constant" in _lib.SYMBOLS
    assert hasattr(L, "pba_set_points_constant")
    assert L.pba_set_points_constant(None, 1) == -1      # PBA_ERR_INVALID


def test_header_declares_the_call():
    with open(os.path.join(ROOT, "include", "pba.h")) as f:
        text = f.read()
    assert "int pba_set_points_constant(pba_engine* e, int32_t on);" in text


def test_python_wrapper_exists():
    from photobundle_amd.engine import Engine
    assert callable(getattr(Engine, "set_points_constant"))


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_cases_have_four_clear_iterations(name):
    """The condition of the device trace test (tests/test_gpu_pose_only.py), on the yardstick alone: every case has at least 4 iterations
    before the first one whose decision hinges on the last bits."""
    p, _ = cases.trace_case(name)
    res = lm.CameraBlocks(p).solve(max_num_iterations=50)
    assert lm.compared_iterations(res) >= 4, [(i["step_is_successful"], i["relative_decrease"]) for i in res["iterations"]]


def test_host_header_compiles_with_trackframe_called(tmp_path):
    import host_class_probe
    L = host_class_probe.HostClassProbe(tmp_path).L
    for name in ("probe_create", "probe_add", "probe_track", "probe_track_defaults"):
        assert hasattr(L, name)


def _run_kitti(args):
    import subprocess
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
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\n%s" % (tmp, tmp, extra))
    return cfg


def test_run_kitti_rejects_an_unknown_initial_pose(tmp_path):
    cfg = _tiny_sequence(tmp_path, "InitialPose = bogus\n")
    r = _run_kitti(["-c", cfg, "-o", os.path.join(str(tmp_path), "out.txt")])
    assert r.returncode == 1
    assert "InitialPose must be trajectory or track, not bogus" in r.stderr


def test_run_kitti_rejects_the_batch_with_tracking(tmp_path):
    cfg = _tiny_sequence(tmp_path, "InitialPose = track\n")
    r = _run_kitti(["-b", "%s:%s" % (cfg, os.path.join(str(tmp_path), "out.txt"))])
    assert r.returncode == 1
    assert "-b does not take InitialPose = track" in r.stderr
