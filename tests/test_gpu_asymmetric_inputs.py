"""-m gpu: the engine on inputs that no symmetry hides (tests/asym_cases.py): patch weights that differ from each of their rotations and
flips, fx != fy, cx != cy.  Every other window of the suite has unit or Gaussian weights and fx == fy, so a weight read at the transposed
or mirrored tap, or two exchanged focal lengths, passes there.  tests/test_asymmetric_inputs_cpu.py shows that the reference holds these
inputs to 1e-14 and that each such mix-up moves every block by more than 1e-6: none passes the bars below.

a. every sampler path (the border sweep, radius 1..5, 1 / 3 / 8 channels) with asymmetric weights;
b. every mode on an anisotropic, asymmetric window, each against its own yardstick;
c. every driver.  (d, the class, is the K parameter of tests/test_gpu_dropin_class.py.)

Tolerances are the project's existing ones: records and costs 1e-12 (gpu_util.check_obs_records), system entries 1e-9 of the largest entry,
traces as tests/test_gpu_anchors.py holds them (decisions equal, cost 1e-9, step norm 1e-5, model cost change 1e-7, radius 1e-6, final
parameters 1e-5), covariance and marginalisation 10 x kappa x 1e-12 (their case modules)."""
import numpy as np
import pytest

from oracle import oracle
from photobundle_amd.engine import Engine, default_solver_options, solve_batch

import admit_cases
import asym_cases as ac
import covariance_cases as cc
import cull_cases
import lm_yardstick as lm
import marginal_cases as mc
from gpu_util import check_obs_records, dense_system, reference_step

pytestmark = pytest.mark.gpu


def _engine(p, slots=None, keep=True, rays=None, rho=None, mode="full", prior=None):
    """An engine loaded with p: the cameras through the mask (slots) or through the one-slot call (p.fixed_slot)."""
    rows, cols = p.planes.shape[-2:]
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, channels=p.channels)
    for s in range(p.n_frames):
        if p.channels > 1:
            e.set_frame_channels(s, p.channel_images[s])
        else:
            e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    if rays is not None:
        e.set_inverse_depth(rays, rho)
    if mode == "pose":
        e.set_points_constant()
    elif mode == "structure":
        e.set_cameras_constant()
    if slots is None:
        e.set_cameras(p.cams, p.fixed_slot)
    else:
        e.set_cameras(p.cams, constant_slots=slots)
    if prior is not None:
        e.set_camera_prior(**prior)
    return e


def _check_trace(tag, res, res_ref, n_cmp):
    """tests/test_gpu_anchors.py::_check_trace, with the largest distances printed."""
    gi, ri = res["iterations"], res_ref["iterations"][:n_cmp]
    assert len(gi) == n_cmp, (res["message"], res_ref["message"])
    worst = dict(cost=0.0, radius=0.0, step=0.0, mcc=0.0)

    def rel(a, b):
        return abs(a - b) / max(abs(a), 1e-300)

    for a, b in zip(ri, gi):
        assert a["iteration"] == b["iteration"]
        assert a["step_is_successful"] == b["step_is_successful"] and a["step_is_valid"] == b["step_is_valid"], (tag, a["iteration"])
        worst["cost"] = max(worst["cost"], rel(a["cost"], b["cost"]))
        worst["radius"] = max(worst["radius"], rel(a["trust_region_radius"], b["trust_region_radius"]))
        if a["iteration"] > 0 and a["step_is_valid"]:
            worst["step"] = max(worst["step"], rel(a["step_norm"], b["step_norm"]))
            worst["mcc"] = max(worst["mcc"], rel(a["model_cost_change"], b["model_cost_change"]))
    print("ASYM trace %s: %d iterations, cost %.3e, radius %.3e, step norm %.3e, model cost change %.3e" % (
        tag, n_cmp, worst["cost"], worst["radius"], worst["step"], worst["mcc"]))
    for a, b in zip(ri, gi):
        assert np.isclose(a["cost"], b["cost"], rtol=1e-9), (tag, a["iteration"], a["cost"], b["cost"])
        assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-6), (tag, a["iteration"])
        if a["iteration"] > 0 and a["step_is_valid"]:
            assert np.isclose(a["step_norm"], b["step_norm"], rtol=1e-5), (tag, a["iteration"])
            assert np.isclose(a["model_cost_change"], b["model_cost_change"], rtol=1e-7), (tag, a["iteration"])
    assert np.isclose(res["initial_cost"], res_ref["initial_cost"], rtol=1e-9)


def _check_dense_state(tag, e, res_ref, n_cmp, p, slots, inverse_depth=False):
    cams_after, x_after = e.get_state()
    cams_ref, x_ref = res_ref["states"][n_cmp - 1]
    d = x_ref.shape[1]
    print("ASYM state %s: cameras %.3e, points %.3e" % (tag, np.abs(cams_after - cams_ref).max(), np.abs(x_after[:, :d] - x_ref).max()))
    assert np.abs(cams_after - cams_ref).max() <= 1e-5 and np.abs(x_after[:, :d] - x_ref).max() <= 1e-5
    if inverse_depth:
        assert not x_after[:, 1:].any()
    for s in slots:
        assert cams_after[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()


# ---- a. every sampler path with asymmetric weights --------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3, 8])
@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5])
def test_every_border_and_corner_with_asymmetric_weights(radius, channels):
    p = ac.border_problem(radius, channels)
    assert p.n_obs == 968 and (p.weights != 1.0).any()
    lin = oracle.linearize(p, blocks=False)
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
        info = e.step(1e4, init_scale=True)
        e.accept()
        cams1, xyz1 = e.get_state()
    d_cost = abs(cost - lin["cost"]) / lin["cost"]
    d_block = np.abs(rec[:, 5] - 0.5 * lin["block_sqnorm"]) / np.maximum(0.5 * lin["block_sqnorm"], 1e-300)
    print("ASYM sweep radius %d channels %d: cost %.3e, block costs %.3e" % (radius, channels, d_cost, d_block.max()))
    assert np.isfinite(cost) and np.isclose(cost, lin["cost"], rtol=1e-12), (cost, lin["cost"])
    assert np.allclose(rec[:, 5], 0.5 * lin["block_sqnorm"], rtol=1e-12, atol=0.0)
    worst = check_obs_records(p, rec)
    print("ASYM sweep radius %d channels %d: worst record %.3e %r" % (radius, channels, max(worst.values()), worst))
    # the fused cost pass over the same borders: the candidate's cost at the state the step wrote
    c_ref, _ = oracle.cost(p, cams=cams1, xyz=xyz1, threads=8)
    print("ASYM sweep radius %d channels %d: candidate cost %.3e" % (radius, channels, abs(info["candidate_cost"] - c_ref) / c_ref))
    assert np.isclose(info["candidate_cost"], c_ref, rtol=1e-11, atol=0.0), (info["candidate_cost"], c_ref)
    assert cams1[0].tobytes() == np.zeros(6).tobytes() and cams1[1].any()


# ---- b. every mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A4-anchors-0-3", "A5-anchors-0-4"])
def test_full_mode_system_and_trace(case):
    import test_gpu_anchors as anchors
    p, slots, _, _, _ = ac.dense_program(case)
    anchors._check_system(p, slots, "ASYM system " + case)
    res_ref, n_cmp = ac.dense_trace(case)
    with _engine(p, slots, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() != "host-stepped"
        _check_trace(case, res, res_ref, n_cmp)
        _check_dense_state(case, e, res_ref, n_cmp, p, slots)
    assert res["fixed_cost"] == 0.0 and res["num_residual_blocks"] == p.n_obs and res["num_residuals"] == p.n_obs * p.patch_len


def test_wide_chain():
    case = "A17-anchor-0"
    p, slots, _, _, _ = ac.dense_program(case)
    assert p.n_frames == 17 and slots == (0,) and p.fixed_slot == 0 and len(np.unique(p.obs_slot)) == 17
    lin = oracle.linearize(p, blocks=False)
    J, r, n_cam = dense_system(p)
    assert n_cam == 6 * 16
    ref = reference_step(J, r, n_cam, 1e4)
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
    assert np.isclose(cost, lin["cost"], rtol=1e-12)
    assert np.allclose(rec[:, 5], 0.5 * lin["block_sqnorm"], rtol=1e-12, atol=0.0)
    worst = check_obs_records(p, rec)
    d_S, d_rhs = np.abs(S - ref["S"]).max() / np.abs(ref["S"]).max(), np.abs(rhs - ref["rhs"]).max() / np.abs(ref["rhs"]).max()
    print("ASYM system %s: records %.3e, S %.3e, rhs %.3e of the largest entry" % (case, max(worst.values()), d_S, d_rhs))
    assert S.shape == (n_cam, n_cam) and d_S <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] and info["eval_ok"]
    assert np.isclose(info["gradient_max_norm"], np.abs(ref["gradient"]).max(), rtol=1e-10)
    assert np.isclose(info["gradient_norm"], np.linalg.norm(ref["gradient"]), rtol=1e-10)
    assert np.isclose(info["model_cost_change"], ref["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], np.linalg.norm(ref["delta"]), rtol=1e-7)
    res_ref, n_cmp = ac.dense_trace(case)
    assert n_cmp == ac.REF_ITERATIONS + 1            # a trace of 6 iterations
    with _engine(p, slots, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"    # the wide chain
        _check_trace(case, res, res_ref, n_cmp)
        _check_dense_state(case, e, res_ref, n_cmp, p, slots)


@pytest.mark.parametrize("name", ac.POSE_CASES)
def test_pose_only(name):
    import test_gpu_pose_only as pose
    p = ac.window(name)
    st = ac.pose_program(name).first_step(radius=1e4)
    S_ref, rhs_ref, free = pose._expected_system(p, st)
    with _engine(p, mode="pose") as e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
    d_S, d_rhs = np.abs(S - S_ref).max() / np.abs(S_ref).max(), np.abs(rhs - rhs_ref).max() / np.abs(rhs_ref).max()
    print("ASYM system pose-only %s: S %.3e, rhs %.3e of the largest entry" % (name, d_S, d_rhs))
    assert S.shape == S_ref.shape and d_S <= 1e-9 and d_rhs <= 1e-9
    assert not S[S_ref == 0.0].any()
    assert info["linear_solver_ok"] == 1
    assert np.isclose(info["cost"], st["cost"], rtol=1e-12)
    assert np.isclose(info["gradient_max_norm"], np.abs(st["gradient"]).max(), rtol=1e-10)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], np.linalg.norm(st["delta"]), rtol=1e-7)
    res_ref, n_cmp = ac.pose_trace(name)
    with _engine(p, mode="pose", keep=False) as e:
        pts_before = e.get_state()[1].tobytes()
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        cams_after, pts_after = e.get_state()
    _check_trace("pose-only " + name, res, res_ref, n_cmp)
    cams_ref = res_ref["states"][n_cmp - 1]
    print("ASYM state pose-only %s: cameras %.3e" % (name, np.abs(cams_after - cams_ref).max()))
    assert np.abs(cams_after - cams_ref).max() <= 1e-5
    assert pts_after.tobytes() == pts_before and np.array_equal(cams_after[0], p.cams[0])
    assert np.isclose(res["fixed_cost"], res_ref["fixed_cost"], rtol=1e-12, atol=0.0)
    assert res["num_residual_blocks"] == res_ref["num_residual_blocks"]


@pytest.mark.parametrize("case", sorted(ac.STRUCTURE_CASES))
def test_structure_only(case):
    import test_gpu_points_only as points
    p, rays, rho, _ = ac.structure_program(case)
    points._check_system(p, _engine(p, rays=rays, rho=rho, mode="structure"), rays, rho)
    if case in ac.FIRST_STEP_ONLY:
        return                                       # the first candidate leaves the domain of the inverse depths (asym_cases.WINDOWS)
    res_ref, n_cmp = ac.structure_trace(case)
    with _engine(p, rays=rays, rho=rho, mode="structure", keep=False) as e:
        cams_before = e.get_state()[0].tobytes()
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        cams_after, x_after = e.get_state()
    _check_trace("structure-only " + case, res, res_ref, n_cmp)
    x_ref = res_ref["states"][n_cmp - 1]
    d = x_ref.shape[1]
    print("ASYM state structure-only %s: points %.3e" % (case, np.abs(x_after[:, :d] - x_ref).max()))
    assert np.abs(x_after[:, :d] - x_ref).max() <= 1e-5
    assert cams_after.tobytes() == cams_before == np.ascontiguousarray(p.cams, np.float64).tobytes()
    assert res["fixed_cost"] == 0.0 and res["num_residual_blocks"] == p.n_obs


def test_inverse_depth_full_mode_first_step_on_a4():
    """The system and the step; the candidate itself has a point behind its ray origin (asym_cases.WINDOWS), which the engine reports as
    a failed evaluation."""
    case = "A4-inverse-depth-anchors-0-3"
    p, slots, rays, rho, _ = ac.dense_program(case)
    st = ac.dense_first_step(case)
    with _engine(p, slots, rays=rays, rho=rho) as e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
        e.accept()
        cams1, x1 = e.get_state()
    d_S, d_rhs = np.abs(S - st["S"]).max() / np.abs(st["S"]).max(), np.abs(rhs - st["rhs"]).max() / np.abs(st["rhs"]).max()
    print("ASYM system %s: S %.3e, rhs %.3e of the largest entry" % (case, d_S, d_rhs))
    assert S.shape == st["S"].shape == (12, 12) and d_S <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] == 1 and st["linear_solver_ok"]
    assert np.isclose(info["cost"], st["cost"], rtol=1e-9)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], st["step_norm"], rtol=1e-5)
    assert np.isclose(info["x_norm"], st["x_norm"], rtol=1e-12)
    assert (rho + st["delta_p"].ravel()).min() < 0.0 and not info["eval_ok"]
    assert np.abs(cams1[st["free"]] - (p.cams[st["free"]] + st["delta_c"])).max() <= 1e-5
    assert np.abs(x1[:, :1] - (rho[:, None] + st["delta_p"])).max() <= 1e-5 and not x1[:, 1:].any()


def test_inverse_depth_full_mode_trace():
    case = "G11-inverse-depth-anchors-0-3"
    p, slots, rays, rho, _ = ac.dense_program(case)
    res_ref, n_cmp = ac.dense_trace(case)
    assert res_ref["min_candidate"] > 0.0
    with _engine(p, slots, keep=False, rays=rays, rho=rho) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() != "host-stepped"
        _check_trace(case, res, res_ref, n_cmp)
        _check_dense_state(case, e, res_ref, n_cmp, p, slots, inverse_depth=True)


def test_multichannel_records_and_first_step():
    p = ac.window("A4c3")
    assert p.channels == 3 and p.desc.shape[1] == 3 * p.patch_len
    lin = oracle.linearize(p, blocks=False)
    J, r, n_cam = dense_system(p)
    ref = reference_step(J, r, n_cam, 1e4)
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
    assert np.isclose(cost, lin["cost"], rtol=1e-12)
    assert np.allclose(rec[:, 5], 0.5 * lin["block_sqnorm"], rtol=1e-12, atol=0.0)
    worst = check_obs_records(p, rec)
    d_S, d_rhs = np.abs(S - ref["S"]).max() / np.abs(ref["S"]).max(), np.abs(rhs - ref["rhs"]).max() / np.abs(ref["rhs"]).max()
    print("ASYM system A4c3: records %.3e, S %.3e, rhs %.3e of the largest entry" % (max(worst.values()), d_S, d_rhs))
    assert d_S <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] == 1
    assert np.isclose(info["gradient_max_norm"], np.abs(ref["gradient"]).max(), rtol=1e-10)
    assert np.isclose(info["model_cost_change"], ref["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], np.linalg.norm(ref["delta"]), rtol=1e-7)


def test_covariance():
    import test_gpu_covariance as covariance
    name, slots = ac.COVARIANCE_CASE
    p = ac.window(name)
    ref = cc.full_reference(p, slots)
    with _engine(p, slots, keep=False) as e:
        covariance._check_full("ASYM covariance " + name, p, slots, e.covariance(), ref)
    # pose-only: the blocks of the free cameras
    cols, ref_pose, U, cost = cc.pose_reference(p, slots)
    bar = 10 * max(np.linalg.cond(cc.unit_diagonal(u)[0]) for u in U) * cc.RECORD_BAR
    with _engine(p, slots, keep=False, mode="pose") as e:
        cov = e.covariance(points=False)
    err = cc.correlation_error(cov["cam_cov"], ref_pose)
    print("ASYM covariance pose-only: columns %r, bar %.3e, error %.3e" % (cols, bar, err))
    assert cols == [1, 2] and cov["n_cam"] == 12 and err <= bar
    assert np.isclose(cov["cost"], cost, rtol=1e-9)
    # structure-only
    ref_pts, V, cost = cc.structure_reference(p)
    with _engine(p, slots, keep=False, mode="structure") as e:
        covariance._check_structure("ASYM covariance structure-only", p, e.covariance(cameras=False), ref_pts, V, cost, 3)


@pytest.mark.parametrize("case", sorted(ac.MARGINAL_CASES))
def test_marginalisation(case):
    name, anchors, drop = ac.MARGINAL_CASES[case]
    p = ac.window(name)
    ref = ac.marginal_reference(case)
    with _engine(p, anchors, keep=False) as e:
        got = e.marginalize(drop)
        mc.check_against_reference(got, ref, "ASYM " + case)
        assert got["failed_is_point"] == 0 and got["failed_index"] == -1
        # the returned prior goes back in: the cost is then the photometric one plus E at the unmoved cameras, which is c
        c_plain = e.linearize()
        e.set_camera_prior(**mc.as_prior(got))
        c_with = e.linearize()
    print("ASYM %s: cost %.12e, with the returned prior %.12e, c %.12e" % (case, c_plain, c_with, got["c"]))
    assert np.isclose(c_with - c_plain, got["c"], rtol=1e-9)


def test_solve_with_a_prior():
    """The engine and the yardstick are given the same prior (the reference's, as tests/test_gpu_marginal.py does), on the window it came
    from: A4 is dense, so the window without the marginalised points would be empty."""
    name, anchors, _ = ac.MARGINAL_CASES[ac.PRIOR_SOLVE]
    p = ac.window(name)
    res_ref, n_cmp, prior = ac.prior_trace()
    prog = mc.DenseWithPrior(p, anchors, prior)
    with _engine(p, anchors, keep=False, prior=prior) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        _check_trace("prior " + ac.PRIOR_SOLVE, res, res_ref, n_cmp)
        _check_dense_state("prior " + ac.PRIOR_SOLVE, e, res_ref, n_cmp, p, anchors)
        state = e.get_state()
    total, E = prog.cost(state), prog.prior_cost(state)
    assert np.isclose(res["final_cost"], total, rtol=1e-9) and E > 1e-6 * total


def test_block_costs_after_a_solve():
    name, slots, n_it = ac.CULL_CASE
    p = ac.window(name)
    with _engine(p, slots, keep=False) as e:
        e.solve(default_solver_options(max_num_iterations=n_it))
        c = e.block_costs()
        assert c.tobytes() == np.ascontiguousarray(e.obs_records()[:, 5]).tobytes()
        cams, xyz = e.get_state()
    want = cull_cases.yardstick_block_costs(p, cams, xyz)
    err = np.abs(c - want) / np.maximum(np.abs(want), 1e-300)
    print("ASYM block costs %s after %d iterations: largest relative difference %.3e" % (name, n_it, err.max()))
    assert np.isfinite(c).all() and (c >= 0).all()
    np.testing.assert_allclose(c, want, rtol=1e-12, atol=0.0)


def test_admission_candidates_and_costs():
    """pba_admit projects with fx, fy and tests u against the columns and v against the rows: on a 120 x 160 image with fx / fy = 1.35 an
    exchanged pair changes the list."""
    name, slots, n_it = ac.ADMIT_CASE
    p = admit_cases.with_holes(ac.window(name))
    with _engine(p, slots, keep=False) as e:
        e.solve(default_solver_options(max_num_iterations=n_it))
        cams, xyz = e.get_state()
        cp, cs, cost, _, info = e.admit(apply=False)
    want_point, want_slot, margins = admit_cases.reference_candidates(p, cams, xyz, (1 << p.n_frames) - 1, 0.1, p.radius)
    print("ASYM admit: %d candidates, margins %.3g px, %.3g depth" % (len(want_point), margins["px"], margins["depth"]))
    assert margins["px"] >= 1e-6 and margins["depth"] >= 1e-9 and len(want_point) > 20
    assert cp.tobytes() == want_point.tobytes() and cs.tobytes() == want_slot.tobytes()
    assert info["n_candidates"] == info["n_written"] == len(want_point) and info["applied"] == 0
    want = cull_cases.yardstick_block_costs(admit_cases.candidate_window(p, cams, xyz, want_point, want_slot), cams, xyz)
    err = np.abs(cost - want) / np.maximum(np.abs(want), 1e-300)
    print("ASYM admit: candidate costs, largest relative difference %.3e" % err.max())
    np.testing.assert_allclose(cost, want, rtol=1e-12, atol=0.0)


# ---- c. every driver ------------------------------------------------------------------------------------------------------------------------
def _solve(p, slots, driver, n_it):
    import test_gpu_anchors as anchors
    with anchors._env(anchors.DRIVERS[driver]):
        with _engine(p, slots, keep=False) as e:
            res = e.solve(default_solver_options(max_num_iterations=n_it))
            assert e.solve_driver() == driver, (driver, e.solve_driver())
            return res, e.get_state()


@pytest.mark.parametrize("driver", ["resident", "pipelined", "host-stepped", "batched"])
@pytest.mark.parametrize("case", ["A4-anchor-0", "A3h-anchor-0"])
def test_every_driver_matches_the_yardstick(case, driver):
    p, slots, _, _, _ = ac.dense_program(case)
    res_ref, n_cmp = ac.dense_trace(case)
    o = default_solver_options(max_num_iterations=n_cmp - 1)
    if driver == "batched":
        with _engine(p, slots, keep=False) as a, _engine(p, slots, keep=False) as b:
            results = solve_batch([a, b], o)
            assert a.solve_driver() == b.solve_driver() == "batched"
            for k, (res, e) in enumerate(zip(results, (a, b))):
                _check_trace("%s %s-%d" % (case, driver, k), res, res_ref, n_cmp)
                _check_dense_state("%s %s-%d" % (case, driver, k), e, res_ref, n_cmp, p, slots)
    else:
        import test_gpu_anchors as anchors
        with anchors._env(anchors.DRIVERS[driver]):
            with _engine(p, slots, keep=False) as e:
                res = e.solve(o)
                assert e.solve_driver() == driver
                _check_trace("%s %s" % (case, driver), res, res_ref, n_cmp)
                _check_dense_state("%s %s" % (case, driver), e, res_ref, n_cmp, p, slots)


@pytest.mark.parametrize("case", ["A4-anchor-0", "A3h-anchor-0"])
def test_resident_equals_pipelined_and_batched_equals_solo_bit_for_bit(case):
    import test_gpu_anchors as anchors
    p, slots, _, _, _ = ac.dense_program(case)
    runs = {d: anchors._strip(_solve(p, slots, d, 10)[0]) for d in ("resident", "pipelined")}
    with _engine(p, slots, keep=False) as a, _engine(p, slots, keep=False) as b:
        ra, rb = solve_batch([a, b], default_solver_options(max_num_iterations=10))
        assert a.solve_driver() == b.solve_driver() == "batched"
    assert len(ra["iterations"]) >= 4
    assert runs["resident"] == runs["pipelined"]
    assert anchors._strip(ra) == anchors._strip(rb) == runs["pipelined"]


@pytest.mark.parametrize("driver", ["pipelined", "host-stepped"])
@pytest.mark.parametrize("case", ["R4-anchor-0", "R5-anchor-0"])
def test_large_radius_drivers(case, driver):
    """Radius 4 and 5: the second round of the per-tap pass (taps 64 and up).  The resident kernel exists for radius 1 and 2."""
    p, slots, _, _, _ = ac.dense_program(case)
    res_ref, n_cmp = ac.dense_trace(case)
    lin = oracle.linearize(p, blocks=False)
    with _engine(p, slots) as e:
        assert np.isclose(e.linearize(), lin["cost"], rtol=1e-12)
        worst = check_obs_records(p, e.obs_records())
    print("ASYM records %s: %.3e" % (case, max(worst.values())))
    import test_gpu_anchors as anchors
    with anchors._env(anchors.DRIVERS[driver]):
        with _engine(p, slots, keep=False) as e:
            res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
            assert e.solve_driver() == driver
            _check_trace("%s %s" % (case, driver), res, res_ref, n_cmp)
            _check_dense_state("%s %s" % (case, driver), e, res_ref, n_cmp, p, slots)
