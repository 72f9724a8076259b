"""-m gpu: the point prior (pba_set_point_prior) against the prior-augmented yardsticks of tests/point_prior_cases.py.

Bars, those of tests/test_gpu_marginal.py for a camera prior: system entries 1e-9 of the largest, cost 1e-9, model cost change 1e-7, step
norm 1e-5, x_norm 1e-12, radius 1e-6, final parameters 1e-5, decisions equal; the covariance against the longdouble inverse of the
yardstick's H + Lambda within 10 x kappa x 1e-12 in correlation units (covariance_cases)."""
import numpy as np
import pytest

from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

import admit_cases as ac
import covariance_cases as cc
import lm_yardstick as lm
import marginal_cases as mc
import point_prior_cases as pp

pytestmark = pytest.mark.gpu

PBA_ERR_INVALID, PBA_ERR_STATE, PBA_ERR_NUMERIC = -1, -4, -6
TIME_FIELDS = ("iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds", "total_time_in_seconds")
NO_LIN = "call order violated.*pba_step before pba_linearize"


def _engine(p, anchors, keep=True, prior=None, cams_const=False, max_frames=None, **kw):
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, max_frames or p.n_frames, huber=p.huber, keep_reduced_system=keep, **kw)
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(p.cams, constant_slots=anchors)
    if cams_const:
        e.set_cameras_constant(True)
    if prior is not None:
        e.set_point_prior(*prior)
    return e


def _strip(res):
    out = {k: v for k, v in res.items() if k not in TIME_FIELDS and k not in ("iterations", "cams", "xyz", "num_resolve_passes")}
    its = [{k: v for k, v in it.items() if k not in TIME_FIELDS} for it in res["iterations"]]
    return out, its, res["cams"].tobytes(), res["xyz"].tobytes()


# ---- 1. first step and reduced system ------------------------------------------------------------------------------------------------------
STEP_PARAMS = [(n, k) for n in pp.STEP_CASES for k in pp.KINDS]      # every case with every prior


@pytest.mark.parametrize("name,kind", STEP_PARAMS)
def test_reduced_system_and_first_step(name, kind):
    p, anchors, prior = pp.window(name), pp.anchors_of(name), pp.prior(name, kind)
    st = pp.DenseWithPointPrior(p, anchors, *prior).first_step(radius=1e4)
    with _engine(p, anchors, prior=prior) as e:
        assert e.n_free == len(st["free"])
        cost_lin = e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
        e.accept()
        cams1, xyz1 = e.get_state()
    d_S, d_rhs = np.abs(S - st["S"]).max() / np.abs(st["S"]).max(), np.abs(rhs - st["rhs"]).max() / np.abs(st["rhs"]).max()
    print("%s %s: n %d, S %.3e, rhs %.3e of the largest entry; cost %.12e / %.12e, mcc %.9e / %.9e, step %.9e / %.9e, x %.12e / %.12e" % (
        name, kind, S.shape[0], d_S, d_rhs, info["cost"], st["cost"], info["model_cost_change"], st["model_cost_change"], info["step_norm"],
        st["step_norm"], info["x_norm"], st["x_norm"]))
    assert S.shape == st["S"].shape
    assert d_S <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] == 1 and st["linear_solver_ok"]
    assert np.isclose(info["cost"], st["cost"], rtol=1e-9) and np.isclose(cost_lin, st["cost"], rtol=1e-9)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], st["step_norm"], rtol=1e-5)
    assert np.isclose(info["x_norm"], st["x_norm"], rtol=1e-12)
    assert np.abs(cams1[st["free"]] - (p.cams[st["free"]] + st["delta_c"])).max() <= 1e-5
    assert np.abs(xyz1 - (p.xyz + st["delta_p"])).max() <= 1e-5
    for s in anchors:
        assert cams1[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()


@pytest.mark.parametrize("name,kind", STEP_PARAMS)
def test_point_system_in_the_cameras_constant_mode(name, kind):
    p, prior = pp.window(name), pp.prior(name, kind)
    st = pp.PointBlocksWithPrior(p, *prior).first_step(radius=1e4)
    with _engine(p, pp.anchors_of(name), prior=prior, cams_const=True) as e:
        cost_lin = e.linearize()
        info = e.step(1e4, init_scale=True)
        V, rhs = e.point_system()
        e.accept()
        _, xyz1 = e.get_state()
    d_V, d_rhs = np.abs(V - st["S"]).max() / np.abs(st["S"]).max(), np.abs(rhs - st["rhs"]).max() / np.abs(st["rhs"]).max()
    print("%s %s: blocks %.3e, rhs %.3e of the largest entry; cost %.12e / %.12e, mcc %.9e / %.9e, step %.9e / %.9e" % (
        name, kind, d_V, d_rhs, info["cost"], st["cost"], info["model_cost_change"], st["model_cost_change"], info["step_norm"], st["step_norm"]))
    assert d_V <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] == 1 and st["linear_solver_ok"]
    assert np.isclose(info["cost"], st["cost"], rtol=1e-9) and np.isclose(cost_lin, st["cost"], rtol=1e-9)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], st["step_norm"], rtol=1e-5)
    assert np.isclose(info["x_norm"], st["x_norm"], rtol=1e-12)
    assert np.abs(xyz1 - (p.xyz + st["delta"])).max() <= 1e-5


# ---- 2. the whole LM log ---------------------------------------------------------------------------------------------------------------------
def _check_trace(name, res, res_ref, n_cmp, p):
    """test_gpu_marginal.py::_check_trace."""
    gi, ri = res["iterations"], res_ref["iterations"][:n_cmp]
    assert len(gi) == n_cmp, (res["message"], res_ref["message"])
    for a, b in zip(ri, gi):
        print(name, a["iteration"], a["step_is_successful"], b["step_is_successful"], "cost %.12e %.12e" % (a["cost"], b["cost"]),
              "step %.6e %.6e" % (a["step_norm"], b["step_norm"]), "mcc %.6e %.6e" % (a["model_cost_change"], b["model_cost_change"]),
              "radius %.6e %.6e" % (a["trust_region_radius"], b["trust_region_radius"]))
        assert a["iteration"] == b["iteration"]
        assert a["step_is_successful"] == b["step_is_successful"] and a["step_is_valid"] == b["step_is_valid"], a["iteration"]
        assert np.isclose(a["cost"], b["cost"], rtol=1e-9), a["iteration"]
        assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-6)
        if a["iteration"] > 0 and a["step_is_valid"]:
            assert np.isclose(a["step_norm"], b["step_norm"], rtol=1e-5)
            assert np.isclose(a["model_cost_change"], b["model_cost_change"], rtol=1e-7)
    assert res["fixed_cost"] == 0.0
    assert res["num_residual_blocks"] == p.n_obs                   # the photometric blocks only
    assert res["num_residuals"] == p.n_obs * p.patch_len * p.channels
    assert np.isclose(res["initial_cost"], res_ref["initial_cost"], rtol=1e-9)


@pytest.mark.parametrize("mode", ("full", "cameras-constant"))
@pytest.mark.parametrize("name", pp.TRACE_CASES)
def test_trace_matches_the_yardstick(name, mode):
    kind = "depth" if name != pp.CAUSAL else "mixed"
    p, anchors, prior = pp.window(name), pp.anchors_of(name), pp.prior(name, kind)
    res_ref, n_cmp = pp.yardstick(name, kind, mode)
    assert n_cmp >= 3
    if p.n_frames >= 16:
        n_cmp = min(n_cmp, pp.BOUNDARY_ITERATIONS)
    full = mode == "full"
    prog = pp.DenseWithPointPrior(p, anchors, *prior) if full else pp.PointBlocksWithPrior(p, *prior)
    with _engine(p, anchors, keep=False, prior=prior, cams_const=not full) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        cams_after, xyz_after = e.get_state()
    _check_trace("%s %s" % (name, mode), res, res_ref, n_cmp, p)
    ref_state = res_ref["states"][n_cmp - 1]
    cams_ref, x_ref = ref_state if full else (p.cams, ref_state)
    print(name, mode, "max parameter difference: cameras %.3e, points %.3e" % (np.abs(cams_after - cams_ref).max(), np.abs(xyz_after - x_ref).max()))
    assert np.abs(cams_after - cams_ref).max() <= 1e-5 and np.abs(xyz_after - x_ref).max() <= 1e-5
    # final_cost = photometric + E_pts, both recomputed on the host at the state read back
    E_final = pp.energy(*prior, xyz_after)
    photometric = lm.huber_cost(p, cams_after, xyz_after)
    print(name, mode, "final cost %.12e, host %.12e of which E %.6e" % (res["final_cost"], photometric + E_final, E_final))
    assert np.isclose(res["final_cost"], photometric + E_final, rtol=1e-9)
    assert np.isclose(prog.cost((cams_after, xyz_after) if full else xyz_after), photometric + E_final, rtol=1e-12)
    assert E_final > 1e-6 * res["final_cost"]


# ---- 3. the headline: the gauge closed -------------------------------------------------------------------------------------------------------
def test_depth_priors_close_the_gauge():
    """Three frames, one constant camera.  Without the prior the covariance fails (or passes by rounding, with a pivot near 1e-13); with
    the rank-1 depth priors it is the longdouble inverse of the yardstick's H + Lambda."""
    p, anchors, prior = pp.window(pp.GAUGE), pp.anchors_of(pp.GAUGE), pp.prior(pp.GAUGE, "depth")
    prog = pp.DenseWithPointPrior(p, anchors, *prior)
    H, nc = prog.linearize(prog.start())["H"], prog.n_cam
    inv, _ = cc.inverse_ld(H)
    kappa = cc.kappa(H)
    bar = 10 * kappa * cc.RECORD_BAR
    want_pts = np.stack([inv[nc + 3 * i:nc + 3 * i + 3, nc + 3 * i:nc + 3 * i + 3] for i in range(p.n_points)])
    with _engine(p, anchors, keep=False) as e:
        try:
            piv0 = e.covariance()["min_cam_pivot"]
            print("without the prior: PBA_OK with min_cam_pivot %.3e" % piv0)
            assert piv0 < 1e-9
        except EngineError as err:
            print("without the prior:", err)
            assert err.status == PBA_ERR_NUMERIC
        e.set_point_prior(*prior)
        got = e.covariance()
    d_c, d_p = cc.correlation_error(got["cam_cov"], inv[:nc, :nc]), cc.correlation_error(got["point_cov"], want_pts)
    print("with the prior: min_cam_pivot %.3e, kappa %.3e, bar %.3e; cam_cov %.3e, point_cov %.3e in correlation units" % (
        got["min_cam_pivot"], kappa, bar, d_c, d_p))
    assert kappa <= mc.KAPPA_MAX
    assert got["min_cam_pivot"] >= mc.PIVOT_MIN
    assert got["cam_cov"].shape == (nc, nc)
    assert d_c <= bar and d_p <= bar


def test_covariance_in_the_cameras_constant_mode_includes_the_prior():
    name = "3-dense-257-points-anchor-0"
    p, prior = pp.window(name), pp.prior(name, "mixed")
    prog = pp.PointBlocksWithPrior(p, *prior)
    V = prog.linearize(prog.start())["V"]
    want = np.stack([cc.inverse_ld(v)[0] for v in V])
    bar = 10 * max(cc.kappa(v) for v in V) * cc.RECORD_BAR
    with _engine(p, pp.anchors_of(name), keep=False, prior=prior, cams_const=True) as e:
        got = e.covariance(cameras=False)
        e.set_point_prior(None)
        plain = e.covariance(cameras=False)
    d = cc.correlation_error(got["point_cov"], want)
    print("cameras-constant covariance with the prior: %.3e in correlation units, bar %.3e" % (d, bar))
    assert d <= bar
    assert cc.correlation_error(plain["point_cov"], want) > 100 * bar      # the prior is not nothing
    # a point with Lambda = 0 keeps the covariance it had, bit for bit
    zero = np.abs(prior[1]).max(1) == 0
    assert zero.any() and got["point_cov"][zero].tobytes() == plain["point_cov"][zero].tobytes()


# ---- 4. the zero prior -----------------------------------------------------------------------------------------------------------------------
def _zero(p):
    return np.ascontiguousarray(p.xyz, np.float64) + 0.5, np.zeros((p.n_points, 6))


def test_zero_prior_on_a_wide_window_solves_bit_for_bit_as_no_prior():
    """A window of more than 16 slots runs the wide chain with and without a prior: adding zeros changes no bit."""
    p, anchors = pp.window(pp.WIDE), pp.anchors_of(pp.WIDE)
    o = default_solver_options(max_num_iterations=6)
    with _engine(p, anchors, keep=False) as e:
        plain = e.solve(o)
        assert e.solve_driver() == "host-stepped"
    with _engine(p, anchors, keep=False, prior=_zero(p)) as e:
        with_zero = e.solve(o)
        assert e.solve_driver() == "host-stepped"
    assert len(plain["iterations"]) >= 4
    assert _strip(plain)[0] == _strip(with_zero)[0]
    for a, b in zip(_strip(plain)[1], _strip(with_zero)[1]):
        assert a == b, a["iteration"]
    assert plain["cams"].tobytes() == with_zero["cams"].tobytes() and plain["xyz"].tobytes() == with_zero["xyz"].tobytes()


@pytest.mark.parametrize("name", ("3-dense-65-points-anchor-0", pp.CAUSAL))
def test_zero_prior_on_a_narrow_window_meets_the_yardstick(name):
    """A narrow window changes its elimination (the wide chain instead of k_schur) and its driver: the bars are the yardstick's."""
    p, anchors = pp.window(name), pp.anchors_of(name)
    res_ref = lm.Dense(p, anchors).solve(max_num_iterations=pp.REF_ITERATIONS)
    n_cmp = lm.compared_iterations(res_ref)
    assert n_cmp >= 3
    with _engine(p, anchors, keep=False, prior=_zero(p)) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
    _check_trace(name + " zero prior", res, res_ref, n_cmp, p)
    cams_ref, x_ref = res_ref["states"][n_cmp - 1]
    assert np.abs(res["cams"] - cams_ref).max() <= 1e-5 and np.abs(res["xyz"] - x_ref).max() <= 1e-5


# ---- 5. state --------------------------------------------------------------------------------------------------------------------------------
def test_setting_and_clearing_the_prior_drops_the_linearisation():
    name = "3-dense-257-points-anchor-0"
    p, anchors, prior = pp.window(name), pp.anchors_of(name), pp.prior(name, "full")
    with _engine(p, anchors) as e:
        e.linearize()
        e.step(1e4, init_scale=True)
        e.set_point_prior(*prior)
        with pytest.raises(EngineError, match=NO_LIN):
            e.step(1e4, init_scale=True)
        c_with = e.linearize()
        e.step(1e4, init_scale=True)
        e.set_point_prior(None)
        with pytest.raises(EngineError, match=NO_LIN):
            e.step(1e4, init_scale=True)
        c_without = e.linearize()
    E = pp.energy(*prior, p.xyz)
    print("cost with the prior %.12e, without %.12e, E %.12e" % (c_with, c_without, E))
    assert E > 1e-3 * c_without
    assert np.isclose(c_with - c_without, E, rtol=1e-9)


def test_set_problem_clears_the_prior_and_set_cameras_keeps_it():
    p, anchors, prior = pp.window(pp.CAUSAL), pp.anchors_of(pp.CAUSAL), pp.prior(pp.CAUSAL, "depth")
    o = default_solver_options(max_num_iterations=5)
    with _engine(p, anchors, keep=False) as e:
        fresh = _strip(e.solve(o))
        assert e.solve_driver() != "host-stepped"
    with _engine(p, anchors, keep=False, prior=prior) as e:
        with_prior = _strip(e.solve(o))
        assert e.solve_driver() == "host-stepped" and with_prior[1] != fresh[1]
        # pba_set_cameras keeps the prior ...
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_point_prior(*prior)
        e.set_cameras(p.cams, constant_slots=anchors)
        assert _strip(e.solve(o)) == with_prior and e.solve_driver() == "host-stepped"
        # ... pba_set_problem clears it: the engine solves as a fresh one does, on the device-decided drivers again
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, constant_slots=anchors)
        assert _strip(e.solve(o)) == fresh and e.solve_driver() != "host-stepped"


def _measure(e, o):
    cost = e.linearize()
    res = e.solve(o)
    return cost.hex(), _strip(res)


@pytest.mark.parametrize("cams_const", (False, True))
def test_applied_cull_gathers_the_prior_rows(cams_const):
    """After an applied pba_cull, solve and state equal a fresh engine given the surviving problem and the gathered rows."""
    p = synthetic.make_window(n_frames=4, n_points=300, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0), visibility="causal", huber=0.05)
    prior = pp.prior_of(p, "mixed")
    o = default_solver_options(max_num_iterations=4)
    with _engine(p, (0,), keep=False, prior=prior, cams_const=cams_const) as E:
        E.solve(default_solver_options(max_num_iterations=2))
        cams, x = E.get_state()
        keep, pmap, info = E.cull(factor=1.0, quantile=0.8)
        print("cull: %d -> %d points, %d -> %d blocks" % (info["n_points_before"], info["n_points_after"], info["n_blocks_before"], info["n_blocks_after"]))
        assert info["applied"] == 1 and 0 < info["n_points_after"] < p.n_points
        with pytest.raises(EngineError, match=NO_LIN):
            E.step(1e4, init_scale=True)
        alive = pmap >= 0
        op = pmap[p.obs_point[keep.astype(bool)]].astype(np.int32)
        os_ = p.obs_slot[keep.astype(bool)].astype(np.int32)
        with _engine(p, (0,), keep=False) as F:
            F.set_problem(x[alive], p.desc[alive], op, os_, p.weights)
            for e in (E, F):      # (accepted and set cameras differ in the last bit of dR: tests/test_gpu_state_rules.py)
                e.set_cameras(cams, constant_slots=(0,))
            if cams_const:
                F.set_cameras_constant(True)
            without = F.linearize()
            F.set_point_prior(*pp.gathered(*prior, pmap))
            want, got = _measure(F, o), _measure(E, o)
            state_f, state_e = F.get_state(), E.get_state()
    assert got[0] == want[0] != without.hex()
    assert got[1] == want[1]
    assert state_e[0].tobytes() == state_f[0].tobytes() and state_e[1].tobytes() == state_f[1].tobytes()


def test_applied_admit_keeps_the_prior_rows():
    base = synthetic.make_window(**ac.BASE)
    p = ac.with_holes(base)
    prior = pp.prior_of(p, "mixed")
    o = default_solver_options(max_num_iterations=4)
    with _engine(p, (0,), keep=False, prior=prior) as E:
        E.solve(default_solver_options(max_num_iterations=2))
        cams, x = E.get_state()
        cp, cs, _, take, info = E.admit(**ac.DEFAULTS)
        assert info["applied"] == 1 and info["n_admitted"] > 20
        mp, ms = ac.merged_lists(p.obs_point, p.obs_slot, cp, cs, take)
        with _engine(p, (0,), keep=False) as F:
            F.set_problem(x, p.desc, mp, ms, p.weights)
            for e in (E, F):
                e.set_cameras(cams, constant_slots=(0,))
            without = F.linearize()
            F.set_point_prior(*prior)
            want, got = _measure(F, o), _measure(E, o)
    assert got[0] == want[0] != without.hex()
    assert got[1] == want[1]


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------------
def test_two_fresh_engines_give_the_same_bytes():
    name = "3-dense-257-points-anchor-0"
    p, anchors, prior = pp.window(name), pp.anchors_of(name), pp.prior(name, "mixed")
    out = []
    for _ in range(2):
        with _engine(p, anchors, keep=False, prior=prior) as e:
            res = e.solve(default_solver_options(max_num_iterations=5))
            cov = e.covariance()
            out.append((_strip(res), cov["cam_cov"].tobytes(), cov["point_cov"].tobytes(), cov["min_cam_pivot"], cov["min_point_pivot"]))
    assert len(out[0][0][1]) >= 4
    assert out[0] == out[1]


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was():
    p, anchors, prior = pp.window(pp.CAUSAL), (0,), pp.prior(pp.CAUSAL, "depth")      # (one constant slot: multi-rank takes no more)
    x0, L6 = prior
    o = default_solver_options(max_num_iterations=4)
    with _engine(p, anchors, keep=False, prior=prior) as e:
        with_prior = _strip(e.solve(o))
    with _engine(p, anchors, keep=False) as e:
        fresh = _strip(e.solve(o))
    assert with_prior != fresh

    def reset(e, want, solve=True):
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, constant_slots=anchors)
        if want is with_prior:
            e.set_point_prior(*prior)
        if solve:
            assert _strip(e.solve(o)) == want

    def refused(call, sentence):
        with pytest.raises(EngineError) as err:
            call()
        assert "invalid argument" in str(err.value) and sentence in str(err.value), str(err.value)

    nan, neg = L6.copy(), L6.copy()
    nan[7, 4] = np.nan
    neg[3, 3] = -1e-3
    inf_x0 = x0.copy()
    inf_x0[1, 2] = np.inf
    with _engine(p, anchors, keep=False) as e:
        # invalid arguments, on an engine without a prior and on one that holds one
        for want in (fresh, with_prior):
            reset(e, want, solve=False)                           # the refused calls below, then the solve: the engine held what it held
            refused(lambda: e.set_point_prior(x0[:-1], L6[:-1]), "n_points = %d, the problem has %d" % (p.n_points - 1, p.n_points))
            refused(lambda: e.set_point_prior(x0, None), "exactly one of x0 and Lambda6 is NULL")
            refused(lambda: e.set_point_prior(None, L6), "exactly one of x0 and Lambda6 is NULL")
            refused(lambda: e.set_point_prior(x0, nan), "non-finite Lambda of point 7")
            refused(lambda: e.set_point_prior(inf_x0, L6), "non-finite x0 of point 1")
            refused(lambda: e.set_point_prior(x0, neg), "negative diagonal entry of Lambda of point 3")
            assert _strip(e.solve(o)) == want
        # the prior second: the modes that are on refuse it
        reset(e, fresh)
        e.set_points_constant(True)
        refused(lambda: e.set_point_prior(*prior), "the point prior is not built for the points-constant mode (pba_set_points_constant): the prior is then a constant")
        e.set_points_constant(False)
        rays, rho = synthetic.inverse_depth_rays(p)
        e.set_inverse_depth(rays, rho)
        refused(lambda: e.set_point_prior(*prior), "the point prior is not built for the inverse-depth mode (pba_set_inverse_depth)")
        reset(e, fresh)
        cam_prior = dict(slots=[1], x0=p.cams[[1]], Lambda=np.eye(6), eta=np.zeros(6), c=0.0)
        e.set_camera_prior(**cam_prior)
        refused(lambda: e.set_point_prior(*prior), "the point prior is not built next to the camera prior (pba_set_camera_prior)")
        e.clear_camera_prior()
        # the prior first: the second call is refused and the prior stays
        reset(e, with_prior, solve=False)
        refused(lambda: e.set_points_constant(True), "the point prior (pba_set_point_prior) is not built for the points-constant mode: the prior is then a constant")
        refused(lambda: e.set_inverse_depth(rays, rho), "the point prior (pba_set_point_prior) is not built for the inverse-depth mode")
        refused(lambda: e.set_camera_prior(**cam_prior), "the camera prior is not built next to the point prior (pba_set_point_prior)")
        refused(lambda: e.marginalize((1,)), "the camera prior is not built next to the point prior (pba_set_point_prior)")
        refused(lambda: e.comm_init_callback(lambda v, op: None, 0, 2), "multi-rank solves are not built for the point prior (pba_set_point_prior)")
        with _engine(p, anchors, keep=False) as other:
            with pytest.raises(EngineError, match=r"the point prior \(pba_set_point_prior\) solves alone"):
                solve_batch([other, e], o)
        assert _strip(e.solve(o)) == with_prior
    # no problem set
    _, _, rows, cols = p.planes.shape
    with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber) as e:
        refused(lambda: e.set_point_prior(*prior), "no problem is set")
    # the precision-sweep flags are fixed when the engine is created
    with _engine(p, (0,), keep=False, precision="fp32") as e:
        refused(lambda: e.set_point_prior(*prior), "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the point prior")


def test_multi_rank_engine_refuses_the_prior():
    p, anchors, prior = pp.window(pp.CAUSAL), (0,), pp.prior(pp.CAUSAL, "depth")
    with _engine(p, anchors, keep=False) as e:
        e.comm_init_callback(lambda v, op: None, 0, 2)
        with pytest.raises(EngineError, match=r"multi-rank solves \(pba_comm_\*\) are not built for the point prior"):
            e.set_point_prior(*prior)


# ---- 8. the host class: Options::depthPriorSigma ---------------------------------------------------------------------------------------------
SEQ_SIZE, SEQ_K = (120, 160), (200.0, 200.0, 80.0, 60.0)


def _sequence(n):
    """The synthetic sequence of tests/test_gpu_anchors.py: exactly photo-consistent frames, depth maps scaled by a smooth +-2 % field."""
    import host_class_probe
    imgs, depths, _, local = host_class_probe.sequence(n, SEQ_SIZE, SEQ_K)
    rows, cols = depths[0].shape
    y, x = np.mgrid[0:rows, 0:cols]
    field = 1.0 + 0.02 * np.sin(2 * np.pi * x / cols) * np.cos(2 * np.pi * y / rows)
    return imgs, [np.where(z > 0, z * field, z).astype(np.float32) for z in depths], local


def test_class_with_the_depth_prior(tmp_path):
    """addFrame with depthPriorSigma = 1: every optimisation reports depthPriorCost > 0 as a part of finalCost, and computeCovariance
    works with ONE constant frame; with depthPriorSigma = 0 the class gives the bytes it gives without the field; addFrames throws."""
    import point_prior_class_probe
    n, window = 8, 4
    imgs, depths, local = _sequence(n)
    probe = point_prior_class_probe.PointPriorClassProbe(tmp_path)
    runs = {}
    for key, kw in (("off", dict(sigma=0.0)), ("on", dict(sigma=1.0)), ("cov", dict(sigma=1.0, compute_covariance=True))):
        rc, what = probe.create(SEQ_SIZE, SEQ_K, window, 1, min_score=0.65, num_constant=1, **kw)
        assert rc == 0, what
        runs[key] = [r for r in (probe.add(imgs[i], depths[i], local[i]) for i in range(n)) if r is not None]
        assert len(runs[key]) == n - (window - 1)
    for off, on, cov in zip(runs["off"], runs["on"], runs["cov"]):
        print("finalCost %.6e off / %.6e on of which depthPriorCost %.6e; covariance ok %d, pivots camera %.3e point %.3e (%s)" % (
            off["final_cost"], on["final_cost"], on["depth_prior_cost"], cov["covariance_ok"], cov["min_camera_pivot"], cov["min_point_pivot"], cov["message"]))
        assert off["depth_prior_cost"] == 0.0 and not off["covariance_ok"]
        assert 0.0 < on["depth_prior_cost"] < on["final_cost"]
        assert on["poses"].tobytes() != off["poses"].tobytes()
        # the covariance: one constant frame, window - 1 free ones, pivots well above the rounding level of an open gauge (1e-9)
        assert cov["covariance_ok"], cov["message"]
        assert cov["n_free"] == window - 1 and 1e-6 <= cov["min_camera_pivot"] <= 1 and 0 < cov["min_point_pivot"] <= 1
        assert cov["poses"].tobytes() == on["poses"].tobytes() and cov["depth_prior_cost"] == on["depth_prior_cost"]
    rc, what = probe.create(SEQ_SIZE, SEQ_K, window, 1, sigma=1.0)
    assert rc == 0, what
    rc, what = probe.add_frames()
    assert rc == 1 and what.startswith("addFrames: Options::depthPriorSigma solves alone"), what
    probe.release()


def test_run_kitti_with_the_config_key(tmp_path):
    """run_kitti on the synthetic sequence of tests/test_gpu_anchors.py with the solver settings of the configs0 fixture
    (tests/golden/configs0/config/kitti_stereo.cfg: 3 x 3 patches, 4096 new points per frame, minScore 0.65, Huber 0.05) and a window of
    four frames, as tests/test_gpu_marginal.py runs it: the 1241 x 376 frames of the fixture's own test take minutes."""
    import os
    import subprocess
    import host_class_probe
    run = os.path.join(host_class_probe.PKG, "bin", "run_kitti")
    n_frames = 8
    imgs, depths, local = _sequence(n_frames)
    common = "maxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\n"

    def go(name, extra, batch=False):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        host_class_probe.write_sequence(d, imgs, depths, SEQ_K, local)
        cfg = os.path.join(d, "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n%s%s" % (d, d, common, extra))
        out, res = os.path.join(d, "refined.txt"), os.path.join(d, "results.txt")
        cmd = [run, "-p", "-b", "%s:%s:%s" % (cfg, out, res)] if batch else [run, "-c", cfg, "-o", out, "-r", res, "-p"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if batch:
            return r
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out, "rb").read(), open(res, "rb").read(), r.stderr

    out_absent, res_absent, _ = go("absent", "")
    out_0, res_0, _ = go("zero", "depthPriorSigma = 0\n")
    assert (out_0, res_0) == (out_absent, res_absent)              # off: what the class wrote without the key, byte for byte
    assert b"\ndepthPrior " not in res_0
    out_1, res_1, _ = go("one", "depthPriorSigma = 1\n")
    costs = [float(line.split()[1]) for line in res_1.decode().splitlines() if line.startswith("depthPrior ")]
    print("depthPriorCost per optimisation:", costs)
    assert len(costs) == n_frames - 3 and all(v > 0.0 for v in costs)
    poses_1 = np.array(out_1.split(), np.float64).reshape(-1, 3, 4)
    assert poses_1.shape == (n_frames, 3, 4) and np.isfinite(poses_1).all() and out_1 != out_0
    # computeCovariance with one constant frame: the constructor takes it with the prior, and the trajectory is the one without the key
    out_c, res_c, _ = go("cov", "depthPriorSigma = 1\ncomputeCovariance = 1\nnumConstantFrames = 1\n")
    assert (out_c, res_c) == (out_1, res_1)
    # the batch refuses the key
    r = go("batch", "depthPriorSigma = 1\n", batch=True)
    assert r.returncode == 1 and "Options::depthPriorSigma solves alone" in r.stderr
