"""-m gpu: structure-only solves (pba_set_cameras_constant) against the numpy yardstick tests/lm_yardstick.py (PointBlocks), which evaluates through
the unchanged oracle.

Tolerances are the project's own, as tests/test_gpu_pose_only.py holds them: the system blocks 1e-9 of the largest entry, the trace
decisions equal, cost 1e-9 relative, step norm 1e-5, model cost change 1e-7, radius 1e-6, final parameters 1e-5 (smoke's bar)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

import lm_yardstick as lm
import points_only_cases as cases
from gpu_util import make_engine

pytestmark = pytest.mark.gpu

TIME_FIELDS = ("iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds", "total_time_in_seconds")


@functools.lru_cache(maxsize=None)
def _case(name):
    return cases.trace_case(name)


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """The yardstick's run of a trace case, computed once and shared: (result, compared iterations)."""
    p, _, rays, rho = _case(name)
    res = lm.PointBlocks(p, rays, rho).solve(max_num_iterations=cases.REF_ITERATIONS)
    return res, lm.compared_iterations(res)


@functools.lru_cache(maxsize=None)
def _boundary_window():
    return cases.cameras_to_ground_truth(synthetic.make_window(**cases.BOUNDARY_WINDOW))


def _engine(p, rays=None, rho=None):
    e = make_engine(p)
    if rays is not None:
        e.set_inverse_depth(rays, rho)
    e.set_cameras_constant()
    return e


def _check_system(p, e, rays, rho):
    with e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        V, rhs = e.point_system()
        with pytest.raises(EngineError, match="no reduced camera system"):
            e.reduced_system()
    st = lm.PointBlocks(p, rays, rho).first_step(radius=1e4)
    d = st["S"].shape[1]
    V_ref, rhs_ref = np.zeros((p.n_points, 3, 3)), np.zeros((p.n_points, 3))
    V_ref[:, :d, :d], rhs_ref[:, :d] = st["S"], st["rhs"]      # inverse depth: entry 0 of each is set, the rest are zero
    print("n_points %d: V %.3e of %.3e, rhs %.3e of %.3e" % (p.n_points, np.abs(V - V_ref).max(), np.abs(V_ref).max(),
                                                             np.abs(rhs - rhs_ref).max(), np.abs(rhs_ref).max()))
    assert np.abs(V - V_ref).max() <= 1e-9 * np.abs(V_ref).max()
    assert np.abs(rhs - rhs_ref).max() <= 1e-9 * np.abs(rhs_ref).max()
    if d == 1:
        assert not V[:, 1:, :].any() and not V[:, :, 1:].any() and not rhs[:, 1:].any()
    assert info["linear_solver_ok"] == 1
    assert np.isclose(info["cost"], st["cost"], rtol=1e-12)
    assert np.isclose(info["gradient_max_norm"], np.abs(st["gradient"]).max(), rtol=1e-10)
    assert np.isclose(info["gradient_norm"], np.linalg.norm(st["gradient"]), rtol=1e-10)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], np.linalg.norm(st["delta"]), rtol=1e-7)
    assert np.isclose(info["x_norm"], np.linalg.norm(st["x"]), rtol=1e-13)      # over the points: cameras enter none of the scalars


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_system_matches_the_yardstick(name):
    p, _, rays, rho = _case(name)
    _check_system(p, _engine(p, rays, rho), rays, rho)


@pytest.mark.parametrize("k", cases.BOUNDARY_COUNTS)
def test_system_at_the_wave_and_workgroup_boundaries(k):
    """The first k points of one 700-point window: one fewer than, exactly and one more than a wave (64) and a workgroup (256) of the
    per-point kernels, one point alone, and three workgroups with a ragged last one."""
    p = cases.first_points(_boundary_window(), k)
    assert p.n_points == k
    _check_system(p, _engine(p), None, None)


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_matches_the_yardstick(name):
    p, extras, rays, rho = _case(name)
    res_ref, n_cmp = _yardstick(name)
    assert n_cmp >= 4, "the case must give 4 clear iterations on the yardstick alone"
    with _engine(p, rays, rho) as e:
        cams_before = e.get_state()[0].tobytes()
        assert cams_before == np.ascontiguousarray(p.cams, np.float64).tobytes()
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        cams_after, x_after = e.get_state()
        world_after = e.get_points_world()
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
    # the summary of the reduced program: every residual block, nothing constant
    assert res["fixed_cost"] == 0.0
    assert res["num_residual_blocks"] == p.n_obs
    assert res["num_residuals"] == p.n_obs * p.patch_len * p.channels
    assert np.isclose(res["initial_cost"], res_ref["initial_cost"], rtol=1e-12)
    # the state the yardstick holds after the last compared iteration, in the parameters the program optimises
    if "single-observation" not in extras:
        x_ref = res_ref["states"][n_cmp - 1]
        d = x_ref.shape[1]
        print(name, "max parameter difference", np.abs(x_after[:, :d] - x_ref).max())
        assert np.abs(x_after[:, :d] - x_ref).max() <= 1e-5
    # constancy: the cameras are byte-identical to what was set, before and after
    assert cams_after.tobytes() == cams_before
    if rays is not None:
        assert not x_after[:, 1:].any()
        assert np.allclose(world_after, rays[:, :3] + rays[:, 3:] / x_after[:, :1], rtol=1e-14, atol=0.0)
    else:
        assert world_after.tobytes() == x_after.tobytes()


def _strip(res):
    out = {k: v for k, v in res.items() if k not in TIME_FIELDS and k not in ("iterations", "cams", "xyz")}
    its = [{k: v for k, v in it.items() if k not in TIME_FIELDS} for it in res["iterations"]]
    return out, its, res["cams"].tobytes(), res["xyz"].tobytes()


def test_two_fresh_engines_give_identical_bits():
    p, _, rays, rho = _case("8-frames-r1-huber-causal")
    runs = []
    for _ in range(2):
        with _engine(p, rays, rho) as e:
            runs.append(_strip(e.solve(default_solver_options(max_num_iterations=10))))
    assert runs[0] == runs[1]


def test_rejected_steps_resolve_the_stored_system():
    """From a radius of 1e12 the yardstick rejects steps (checked without a device in test_points_only_cpu.py too); the device repeats
    the decisions, and a re-solve does not rebuild the per-point system: under event profiling the Schur counter counts the launches
    of k_points_system, one per linearisation a step was taken from."""
    p, _, rays, rho = _case("3-frames-r1-huber")
    res_ref = lm.PointBlocks(p, rays, rho).solve(max_num_iterations=6, initial_trust_region_radius=1e12)
    n_cmp = lm.compared_iterations(res_ref)
    ri = res_ref["iterations"][:n_cmp]
    assert any(i["step_is_valid"] and not i["step_is_successful"] for i in ri[1:])
    with _engine(p, rays, rho) as e:
        e.reset_counters()          # switches event profiling on
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1, initial_trust_region_radius=1e12))
        c = e.counters()
    gi = res["iterations"]
    assert [(i["step_is_valid"], i["step_is_successful"]) for i in gi] == [(i["step_is_valid"], i["step_is_successful"]) for i in ri]
    # Decisions only, as the mode's contract has it for this start: at a radius of 1e12 the blocks are all but undamped (condition
    # numbers up to 3e7 on this 3-frame window) and the yardstick's own costs move by 5e-4 .. 4e-3 when its V blocks are perturbed by
    # 1e-12 of their largest entry, a thousandth of what the system test allows -- no cost bound tighter than that follows from the
    # reference.  (The damped traces above hold the cost to 1e-9.)
    print("costs", ["%.12e / %.12e" % (a["cost"], b["cost"]) for a, b in zip(ri, gi)])
    assert res["num_resolve_passes"] >= 1
    assert c["schur_launches"] == 1 + sum(i["step_is_successful"] for i in gi[1:])      # the first linearisation + one per accepted step
    assert c["solve_launches"] == c["schur_launches"] + res["num_resolve_passes"]


def test_a_failed_block_gives_a_zero_step_everywhere():
    """The single-observation case (every V has rank 2) with min_lm_diagonal = 0 at a radius of 1e30: the damping is below the rounding
    of the blocks, so the third pivot of a block is rounding noise and non-positive in many of them (242 of 400 in numpy's Cholesky).
    Some lanes fail, the others have solved: the step must come back as failed and zero EVERYWHERE -- flag, scalars and candidate points."""
    p, _, _, _ = _case("single-observation-5-frames-r1")
    st = lm.PointBlocks(p).first_step(radius=1e30, min_diag=0.0)
    assert not st["linear_solver_ok"] and not st["delta"].any() and st["model_cost_change"] == 0.0
    o = default_solver_options(min_lm_diagonal=0.0)
    with _engine(p) as e:
        e.linearize()
        info = e.step(1e30, init_scale=True, options=o)
        assert info["linear_solver_ok"] == 0
        assert info["step_norm"] == 0.0 and info["model_cost_change"] == 0.0
        assert np.isclose(info["cost"], st["cost"], rtol=1e-12)
        assert np.isclose(info["gradient_norm"], np.linalg.norm(st["gradient"]), rtol=1e-10)
        e.accept()                   # (what no driver does after a failed step: shows the candidate parity)
        cams, x = e.get_state()
        assert x.tobytes() == np.ascontiguousarray(p.xyz, np.float64).tobytes()
        assert cams.tobytes() == np.ascontiguousarray(p.cams, np.float64).tobytes()
    # the driver: five invalid steps in a row end the solve as a failure, the points stay
    with _engine(p) as e:
        res = e.solve(default_solver_options(min_lm_diagonal=0.0, initial_trust_region_radius=1e30, max_trust_region_radius=1e40))
    res_ref = lm.PointBlocks(p).solve(min_lm_diagonal=0.0, initial_trust_region_radius=1e30, max_trust_region_radius=1e40)
    assert [(i["step_is_valid"], i["step_is_successful"]) for i in res["iterations"]] == \
           [(i["step_is_valid"], i["step_is_successful"]) for i in res_ref["iterations"]]
    assert res["termination_type"] == 2 and "invalid steps" in res["message"] and "invalid steps" in res_ref["message"]
    assert res["xyz"].tobytes() == np.ascontiguousarray(p.xyz, np.float64).tobytes()


@pytest.mark.parametrize("name", ["3-frames-r1-huber", "4-frames-r2-inverse-depth"])
def test_mode_switched_on_before_the_cameras_and_the_inverse_depths(name):
    """pba_set_cameras_constant right after pba_set_problem, before pba_set_cameras / pba_set_inverse_depth: the same bits as the usual
    order, and a second pba_set_cameras in the mode (other cameras, then the right ones again) leaves nothing stale behind."""
    p, _, rays, rho = _case(name)
    _, n_cmp = _yardstick(name)
    o = default_solver_options(max_num_iterations=n_cmp - 1)
    with _engine(p, rays, rho) as e:
        usual = _strip(e.solve(o))
    _, _, rows, cols = p.planes.shape
    with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, channels=p.channels) as e:
        for s in range(p.n_frames):
            e.set_frame(s, p.images[s])
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras_constant()
        if rays is not None:
            e.set_inverse_depth(rays, rho)
        e.set_cameras(synthetic_cams(p), p.fixed_slot)
        e.linearize()
        e.step(1e4, init_scale=True)              # a step of the mode at other cameras: both parities, the stored system
        e.set_cameras(p.cams, -1)                 # (fixed_slot has no effect in the mode)
        other = _strip(e.solve(o))
        assert e.solve_driver() == "host-stepped"
    assert other == usual


def synthetic_cams(p):
    """Other cameras than p.cams: the perturbed initial poses make_window built the points with."""
    from photobundle_amd import se3
    return np.stack([se3.pose_to_params(np.linalg.inv(T)) for T in p.meta["T_init"]])


@pytest.mark.parametrize("how", ["switch-off", "set-problem"])
def test_mode_off_solves_like_a_fresh_engine(small_window, how):
    p = small_window
    o = default_solver_options(max_num_iterations=12)
    with make_engine(p) as e:
        fresh = _strip(e.solve(o))
        driver = e.solve_driver()
    with make_engine(p) as e:
        e.set_cameras_constant()
        if how == "switch-off":
            # a step of the mode that is not accepted: the current points stay, the scales, the candidate parity, the second camera
            # table and the stored linearisation are the mode's
            e.linearize()
            e.step(1e4, init_scale=True)
            e.set_cameras_constant(False)
        else:
            e.solve(default_solver_options(max_num_iterations=6))      # (moves the points: set_problem brings them back)
            assert e.solve_driver() == "host-stepped"
            e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, p.fixed_slot)
        again = _strip(e.solve(o))
        assert e.solve_driver() == driver
    assert again == fresh


def test_refusals(small_window):
    p = small_window
    _, _, rows, cols = p.planes.shape
    # both constant modes, either order
    with make_engine(p) as e:
        e.set_points_constant()
        with pytest.raises(EngineError, match="invalid argument.*pba_set_cameras_constant: the points-constant mode .* the program is empty"):
            e.set_cameras_constant()
    with make_engine(p) as e:
        e.set_cameras_constant()
        with pytest.raises(EngineError, match="invalid argument.*pba_set_points_constant: the cameras-constant mode .* the program is empty"):
            e.set_points_constant()
    # the batch; the refused engine still solves alone afterwards
    with make_engine(p) as e:
        e.set_cameras_constant()
        with pytest.raises(EngineError, match="cameras-constant mode .* solves alone"):
            solve_batch([e])
        res = e.solve(default_solver_options(max_num_iterations=3))
        assert e.solve_driver() == "host-stepped" and res["final_cost"] <= res["initial_cost"]
    # a callback transport, either order
    with make_engine(p) as e:
        e.set_cameras_constant()
        with pytest.raises(EngineError, match="invalid argument.*multi-rank solves are not built for the cameras-constant mode"):
            e.comm_init_callback(lambda v, op: None, 0, 2)
    with make_engine(p) as e:
        e.comm_init_callback(lambda v, op: None, 0, 2)
        with pytest.raises(EngineError, match="invalid argument.*multi-rank solves .* not built for the cameras-constant mode"):
            e.set_cameras_constant()
    # the precision-sweep flags
    with Engine(rows, cols, p.K, p.radius, p.n_frames, precision="fp32") as e:
        e.load(p)
        with pytest.raises(EngineError, match="invalid argument.*precision-sweep .* not built for the cameras-constant mode"):
            e.set_cameras_constant()
    # before a problem exists
    with Engine(rows, cols, p.K, p.radius, p.n_frames) as e:
        with pytest.raises(EngineError, match="call order"):
            e.set_cameras_constant()
    # the point system outside the mode, and without the flag
    with make_engine(p) as e:
        e.linearize()
        e.step(1e4, init_scale=True)
        with pytest.raises(EngineError, match="call order.*pba_get_point_system needs a pba_step in the cameras-constant mode"):
            e.point_system()
    with make_engine(p, keep_reduced_system=False) as e:
        e.set_cameras_constant()
        with pytest.raises(EngineError, match="call order.*flags bit 0"):
            e.point_system()


def test_wide_windows_keep_their_refusals():
    """On 16..32 free cameras pba_set_cameras refuses what it refuses there, mode or no mode: the inverse-depth parameterisation."""
    p, _, _, _ = _case("20-frames-r1-causal")
    rays, rho = synthetic.inverse_depth_rays(p)
    with make_engine(p) as e:
        e.set_cameras_constant()
        with pytest.raises(EngineError, match="invalid argument.*inverse-depth mode is not built for wide windows"):
            e.set_inverse_depth(rays, rho)


# ---- the host class: Options::camerasConstant ---------------------------------------------------------------------------------------------
SEQ_SIZE, SEQ_K = (120, 160), (200.0, 200.0, 80.0, 60.0)


def _noisy_depths(depths):
    """Depth maps scaled by a smooth +-2 % field."""
    rows, cols = depths[0].shape
    y, x = np.mgrid[0:rows, 0:cols]
    field = 1.0 + 0.02 * np.sin(2 * np.pi * x / cols) * np.cos(2 * np.pi * y / rows)
    return [np.where(z > 0, z * field, z).astype(np.float32) for z in depths]


def _chain(local):
    """trajectory.h: T_w_0 = inv(T_0), T_w_i = T_w_(i-1) inv(T_i)."""
    out = [np.linalg.inv(local[0])]
    for T in local[1:]:
        out.append(out[-1] @ np.linalg.inv(T))
    return np.stack(out)


def test_host_class_refines_the_points_and_leaves_the_poses(tmp_path):
    import host_class_probe
    n = 7
    imgs, depths, T_gt, local = host_class_probe.sequence(n, SEQ_SIZE, SEQ_K)
    depths = _noisy_depths(depths)
    probe = host_class_probe.HostClassProbe(tmp_path)
    results = {}
    for on in (True, False):
        probe.create(1, SEQ_SIZE, SEQ_K, window=4, radius=1, min_score=0.65, cameras_constant=on)
        results[on] = [(i, probe.add(imgs[i], depths[i], local[i])) for i in range(n)]
        results[on] = [(i, r) for i, r in results[on] if r is not None]
        assert len(results[on]) == n - 3
    probe.release()
    moved = 0
    for i, r in results[True]:
        print("frame %d: cost %.6e -> %.6e, %d points left" % (i, r["initial_cost"], r["final_cost"], len(r["refined"])))
        assert r["final_cost"] <= r["initial_cost"]
        assert np.abs(r["poses"] - _chain(local[:i + 1])).max() <= 1e-12
        moved += int(np.any(r["refined"] != r["original"]))
    assert moved >= 1
    # the same sequence with the option off still moves the poses
    i, r = results[False][-1]
    assert np.abs(r["poses"] - _chain(local[:i + 1])).max() > 1e-9


@pytest.mark.timeout(900)
def test_run_kitti_maps_against_the_given_trajectory(tmp_path):
    import host_class_probe
    run = os.path.join(host_class_probe.PKG, "bin", "run_kitti")
    n_frames = 8
    imgs, depths, T_gt, local = host_class_probe.sequence(n_frames, SEQ_SIZE, SEQ_K)
    depths = _noisy_depths(depths)
    common = "maxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\n"

    def prepare(name, extra):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        host_class_probe.write_sequence(d, imgs, depths, SEQ_K, local)
        cfg = os.path.join(d, "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n%s%s" % (d, d, common, extra))
        return d, cfg

    def read(d):
        return open(os.path.join(d, "refined.txt"), "rb").read(), open(os.path.join(d, "results.txt"), "rb").read()

    def go(name, extra):
        d, cfg = prepare(name, extra)
        r = subprocess.run([run, "-c", cfg, "-o", os.path.join(d, "refined.txt"), "-r", os.path.join(d, "results.txt"), "-p"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return read(d)

    out_on, res_on = go("on", "camerasConstant = 1\n")
    poses = np.array(out_on.split(), np.float64).reshape(-1, 3, 4)
    # init.txt holds the poses with 17 significant digits: the chain of what run_kitti read is the chain of `local` to the last bit or two
    assert poses.shape[0] == n_frames
    assert np.abs(poses - _chain(local)[:, :3, :]).max() <= 1e-12
    out_off, res_off = go("off", "camerasConstant = 0\n")
    out_absent, res_absent = go("absent", "")
    assert out_off == out_absent and res_off == res_absent
    assert out_off != out_on
    # -b with two such sequences writes what the two solo runs write
    specs = []
    for name in ("batch-a", "batch-b"):
        d, cfg = prepare(name, "camerasConstant = 1\n")
        specs.append((d, "%s:%s:%s" % (cfg, os.path.join(d, "refined.txt"), os.path.join(d, "results.txt"))))
    r = subprocess.run([run, "-p", "-b", specs[0][1], "-b", specs[1][1]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for d, _ in specs:
        assert read(d) == (out_on, res_on)
