"""-m gpu: pose-only solves (pba_set_points_constant) against the numpy yardstick tests/lm_yardstick.py (CameraBlocks), which evaluates through the
unchanged oracle.

Tolerances are the existing ones: the reduced system as test_gpu_parity.py holds it (1e-9 of the largest entry), the trace as
__graft_entry__.smoke and the trace tests do (decisions equal, cost 1e-9 relative, step norm 1e-5, model cost change 1e-7, radius 1e-6),
final cameras 1e-5 (smoke's bar, and under gpu_util.pose_rmse)."""
import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

import lm_yardstick as lm
import pose_only_cases as cases
from gpu_util import make_engine, pose_rmse

pytestmark = pytest.mark.gpu

TIME_FIELDS = ("iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds", "total_time_in_seconds")


def _engine(name):
    p, extras = cases.trace_case(name)
    e = make_engine(p)
    xyz = None
    if "inverse-depth" in extras:
        e.set_inverse_depth(*synthetic.inverse_depth_rays(p))
        xyz = e.get_points_world()
        assert np.abs(xyz - p.xyz).max() <= 1e-9
    e.set_points_constant()
    return p, e, xyz


def _expected_system(p, st):
    """The dense n x n system pba_get_reduced_system returns in the mode: the yardstick's blocks at the free indices of the program's
    cameras; a free camera without residual blocks keeps the damping floor alone."""
    free = [c for c in range(p.n_frames) if c != p.fixed_slot]
    n = 6 * len(free)
    S, rhs = np.zeros((n, n)), np.zeros(n)
    for fa, c in enumerate(free):
        sl = slice(6 * fa, 6 * fa + 6)
        if c in st["cols"]:
            k = st["cols"].index(c)
            S[sl, sl], rhs[sl] = st["S"][k], st["rhs"][k]
        else:
            S[sl, sl] = np.eye(6) * (1e-6 / 1e4)      # clamp(0, min_lm_diagonal, max_lm_diagonal) / radius
    return S, rhs, free


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_system_matches_the_yardstick(name):
    p, e, xyz = _engine(name)
    with e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
    st = lm.CameraBlocks(p, xyz=xyz).first_step(radius=1e4)
    S_ref, rhs_ref, free = _expected_system(p, st)
    assert S.shape == S_ref.shape
    assert np.abs(S - S_ref).max() <= 1e-9 * np.abs(S_ref).max()
    assert np.abs(rhs - rhs_ref).max() <= 1e-9 * np.abs(rhs_ref).max()
    off = S.copy()
    for fa in range(len(free)):
        off[6 * fa:6 * fa + 6, 6 * fa:6 * fa + 6] = 0.0
    assert not off.any()                      # off-diagonal blocks: exactly zero
    assert info["linear_solver_ok"] == 1
    assert np.isclose(info["cost"], st["cost"], rtol=1e-12)
    assert np.isclose(info["gradient_max_norm"], np.abs(st["gradient"]).max(), rtol=1e-10)
    assert np.isclose(info["gradient_norm"], np.linalg.norm(st["gradient"]), rtol=1e-10)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], np.linalg.norm(st["delta"]), rtol=1e-7)
    assert np.isclose(info["x_norm"], np.linalg.norm(p.cams[st["cols"]]), rtol=1e-13)      # points enter none of the scalars


@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_trace_matches_the_yardstick(name):
    p, e, xyz = _engine(name)
    res_ref = lm.CameraBlocks(p, xyz=xyz).solve(max_num_iterations=50)
    n_cmp = lm.compared_iterations(res_ref)
    assert n_cmp >= 4, "the case must give 4 clear iterations on the yardstick alone"
    with e:
        pts_before = (e.get_state()[1].tobytes(), e.get_points_world().tobytes())
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"
        pts_after = (e.get_state()[1].tobytes(), e.get_points_world().tobytes())
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
    # the state the yardstick holds after the last compared iteration
    cams_ref = res_ref["states"][n_cmp - 1]
    rot, tr = pose_rmse(res["cams"], cams_ref)
    print(name, "pose rmse", rot, tr, "max", np.abs(res["cams"] - cams_ref).max())
    assert rot <= 1e-5 and tr <= 1e-5
    assert np.abs(res["cams"] - cams_ref).max() <= 1e-5
    if p.fixed_slot >= 0:
        assert np.array_equal(res["cams"][p.fixed_slot], p.cams[p.fixed_slot])
    # summary: the program's counts, the constant camera's cost
    assert res["num_residual_blocks"] == res_ref["num_residual_blocks"]
    assert res["num_residuals"] == res_ref["num_residual_blocks"] * p.patch_len * p.channels
    assert np.isclose(res["fixed_cost"], res_ref["fixed_cost"], rtol=1e-12, atol=0.0)
    assert np.isclose(res["initial_cost"], res_ref["initial_cost"], rtol=1e-12)
    assert res["initial_cost"] - res["fixed_cost"] == pytest.approx(gi[0]["cost"], rel=1e-12)
    # constancy: the points are byte-identical before and after the solve, in either parameterisation
    assert pts_before == pts_after


def test_fixed_cost_on_a_dense_window():
    p = synthetic.make_window(n_frames=4, n_points=200, radius=1, size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), huber=0.05, seed_offset=3)
    # move the points a little so that the constant camera's blocks carry a cost of their own
    p.xyz = p.xyz + np.random.default_rng(0).normal(0.0, 0.01, p.xyz.shape)
    assert p.fixed_slot == 0 and p.n_obs == 4 * p.n_points
    sq = oracle.linearize(p, blocks=False)["block_sqnorm"]
    c = lm.block_costs(p, sq)
    fixed_ref = float(c[p.obs_slot == 0].sum())
    assert fixed_ref > 0.0
    with make_engine(p) as e:
        e.set_points_constant()
        res = e.solve(default_solver_options(max_num_iterations=5))
    assert np.isclose(res["fixed_cost"], fixed_ref, rtol=1e-12)
    assert res["initial_cost"] - res["fixed_cost"] == pytest.approx(res["iterations"][0]["cost"], rel=1e-12)
    assert np.isclose(res["initial_cost"], c.sum(), rtol=1e-12)
    assert res["num_residual_blocks"] == 3 * p.n_points
    assert res["final_cost"] <= res["initial_cost"]


def _strip(res):
    out = {k: v for k, v in res.items() if k not in TIME_FIELDS and k not in ("iterations", "cams", "xyz")}
    its = [{k: v for k, v in it.items() if k not in TIME_FIELDS} for it in res["iterations"]]
    return out, its, res["cams"].tobytes(), res["xyz"].tobytes()


@pytest.mark.parametrize("how", ["switch-off", "set-problem"])
def test_mode_off_solves_like_a_fresh_engine(small_window, how):
    p = small_window
    o = default_solver_options(max_num_iterations=12)
    with make_engine(p) as e:
        fresh = _strip(e.solve(o))
        driver = e.solve_driver()
    with make_engine(p) as e:
        e.set_points_constant()
        e.solve(default_solver_options(max_num_iterations=6))
        assert e.solve_driver() == "host-stepped"
        if how == "switch-off":
            e.set_points_constant(False)
        else:
            e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, p.fixed_slot)
        again = _strip(e.solve(o))
        assert e.solve_driver() == driver
    assert again == fresh


def test_refusals(small_window):
    p = small_window
    _, _, rows, cols = p.planes.shape
    # the batch
    with make_engine(p) as e:
        e.set_points_constant()
        with pytest.raises(EngineError, match="points-constant mode .* solves alone"):
            solve_batch([e])
    # a callback transport, either order
    with make_engine(p) as e:
        e.set_points_constant()
        with pytest.raises(EngineError, match="invalid argument.*multi-rank solves are not built for the points-constant mode"):
            e.comm_init_callback(lambda v, op: None, 0, 2)
    with make_engine(p) as e:
        e.comm_init_callback(lambda v, op: None, 0, 2)
        with pytest.raises(EngineError, match="invalid argument.*multi-rank solves .* not built for the points-constant mode"):
            e.set_points_constant()
    # the precision-sweep flags
    with Engine(rows, cols, p.K, p.radius, p.n_frames, precision="fp32") as e:
        e.load(p)
        with pytest.raises(EngineError, match="invalid argument.*precision-sweep .* not built for the points-constant mode"):
            e.set_points_constant()
    # before a problem exists
    with Engine(rows, cols, p.K, p.radius, p.n_frames) as e:
        with pytest.raises(EngineError, match="call order"):
            e.set_points_constant()
    # an empty program: only the constant camera has residual blocks
    q = cases.tracking_problem(p, "zero", slot=0)
    with make_engine(q) as e:
        e.set_points_constant()
        with pytest.raises(EngineError, match="invalid argument.*No free camera has a residual block"):
            e.solve()


def test_profiling_mode_one_keeps_working(small_window):
    with make_engine(small_window) as e:
        e.set_points_constant()
        plain = e.solve(default_solver_options(max_num_iterations=4))
    with make_engine(small_window) as e:
        e.set_points_constant()
        e.reset_counters()          # switches event profiling on
        res = e.solve(default_solver_options(max_num_iterations=4))
        c = e.counters()
    assert [i["cost"] for i in res["iterations"]] == [i["cost"] for i in plain["iterations"]]
    assert c["linearize_launches"] >= 1 and c["schur_launches"] >= 1 and c["solve_launches"] >= 1
    assert c["schur_ms"] > 0.0 and c["solve_ms"] > 0.0


# ---- the host class: PhotometricBundleAdjustment::trackFrame ------------------------------------------------------------------------------
SEQ_SIZE, SEQ_K = (120, 160), (200.0, 200.0, 80.0, 60.0)


def _feed(probe, imgs, depths, local, k):
    poses = None
    for i in range(k):
        got = probe.add(imgs[i], depths[i], local[i])
        if got is not None:
            poses = got["poses"]
    return poses


@pytest.mark.parametrize("levels", [1, 2])
def test_track_frame_meets_the_bar_and_leaves_the_instance_alone(tmp_path, levels):
    import host_class_probe
    k = 6
    imgs, depths, T_gt, local = host_class_probe.sequence(k + 1, SEQ_SIZE, SEQ_K)
    probe = host_class_probe.HostClassProbe(tmp_path)
    # a run that never calls trackFrame
    probe.create(levels, SEQ_SIZE, SEQ_K, window=4, radius=1, min_score=0.65)
    _feed(probe, imgs, depths, local, k)
    plain = probe.add(imgs[k], depths[k], local[k])["poses"]
    assert len(plain) == k + 1
    # the same run with trackFrame in between
    probe.create(levels, SEQ_SIZE, SEQ_K, window=4, radius=1, min_score=0.65)
    _feed(probe, imgs, depths, local, k)
    for start, T0 in (("velocity", local[k - 1]), ("zero", np.eye(4))):
        rot0, tr0 = host_class_probe.local_pose_error(T0, local[k])
        T, info = probe.track(imgs[k], T0)
        rot, tr = host_class_probe.local_pose_error(T, local[k])
        print("levels %d from %s: start %.2e rad %.3f m -> end %.2e rad %.4f m; %s" % (levels, start, rot0, tr0, rot, tr, info))
        assert info["tracked"] and info["num_points"] >= 64
        assert info["final_cost"] <= info["initial_cost"]
        assert tr <= cases.TRACK_BAR_M and rot <= cases.TRACK_BAR_RAD, (rot, tr)
    # more points asked for than there are: T_init comes back, tracked = false
    T, info = probe.track(imgs[k], local[k - 1], min_points=10 ** 7)
    assert not info["tracked"] and np.array_equal(T, local[k - 1]) and "too few" in info["message"]
    # const in effect: the following addFrame gives the byte-identical trajectory
    after = probe.add(imgs[k], depths[k], local[k])["poses"]
    assert after.tobytes() == plain.tobytes()
    probe.release()


@pytest.mark.timeout(900)
def test_run_kitti_tracks_its_own_initial_poses(tmp_path):
    import os
    import re
    import subprocess
    import host_class_probe
    run = os.path.join(host_class_probe.PKG, "bin", "run_kitti")
    n_frames = 12
    imgs, depths, T_gt, local = host_class_probe.sequence(n_frames, SEQ_SIZE, SEQ_K)
    common = "maxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\n"

    def go(name, n_lines, extra):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        host_class_probe.write_sequence(d, imgs, depths, SEQ_K, local, n_lines)
        cfg = os.path.join(d, "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n%s%s" % (d, d, common, extra))
        out = os.path.join(d, "refined.txt")
        r = subprocess.run([run, "-c", cfg, "-o", out, "-r", os.path.join(d, "results.txt"), "-p"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r, open(out, "rb").read(), open(os.path.join(d, "results.txt"), "rb").read()

    # tracking, with a two-line trajectory: the run ends with the images
    r, out, _ = go("track", 2, "InitialPose = track\n")
    refined = np.array(out.split(), np.float64).reshape(-1, 3, 4)
    assert refined.shape[0] == n_frames
    tracked = re.findall(r"^track frame (\d+) tracked (\d) points (\d+) iterations (\d+) cost \S+ -> \S+ pose (.*)$", r.stdout, re.M)
    assert [int(t[0]) for t in tracked] == list(range(2, n_frames))
    for t in tracked:
        f_i = int(t[0])
        T = np.eye(4)
        T[:3, :] = np.array(t[4].split(), np.float64).reshape(3, 4)
        rot, tr = host_class_probe.local_pose_error(T, local[f_i])
        print("frame %d: tracked %s, %s points, %s iterations, start pose %.2e rad %.4f m from the ground truth" % (f_i, t[1], t[2], t[3], rot, tr))
        assert t[1] == "1"
        assert tr <= cases.TRACK_BAR_M and rot <= cases.TRACK_BAR_RAD, (f_i, rot, tr)
    # the key absent = InitialPose = trajectory, byte for byte (poses and every Result)
    _, out_a, res_a = go("absent", None, "")
    _, out_b, res_b = go("trajectory", None, "InitialPose = trajectory\n")
    assert out_a == out_b and res_a == res_b
    assert np.array(out_a.split(), np.float64).reshape(-1, 3, 4).shape[0] == n_frames
