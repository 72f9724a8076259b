"""-m gpu: wide windows, 16 to 32 free cameras (DESIGN.md "Wide windows"): the unfused sampling chain with 32-entry camera tables,
the two-stage Schur elimination (k_wide_point, k_wide_pairs, k_wide_assemble) and the reduced solve k_solve_wide, on the
host-stepped driver.  Tolerances of test_gpu_parity.py:
  per-observation records / costs       1e-12 relative
  reduced camera system S, rhs           1e-9 relative to the largest entry
  per-iteration LM cost                  1e-9 relative, identical accept/reject sequence
  refined poses                          1e-5 absolute
Narrow windows on an engine created for 32 slots take exactly the narrow kernels and drivers: same bits as a 16-slot engine."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options
from photobundle_amd.problem import WindowProblem

from gpu_util import check_obs_records, dense_system, reference_step, restated_twin, step_accuracy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))


def _window(n_frames, radius=1, n_points=150, huber=0.0, gaussian=False, seed=0, fixed=0, **kw):
    p = synthetic.make_window(n_frames=n_frames, n_points=n_points, radius=radius, huber=huber, gaussian=gaussian,
                              visibility="causal", seed_offset=seed, **dict(SMALL, **kw))
    assert len(np.unique(p.obs_slot)) == n_frames
    p.fixed_slot = fixed
    return p


def _engine(p, max_frames=None, keep=True):
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, max_frames or p.n_frames, huber=p.huber, keep_reduced_system=keep,
               channels=getattr(p, "channels", 1))
    return e.load(p)


def _compare_traces(p, res, ref, kw=None, restated_twins=0):
    """Identical accept / reject sequence and costs to 1e-9 against the oracle; where the traces separate, the oracle's referee mode
    decides as in gpu_util.referee_parity (these windows are chaotic in the rounding: two double-precision runs of the SAME algorithm
    drift apart once a few iterations have amplified their last-bit differences): per iteration the engine stays within
    max(1e-9, 2 x the largest twin distance up to one iteration later) of the extended-precision referee, with the referee's decisions
    while the twins keep them, and its poses within 2 x the twins' distance + 1e-5.
    restated_twins = k (test_gpu_wide_scale.py; default solver options only) adds k double-precision runs that do not share the oracle's
    linear algebra to the twins' cost and pose distances (gpu_util.restated_twin: as it is, then with one-ulp copies of its blocks)."""
    ri, gi = ref["iterations"], res["iterations"]
    exact = len(ri) == len(gi) and all(a["step_is_successful"] == b["step_is_successful"] and a["step_is_valid"] == b["step_is_valid"]
                                       and np.isclose(a["cost"], b["cost"], rtol=1e-9) for a, b in zip(ri, gi))
    if exact:
        for a, b in zip(ri, gi):
            assert np.isclose(a["gradient_max_norm"], b["gradient_max_norm"], rtol=1e-6), a["iteration"]
            if a["iteration"] > 0 and a["step_is_valid"]:
                assert np.isclose(a["step_norm"], b["step_norm"], rtol=1e-5), a["iteration"]
        assert res["termination_type"] == ref["termination_type"] and res["message"] == ref["message"]
        assert np.isclose(res["final_cost"], ref["final_cost"], rtol=1e-9)
        assert np.abs(res["cams"] - ref["cams"]).max() <= 1e-5
    else:
        kw = kw or {}
        q = oracle.solve(p, oracle.default_options(extended_precision=1, use_autodiff=0, **kw))
        twins = [ref, oracle.solve(p, oracle.default_options(use_autodiff=0, **kw))]
        qi = q["iterations"]
        n = min([len(qi), len(gi)] + [len(t["iterations"]) for t in twins])
        d_tw = [max(abs(t["iterations"][i]["cost"] - qi[i]["cost"]) / qi[i]["cost"] for t in twins) for i in range(n)]
        d_en = [abs(gi[i]["cost"] - qi[i]["cost"]) / qi[i]["cost"] for i in range(n)]
        pose_rs = []
        if restated_twins:
            assert set(kw) <= {"max_num_iterations"}
            for seed in [None, 1, 2, 3, 4][:restated_twins]:
                costs, cams = restated_twin(p, len(qi) - 1, seed)
                for i in range(min(n, len(costs))):
                    d_tw[i] = max(d_tw[i], abs(costs[i] - qi[i]["cost"]) / qi[i]["cost"])
                if len(costs) == len(qi) and all(it["step_is_successful"] for it in qi[1:]):      # the same number of accepted steps
                    pose_rs.append(np.abs(cams - q["cams"]).max())
        same = True
        for i in range(n):
            run = max(d_tw[:min(n, i + 2)])
            same = same and all(t["iterations"][i]["step_is_successful"] == qi[i]["step_is_successful"] for t in twins)
            same = same and max(run, d_en[i]) <= 1e-6
            if same:
                assert gi[i]["step_is_successful"] == qi[i]["step_is_successful"] and gi[i]["step_is_valid"] == qi[i]["step_is_valid"], i
            assert d_en[i] <= max(1e-9, 2.0 * run), (i, d_en[i], d_tw[i], run)
        if same:
            assert len(gi) == len(qi) and res["termination_type"] == q["termination_type"]
        pose_tw = max([np.abs(t["cams"] - q["cams"]).max() for t in twins] + pose_rs)
        assert np.abs(res["cams"] - q["cams"]).max() <= 2.0 * pose_tw + 1e-5
    if p.fixed_slot >= 0:
        assert np.array_equal(res["cams"][p.fixed_slot], p.cams[p.fixed_slot])


def _its(res):
    """The iteration log without its wall-clock fields."""
    return [tuple(sorted((k, v) for k, v in i.items() if "time" not in k)) for i in res["iterations"]]


@pytest.mark.parametrize("n_frames,radius", [(20, 2), (32, 1)])
def test_records(n_frames, radius):
    p = _window(n_frames, radius=radius, seed=n_frames)
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
    lin = oracle.linearize(p, blocks=False)
    assert np.isclose(cost, lin["cost"], rtol=1e-12)
    assert np.allclose(rec[:, 5], 0.5 * lin["block_sqnorm"], rtol=1e-12, atol=0)
    check_obs_records(p, rec)


@pytest.mark.parametrize("n_free", [16, 24, 32])
def test_reduced_system_and_step(n_free):
    # 16 free cameras = 17 frames with a constant one; 32 = 32 frames, none constant
    n_frames, fixed = (n_free + 1, 0) if n_free < 32 else (32, -1)
    p = _window(n_frames, radius=1, n_points=100, huber=0.05, seed=n_free, fixed=fixed)
    J, r, n_cam = dense_system(p)
    assert n_cam == 6 * n_free
    ref = reference_step(J, r, n_cam, 1e4)
    with _engine(p) as e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
        assert S.shape == (n_cam, n_cam)
        assert np.abs(S - ref["S"]).max() <= 1e-9 * np.abs(ref["S"]).max()
        assert np.abs(rhs - ref["rhs"]).max() <= 1e-9 * np.abs(ref["rhs"]).max()
        assert info["linear_solver_ok"] and info["eval_ok"]
        assert np.isclose(info["gradient_max_norm"], np.abs(ref["gradient"]).max(), rtol=1e-10)
        assert np.isclose(info["gradient_norm"], np.linalg.norm(ref["gradient"]), rtol=1e-10)
        assert np.isclose(info["model_cost_change"], ref["model_cost_change"], rtol=1e-7)
        assert np.isclose(info["step_norm"], np.linalg.norm(ref["delta"]), rtol=1e-7)
    for row in step_accuracy(p, 2):
        assert row["bwd_engine"] <= 10.0 * row["bwd_f64_band"] + 1e-14, row
        assert row["fwd_engine"] <= 10.0 * row["fwd_f64_band"] + 1e-13, row


@pytest.mark.parametrize("n_frames,radius,huber,gaussian,fixed", [(24, 1, 0.05, False, 0), (24, 2, 0.0, True, -1),
                                                                 (32, 2, 0.05, False, 0), (32, 1, 0.0, True, 0)])
def test_solve_matches_oracle(n_frames, radius, huber, gaussian, fixed):
    p = _window(n_frames, radius=radius, n_points=300, huber=huber, gaussian=gaussian, seed=7 * n_frames + radius, fixed=fixed)
    ref = oracle.solve(p, oracle.default_options(max_num_iterations=15))
    with _engine(p, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=15))
        assert e.solve_driver() == "host-stepped"
    _compare_traces(p, res, ref, dict(max_num_iterations=15))


def test_profiling_shares():
    """The counters fill the same three shares as on narrow windows: elimination | reduction + solve | sampling."""
    p = _window(24, radius=1, n_points=200, seed=4)
    with _engine(p, keep=False) as e:
        e.set_profiling(1)
        e.reset_counters()
        res = e.solve(default_solver_options(max_num_iterations=5))
        c = e.counters()
    n_steps = len(res["iterations"]) - 1
    assert c["schur_ms"] > 0 and c["solve_ms"] > 0 and c["linearize_ms"] > 0
    assert c["schur_launches"] >= n_steps and c["solve_launches"] >= n_steps


def test_multichannel():
    p = _window(20, radius=1, n_points=120, seed=5, channel_fn=synthetic.channel_fn("IntensityAndGradient"))
    assert p.channels == 3
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
        assert np.isclose(cost, oracle.linearize(p, blocks=False)["cost"], rtol=1e-12)
        check_obs_records(p, rec)
    ref = oracle.solve(p, oracle.default_options(max_num_iterations=5))
    with _engine(p, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=5))
    _compare_traces(p, res, ref, dict(max_num_iterations=5))


def _bits(p, max_frames, n_it=10):
    with _engine(p, max_frames=max_frames, keep=False) as e:
        e.linearize()
        rec = e.obs_records()
        res = e.solve(default_solver_options(max_num_iterations=n_it))
        return dict(driver=e.solve_driver(), rec=rec.tobytes(), cams=res["cams"].tobytes(), xyz=res["xyz"].tobytes(),
                    its=_its(res), msg=res["message"])


@pytest.mark.parametrize("n_frames,radius,driver", [(8, 2, "resident"), (9, 3, "pipelined"), (16, 1, "pipelined")])
def test_narrow_window_unchanged_on_a_32_slot_engine(n_frames, radius, driver):
    p = _window(n_frames, radius=radius, n_points=400, huber=0.05, seed=n_frames)
    a, b = _bits(p, 16), _bits(p, 32)
    assert a["driver"] == driver
    assert a == b


def test_solver_options_on_a_wide_window():
    import test_oracle_solver_options as opts
    p = _window(20, radius=1, n_points=200, seed=11)
    cases = [("max_it", dict(max_num_iterations=6)), ("func", dict(max_num_iterations=40, function_tolerance=1e-3)),
             ("grad", dict(max_num_iterations=40, function_tolerance=0.0, gradient_tolerance=1e-2)),
             ("param", dict(max_num_iterations=40, function_tolerance=0.0, parameter_tolerance=1e-3)),
             ("no_jacobi", dict(max_num_iterations=8, jacobi_scaling=0))]
    with _engine(p, keep=False) as e:
        for cid, kw in cases:
            e.load(p)
            res = e.solve(default_solver_options(**kw))
            ref = oracle.solve(p, oracle.default_options(**kw))
            _compare_traces(p, res, ref, kw)
    # invalid steps: a free camera whose frame is flat has zero columns; with min_lm_diagonal = 0 the factorisation fails
    q, _ = opts.flat_camera(p)
    for m in (0, 3):
        kw = dict(min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=m)
        ref = oracle.solve(q, oracle.default_options(**kw))
        assert ref["message"].startswith(opts.INVALID), ref["message"]
        with _engine(q, keep=False) as e:
            res = e.solve(default_solver_options(**kw))
        _compare_traces(q, res, ref, kw)
        assert not any(i["step_is_valid"] for i in res["iterations"][1:])


def test_run_to_run_bits():
    p = _window(32, radius=2, n_points=400, huber=0.05, seed=3)
    runs = []
    for _ in range(2):
        with _engine(p, keep=True) as e:
            e.linearize()
            e.step(1e4, init_scale=True)
            S, rhs = e.reduced_system()
            e.load(p)
            res = e.solve(default_solver_options(max_num_iterations=8))
            runs.append((S.tobytes(), rhs.tobytes(), res["cams"].tobytes(), res["xyz"].tobytes(),
                         _its(res)))
    assert runs[0] == runs[1]


def test_refusals():
    p = _window(20, radius=1, n_points=100, seed=2)
    _, _, rows, cols = p.planes.shape
    # precision-sweep sampler modes
    e = Engine(rows, cols, p.K, p.radius, 20, precision="fp32")
    with pytest.raises(EngineError, match="precision-sweep .* not built for wide windows"):
        e.load(p)
    e.close()
    # inverse depth: after the cameras, and before them
    rays, rho = synthetic.inverse_depth_rays(p)
    with _engine(p) as e:
        with pytest.raises(EngineError, match="inverse-depth mode is not built for wide windows"):
            e.set_inverse_depth(rays, rho)
        q = _window(8, radius=1, n_points=100, seed=2)
        e.load(q)
        e.set_inverse_depth(*synthetic.inverse_depth_rays(q))
        with pytest.raises(EngineError, match="inverse-depth mode .* not built for wide windows"):
            e.set_cameras(p.cams, p.fixed_slot)
    # multi-rank
    with _engine(p) as e:
        with pytest.raises(EngineError, match="multi-rank solves are not built for wide windows"):
            e.comm_init_callback(lambda v, op: None, 0, 2)
    with Engine(rows, cols, p.K, p.radius, 20) as e:
        e.comm_init_callback(lambda v, op: None, 0, 2)
        for s in range(p.n_frames):
            e.set_frame(s, p.images[s])
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        with pytest.raises(EngineError, match="multi-rank solves .* not built for wide windows"):
            e.set_cameras(p.cams, p.fixed_slot)
    # beyond 32 slots: refused at creation
    with pytest.raises(EngineError, match="invalid argument"):
        Engine(rows, cols, p.K, p.radius, 33)


def test_run_kitti_window24(tmp_path):
    """slidingWindowSize = 24 through the drop-in class and run_kitti: every window's cost decreases, and one dumped window
    replays through the oracle (identical decisions, costs to 1e-9) and through the engine."""
    import test_gpu_configs0 as c0
    size, K = (120, 160), (200.0, 200.0, 80.0, 60.0)
    n_frames, window = 26, 24
    tmp = str(tmp_path)
    tex = synthetic.Texture()
    T_gt = synthetic.make_trajectory(n_frames)
    for T in T_gt:
        T[:3, 3] *= 0.1                   # slow forward motion: the small frames keep overlapping over 24 frames
    local, _ = synthetic.perturb_local_poses(T_gt, rot_deg=0.02, trans=0.002)
    images = []
    for i, T in enumerate(T_gt):
        im, z = synthetic.render_frame(T, K, size, tex)
        z = np.where(np.isfinite(z), z, -1.0).astype(np.float32)
        images.append(im)
        with open(os.path.join(tmp, "image_%06d.pgm" % i), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (size[1], size[0]))
            f.write(im.tobytes())
        z.tofile(os.path.join(tmp, "depth_%06d.bin" % i))
    with open(os.path.join(tmp, "calib.txt"), "w") as f:
        f.write("%r %r %r %r 0.5372\n" % tuple(K))
    with open(os.path.join(tmp, "init.txt"), "w") as f:
        for T in local:
            f.write(" ".join("%.17g" % v for v in T[:3, :].reshape(-1)) + "\n")
    cfg = os.path.join(tmp, "w24.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n" % (tmp, tmp))
        f.write("maxNumPoints = 256\nslidingWindowSize = %d\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\n" % window)
    dump_dir = os.path.join(tmp, "windows")
    os.makedirs(dump_dir)
    out, res_txt = os.path.join(tmp, "refined.txt"), os.path.join(tmp, "results.txt")
    r = subprocess.run([c0.RUN, "-c", cfg, "-o", out, "-r", res_txt, "-p"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PBA_DUMP_WINDOWS=dump_dir))
    assert r.returncode == 0, r.stderr[-3000:]
    got = c0._read_results(res_txt)
    assert len(got) == n_frames - window + 1 and all(g["final"] < g["initial"] for g in got)
    refined = np.loadtxt(out).reshape(-1, 3, 4)
    assert refined.shape[0] == n_frames and np.isfinite(refined).all()
    names = sorted(os.listdir(dump_dir))
    assert len(names) == len(got)
    w = c0._read_window(os.path.join(dump_dir, names[0]))
    assert w["window"] == window
    planes_of = [oracle.planes_from_u8(im) for im in images]
    planes = np.stack([planes_of[w["id_start"] + ((s - w["id_start"]) % window)] for s in range(window)])
    fixed = w["first_slot"] if w["first_slot"] in set(w["obs_slot"].tolist()) else -1
    p = WindowProblem(K=tuple(K), radius=w["radius"], planes=planes, cams=w["cams"], xyz=w["xyz"], desc=w["desc"],
                      obs_point=w["obs_point"], obs_slot=w["obs_slot"], weights=w["weights"], huber=w["huber"], fixed_slot=fixed)
    p.images = np.stack([images[w["id_start"] + ((s - w["id_start"]) % window)] for s in range(window)])
    assert len(np.unique(p.obs_slot)) - (1 if fixed >= 0 else 0) >= 16        # a wide window
    assert np.isclose(got[0]["initial"], oracle.cost(p)[0], rtol=1e-12)
    ref = oracle.solve(p, oracle.default_options(max_num_iterations=12))
    with _engine(p, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=12))
    _compare_traces(p, res, ref, dict(max_num_iterations=12))
