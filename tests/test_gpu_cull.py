"""-m gpu: pba_cull / pba_get_block_costs (include/pba.h "outlier culling") against the rule restated in numpy (tests/cull_cases.py).

1. the radix-select kernels through their test hook, against np.partition on the uint64 view;
2. the verdict (keep bytes, point map, every info field) equals the rule bit for bit, and a verdict alone leaves the engine untouched;
3. an applied cull leaves the engine a fresh one reaches through pba_set_problem with the surviving lists, in every mode;
4. the state rules and the refusals;
5. the class and run_kitti on a sequence with an occluder.
Images are 120 x 160 as in the other small GPU tests."""
import dataclasses
import io
import os
import re
import subprocess

import numpy as np
import pytest

import cull_cases as cc
import host_class_probe
from photobundle_amd import _lib, synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

pytestmark = pytest.mark.gpu

SMALL = dict(radius=1, size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
PBA_ERR_INVALID, PBA_ERR_STATE, PBA_ERR_NUMERIC = -1, -4, -6
TIMES = ("total_time_in_seconds", "iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds")


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _strip(res):
    """A solve result without its wall-clock fields, floats as hex (NaN compares equal to itself)."""
    def val(v):
        if isinstance(v, float):
            return v.hex()
        if isinstance(v, np.ndarray):
            return v.tobytes()
        if isinstance(v, list):
            return [_strip(x) for x in v]
        return v
    return {k: val(v) for k, v in res.items() if k not in TIMES}


# ---- 1. the select kernels ---------------------------------------------------------------------------------------------------------
def _select_arrays():
    rng = np.random.default_rng(7)
    out = {"n1": np.array([3.25])}
    for n in (63, 64, 65):
        out["n%d" % n] = rng.random(n) * 10.0
    out["random-100003"] = rng.random(100003) * 50.0
    out["all-equal"] = np.full(1000, 0.3)
    out["one-against-the-rest"] = np.concatenate([[2.0], np.full(999, 1.0)])
    out["denormals-and-zeros"] = np.concatenate([np.zeros(100), np.arange(1, 200).astype(np.uint64).view(np.float64), [2.2250738585072014e-308]])
    mixed = rng.random(500)
    mixed[::7] = np.inf
    mixed[::11] = np.nan
    out["inf-and-nan"] = mixed
    return out


@pytest.fixture(scope="module")
def tiny_engine():
    with Engine(32, 48, (50.0, 50.0, 24.0, 16.0), 1, 2) as e:
        yield e


@pytest.mark.parametrize("name", list(_select_arrays()))
def test_select_equals_partition_on_the_patterns(tiny_engine, name):
    v = _select_arrays()[name]
    n = len(v)
    for k in sorted({0, n // 2, n - 1}):
        got = tiny_engine.select_u64order(v, k)
        want = cc.u64_order_statistic(v, k)
        assert _bits(got) == _bits(want), (name, k, got, want)


def test_select_narrows_in_every_pass():
    """2^20 + 3 values that differ only in their lowest 16 bits: the six upper passes keep everything, the last two decide."""
    rng = np.random.default_rng(11)
    n = 2 ** 20 + 3
    v = (np.float64(1.5).view(np.uint64) + rng.integers(0, 1 << 16, n).astype(np.uint64)).view(np.float64)
    with Engine(32, 48, (50.0, 50.0, 24.0, 16.0), 1, 2) as e:
        for k in (0, n // 2, n - 1):
            assert _bits(e.select_u64order(v, k)) == _bits(cc.u64_order_statistic(v, k)), k


def test_select_hook_refuses_bad_ranks(tiny_engine):
    for k in (-1, 5):
        with pytest.raises(EngineError):
            tiny_engine.select_u64order(np.arange(5.0), k)


# ---- 2. the verdict ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def windows():
    return dict(big=synthetic.make_window(n_frames=4, n_points=3000, visibility="causal", **SMALL),
                sub_tile=synthetic.make_window(n_frames=2, n_points=70, **SMALL),
                wide=synthetic.make_window(n_frames=17, n_points=300, visibility="causal", **SMALL))


def _engine(p, slots=(0,), keep=False, **kw):
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, **kw)
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(p.cams, constant_slots=slots)
    return e


def _assert_verdict(got, want, what):
    keep, pmap, info = got
    wkeep, wmap, winfo = want
    assert keep.tobytes() == wkeep.tobytes(), "%s: keep bytes differ in %d places" % (what, int((keep != wkeep).sum()))
    assert pmap.tobytes() == wmap.tobytes(), "%s: point map" % (what,)
    for f, w in winfo.items():
        g = info[f]
        assert (_bits(g) == _bits(w)) if isinstance(w, float) else g == w, "%s: %s = %r, the rule gives %r" % (what, f, g, w)


@pytest.mark.parametrize("name", ["big", "sub_tile"])
def test_verdict_equals_the_rule_and_leaves_the_engine_alone(windows, name):
    p = windows[name]
    o3, o5 = default_solver_options(max_num_iterations=3), default_solver_options(max_num_iterations=5)
    with _engine(p) as e, _engine(p) as twin:
        e.solve(o3)
        twin.solve(o3)
        c = e.block_costs()
        assert c.tobytes() == np.ascontiguousarray(e.obs_records()[:, 5]).tobytes()
        assert np.isfinite(c).all() and (c >= 0).all()
        rules = [dict(quantile=q, factor=f, min_observations=m) for q in (0.0, 0.5, 0.9, 1.0) for f in (0.0, 1.0, 3.0) for m in (1, 2, 3)]
        tie = float(np.sort(c)[(2 * len(c)) // 3])
        rules += [dict(min_cost=tie, factor=0.0, min_observations=m) for m in (1, 2)] + [dict(min_cost=tie, factor=1.0, quantile=0.25, min_observations=2)]
        removed = set()
        for rule in rules:
            got = e.cull(apply=False, **rule)
            assert got[2]["applied"] == 0 and (e.n_points, e.n_obs) == (p.n_points, p.n_obs)
            _assert_verdict(got, cc.reference_cull(c, p.obs_point, **rule), "%s %r" % (name, rule))
            removed.add(p.n_obs - got[2]["n_blocks_after"])
        print("%s: %d rules, blocks removed between %d and %d of %d" % (name, len(rules), min(removed), max(removed), p.n_obs))
        assert len(removed) > 5 and 0 in removed      # the sweep is no row of equal verdicts
        assert e.block_costs().tobytes() == c.tobytes()
        assert _strip(e.solve(o5)) == _strip(twin.solve(o5))


def test_two_fresh_engines_give_the_same_bytes(windows):
    p = windows["big"]
    out = []
    for _ in range(2):
        with _engine(p) as e:
            keep, pmap, info = e.cull(factor=1.0, quantile=0.8)       # (no linearisation yet: the call runs it)
            out.append((keep.tobytes(), pmap.tobytes(), info, e.linearize().hex(), e.obs_records().tobytes()))
    assert out[0] == out[1] and out[0][2]["applied"] == 1


# ---- 3. an applied cull is the surviving problem ---------------------------------------------------------------------------------------
RULE = dict(factor=1.0, quantile=0.85, min_observations=2)


def _prior(p, slots=(1, 2)):
    rng = np.random.default_rng(5)
    k = len(slots)
    A = rng.standard_normal((6 * k, 6 * k))
    return dict(slots=list(slots), x0=p.cams[list(slots)] + 1e-3 * rng.standard_normal((k, 6)), Lambda=A @ A.T * 50.0 + 10.0 * np.eye(6 * k),
                eta=rng.standard_normal(6 * k), c=0.5)


MODES = {
    "full": dict(),
    "two-anchors": dict(slots=(0, 3)),
    "inverse-depth": dict(inverse_depth=True),
    "pose-only": dict(points_const=True),
    "structure-only": dict(cams_const=True),
    "wide": dict(window="wide"),
    "prior": dict(prior=True),
    "batch": dict(batch=True),
}


def _set_modes(e, mode, rays=None, rho=None):
    if mode.get("inverse_depth"):
        e.set_inverse_depth(rays, rho)
    if mode.get("points_const"):
        e.set_points_constant()
    if mode.get("cams_const"):
        e.set_cameras_constant()


def _measure(e, mode, partner=None):
    """linearize cost, records, the system of one step, a full solve (next to an untouched engine in one batch when asked)."""
    cost = e.linearize()
    rec = e.obs_records()
    e.step(1e4, init_scale=True)
    V, r = e.point_system() if mode.get("cams_const") else e.reduced_system()
    o = default_solver_options(max_num_iterations=6)
    res = solve_batch([e, partner], o)[0] if partner is not None else e.solve(o)
    return cost.hex(), rec.tobytes(), V.tobytes(), r.tobytes(), _strip(res)


def _fresh_survivor(p, E, desc, obs_point, obs_slot, rays, mode, slots, prior):
    """A fresh engine with the surviving problem of E through pba_set_problem, E's parameters and cameras."""
    cams, x = E.get_state()
    _, _, rows, cols = p.planes.shape
    F = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=True)
    for s in range(p.n_frames):
        F.set_frame(s, p.images[s])
    F.set_problem(x, desc, obs_point, obs_slot, p.weights)
    _set_modes(F, mode, rays, x[:, 0].copy())
    for e in (E, F):      # (accepted and set cameras differ in the last bit of dR: tests/test_gpu_state_rules.py)
        e.set_cameras(cams, constant_slots=slots)
        if prior:
            e.set_camera_prior(**prior)
    return F


@pytest.mark.parametrize("name", list(MODES))
def test_applied_cull_equals_set_problem_with_the_survivors(windows, name):
    mode = MODES[name]
    p = windows[mode.get("window", "big")]
    slots = mode.get("slots", (0,))
    rays, rho = synthetic.inverse_depth_rays(p) if mode.get("inverse_depth") else (None, None)
    prior = _prior(p) if mode.get("prior") else None
    E = _engine(p, slots, keep=True)
    try:
        _set_modes(E, mode, rays, rho)
        if prior:
            E.set_camera_prior(**prior)
        E.solve(default_solver_options(max_num_iterations=3))
        desc, obs_point, obs_slot = p.desc, p.obs_point, p.obs_slot
        for round_ in range(2):
            n_obs, n_points = E.n_obs, E.n_points
            keep, pmap, info = E.cull(apply=True, **RULE)
            frac = 1.0 - info["n_blocks_after"] / n_obs
            print("%s, cull %d: %d -> %d blocks (%.1f %%), %d -> %d points, threshold %.6g" % (name, round_, n_obs, info["n_blocks_after"], 100 * frac,
                                                                                                  n_points, info["n_points_after"], info["threshold"]))
            assert info["applied"] == 1 and (E.n_points, E.n_obs) == (info["n_points_after"], info["n_blocks_after"])
            assert 0.05 <= frac <= 0.30 and info["n_points_after"] < n_points
            obs_point, obs_slot = cc.surviving_lists(obs_point, obs_slot, keep, pmap)
            desc = desc[pmap >= 0]
            if rays is not None:
                rays = rays[pmap >= 0]
            assert E.counters()["n_obs"] == len(obs_point) and E.counters()["n_points"] == len(desc)
            with _fresh_survivor(p, E, desc, obs_point, obs_slot, rays, mode, slots, prior) as F:
                if mode.get("batch"):
                    with _engine(p) as pa, _engine(p) as pb:
                        want, got = _measure(F, mode, pa), _measure(E, mode, pb)
                else:
                    want, got = _measure(F, mode), _measure(E, mode)
            for what, g, w in zip(("linearize cost", "records", "system matrix", "right-hand side", "solve"), got, want):
                assert g == w, "%s, cull %d: %s differs from the fresh engine's" % (name, round_, what)
    finally:
        E.close()


# ---- 4. state rules and refusals ---------------------------------------------------------------------------------------------------------
def test_state_after_an_applied_cull(windows):
    p = windows["big"]
    o3 = default_solver_options(max_num_iterations=3)
    # the linearisation is dropped; the anchor mask stays
    with _engine(p, (0, 3)) as e:
        e.solve(o3)
        cams_before = e.get_state()[0]
        assert e.cull(**RULE)[2]["applied"] == 1
        with pytest.raises(EngineError, match="pba_step before pba_linearize") as ei:
            e.step(1e4, init_scale=True)
        res = e.solve(o3)
        assert res["cams"][[0, 3]].tobytes() == cams_before[[0, 3]].tobytes() and res["cams"][1].tobytes() != cams_before[1].tobytes()
    # the points-constant switch stays: the surviving points come back byte for byte after a solve
    with _engine(p) as e:
        e.set_points_constant()
        e.solve(o3)
        x = e.get_state()[1]
        _, pmap, info = e.cull(**RULE)
        assert info["applied"] == 1 and _lib.lib().pba_internal_points_constant(e._h) == 1
        assert e.solve(o3)["xyz"].tobytes() == x[pmap >= 0].tobytes()
    # the cameras-constant switch stays
    with _engine(p) as e:
        e.set_cameras_constant()
        e.solve(o3)
        cams = e.get_state()[0]
        assert e.cull(**RULE)[2]["applied"] == 1
        res = e.solve(o3)
        assert res["cams"].tobytes() == cams.tobytes() and res["num_successful_steps"] >= 1
    # the inverse-depth mode stays, with the survivors' rays (also in the host copy pba_get_points_world reads)
    rays, rho = synthetic.inverse_depth_rays(p)
    with _engine(p) as e:
        e.set_inverse_depth(rays, rho)
        e.solve(o3)
        _, pmap, info = e.cull(**RULE)
        assert info["applied"] == 1
        x = e.get_state()[1]
        s = pmap >= 0
        assert (x[:, 1:] == 0).all() and (x[:, 0] > 0).all()
        assert np.allclose(e.get_points_world(), rays[s, :3] + rays[s, 3:] * (1.0 / x[:, :1]), rtol=1e-14, atol=0.0)
    # the prior stays: the cost of the culled engine is that of a fresh one with the surviving problem AND the prior
    prior = _prior(p)
    with _engine(p) as e:
        e.set_camera_prior(**prior)
        e.solve(o3)
        keep, pmap, info = e.cull(**RULE)
        assert info["applied"] == 1
        cams, x = e.get_state()
        got = e.linearize()
        q_point, q_slot = cc.surviving_lists(p.obs_point, p.obs_slot, keep, pmap)
        costs = []
        for with_prior in (True, False):
            with _engine(p) as f:
                f.set_problem(x, p.desc[pmap >= 0], q_point, q_slot, p.weights)
                f.set_cameras(cams, constant_slots=(0,))
                if with_prior:
                    f.set_camera_prior(**prior)
                costs.append(f.linearize())
        assert got.hex() == costs[0].hex() and costs[0] != costs[1]


def test_a_cull_that_removes_nothing_changes_nothing(windows):
    p = windows["big"]
    with _engine(p) as e, _engine(p) as twin:
        for x in (e, twin):
            x.reset_counters()
            x.linearize()
        before = e.counters()["linearize_launches"]
        keep, pmap, info = e.cull(min_cost=1e300, factor=0.0, min_observations=1, apply=True)
        assert info["applied"] == 0 and keep.all() and np.array_equal(pmap, np.arange(p.n_points))
        assert info["n_blocks_after"] == p.n_obs and info["n_points_after"] == p.n_points and info["threshold"] == 1e300
        assert e.counters()["linearize_launches"] == before == 1
        assert e.step(1e4, init_scale=True) == twin.step(1e4, init_scale=True)      # (the linearisation is still valid)


def test_refusals_leave_the_engine_as_it_was(windows):
    p = windows["big"]
    o = default_solver_options(max_num_iterations=4)
    with _engine(p) as plain:
        want = _strip(plain.solve(o))

    def refused(e, match, status=PBA_ERR_INVALID, **kw):
        with pytest.raises(EngineError, match=match) as ei:
            e.cull(**kw)
        assert ei.value.status == status
        return ei.value

    with _engine(p) as e:
        for kw, match in ((dict(min_cost=-1.0), "min_cost"), (dict(min_cost=float("nan")), "min_cost"), (dict(min_cost=float("inf")), "min_cost"),
                          (dict(factor=-0.5), "factor"), (dict(factor=float("inf")), "factor"), (dict(quantile=1.5), "quantile"),
                          (dict(quantile=-0.1), "quantile"), (dict(quantile=float("nan")), "quantile"), (dict(min_observations=0), "min_observations")):
            refused(e, match, **kw)
        # no point would be left (threshold 0: only the block of a point's own reference frame, whose residual is exactly zero at the
        # initial state, is not over): the verdict is reported, the engine keeps its problem
        err = refused(e, "no point would be left", min_cost=0.0, factor=0.0, min_observations=2)
        assert err.info["n_points_after"] == 0 and err.info["n_blocks_after"] == 0 and err.info["applied"] == 0
        assert err.info["n_blocks_over_threshold"] + err.info["n_blocks_by_point_rule"] == p.n_obs and err.info["n_blocks_by_point_rule"] > 0
        assert not err.block_keep.any() and (err.point_map == -1).all()
        # factor * quantile_cost overflows
        err = refused(e, "not finite", status=PBA_ERR_NUMERIC, factor=1e308, quantile=1.0)
        assert err.info["n_blocks_before"] == p.n_obs and err.info["applied"] == 0 and np.isinf(err.info["threshold"])
        # ... and the verdict alone is no refusal
        assert e.cull(min_cost=0.0, factor=0.0, min_observations=2, apply=False)[2]["n_points_after"] == 0
        assert (e.n_points, e.n_obs) == (p.n_points, p.n_obs)
        assert _strip(e.solve(o)) == want
    with _engine(p, precision="fp32") as e:
        refused(e, "precision-sweep")
    with _engine(p) as e, _engine(p) as twin:
        for x in (e, twin):
            x.comm_init_callback(lambda v, op: None, 0, 2)
        refused(e, "multi-rank")
        assert _strip(e.solve(o)) == _strip(twin.solve(o))
    _, _, rows, cols = p.planes.shape
    with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber) as e:
        refused(e, "call order violated", status=PBA_ERR_STATE)
        with pytest.raises(EngineError, match="call order violated"):
            e.block_costs()


# ---- 5. the class --------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
SEQ = dict(n_frames=6, window=4, occluded_frame=2)


@pytest.fixture(scope="module")
def occluder_sequence():
    """Six photo-consistent 120 x 160 frames with exact depth and perturbed initial poses; the rectangle of cull_cases (the CPU case's
    occluder) overwrites frame 2, which sits in both windows a 4-frame class optimises before the sequence ends."""
    size, K = SMALL["size"], SMALL["K"]
    imgs, depths, T_gt, _ = host_class_probe.sequence(SEQ["n_frames"], size, K)
    local, _ = synthetic.perturb_local_poses(T_gt, rot_deg=0.03, trans=0.005)
    r0, r1, c0, c1 = cc.OCCLUDER_RECT
    imgs = [im.copy() for im in imgs]
    imgs[SEQ["occluded_frame"]][r0:r1, c0:c1] = cc.occluder_patch((r1 - r0, c1 - c0), (r0, c0))
    return imgs, depths, T_gt, local


def _run_kitti(tmp, seq, extra, dump_windows=False):
    imgs, depths, _, local = seq
    os.makedirs(tmp)
    host_class_probe.write_sequence(tmp, imgs, depths, SMALL["K"], local)
    cfg = os.path.join(tmp, "test.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nmaxNumPoints = 4096\nslidingWindowSize = %d\npatchRadius = 1\nminScore = 0.65\n"
                "robustThreshold = 0.05\nverbose = 0\n%s" % (tmp, tmp, SEQ["window"], extra))
    env = dict(os.environ)
    if dump_windows:
        os.makedirs(os.path.join(tmp, "windows"))
        env["PBA_DUMP_WINDOWS"] = os.path.join(tmp, "windows")
    r = subprocess.run([RUN, "-c", cfg, "-o", os.path.join(tmp, "refined.txt"), "-r", os.path.join(tmp, "results.txt"), "-p"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(tmp, "refined.txt")).read(), open(os.path.join(tmp, "results.txt")).read(), r.stdout


def _trajectory_error(refined_text, T_gt):
    T = np.loadtxt(io.StringIO(refined_text)).reshape(-1, 3, 4)
    return float(np.sqrt(np.mean([np.sum((a[:, 3] - b[:3, 3]) ** 2) for a, b in zip(T, T_gt)])))


def test_run_kitti_with_the_occluder(tmp_path, occluder_sequence):
    from oracle import oracle
    from photobundle_amd import imgproc, se3
    from photobundle_amd.problem import WindowProblem
    from test_gpu_configs0 import _read_window
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    imgs, _, T_gt, _ = occluder_sequence
    window = SEQ["window"]
    # outlierPasses = 0 is the class without the keys, byte for byte
    absent = _run_kitti(str(tmp_path / "absent"), occluder_sequence, "")
    zero = _run_kitti(str(tmp_path / "zero"), occluder_sequence, "outlierPasses = 0\noutlierFactor = 1\noutlierQuantile = 0.1\n")
    assert absent == zero and "culled" not in absent[1]
    one = _run_kitti(str(tmp_path / "one"), occluder_sequence, "outlierPasses = 1\n", dump_windows=True)
    culled = [tuple(int(v) for v in m.groups()) for m in re.finditer(r"^culled blocks (\d+) points (\d+)$", one[1], re.M)]
    assert len(culled) == SEQ["n_frames"] - window + 1 and all(b > 0 for b, _ in culled), culled
    e0, e1 = _trajectory_error(absent[0], T_gt), _trajectory_error(one[0], T_gt)
    print("camera-centre RMSE against the ground truth: %.4e without the passes, %.4e with one (culled blocks, points per window: %s)" % (e0, e1, culled))
    assert e1 < e0

    # the first window again, through the engine (the class's own calls: the same bits) and through the CPU yardstick
    w = _read_window(os.path.join(str(tmp_path / "one"), "windows", "window_%06d.bin" % (window - 1)))
    assert (w["id_start"], w["id_end"]) == (0, window - 1)
    frames = np.stack(imgs[:window])      # slot = id % window = id
    p = WindowProblem(K=SMALL["K"], radius=1, planes=np.stack([imgproc.planes_from_u8(im) for im in frames]), cams=w["cams"], xyz=w["xyz"],
                      desc=w["desc"], obs_point=w["obs_point"], obs_slot=w["obs_slot"], weights=w["weights"], huber=w["huber"],
                      fixed_slot=w["first_slot"], images=frames)
    with _engine(p, (w["first_slot"],)) as e:
        e.solve()
        keep, pmap, info = e.cull(apply=True, **cc.DEFAULTS)
        final = e.solve()
    assert (p.n_obs - info["n_blocks_after"], p.n_points - info["n_points_after"]) == culled[0]
    # no removed (point, frame) pair is in the next window (points are told apart by their descriptors)
    nxt = _read_window(os.path.join(str(tmp_path / "one"), "windows", "window_%06d.bin" % window))
    removed = {(p.desc[pt].tobytes(), int(sl)) for pt, sl, k in zip(p.obs_point, p.obs_slot, keep) if not k}      # (slot = frame id here)
    assert len({d for d, _ in removed}) > 1 and len({p.desc[i].tobytes() for i in range(p.n_points)}) == p.n_points
    again = {(nxt["desc"][pt].tobytes(), nxt["id_start"] + (int(sl) - nxt["id_start"]) % window) for pt, sl in zip(nxt["obs_point"], nxt["obs_slot"])}
    assert {d for d, _ in again} & {d for d, _ in removed}, "the next window shares no point with the removed blocks: the check would be empty"
    assert not (again & removed)
    # the class's poses of the window against the yardstick's solve -> rule -> solve, at the replay tolerance of tests/test_gpu_dropin_class.py
    o = oracle.default_options()
    first = oracle.solve(p, o)
    c = cc.yardstick_block_costs(p, first["cams"], first["xyz"])
    rkeep, rmap, _ = cc.reference_cull(c, p.obs_point, **cc.DEFAULTS)
    assert rkeep.tobytes() == keep.tobytes()
    second = oracle.solve(cc.surviving_window(p, dataclasses.replace, first["cams"], first["xyz"], rkeep, rmap), o)
    assert np.abs(final["cams"] - second["cams"]).max() <= 1e-5, np.abs(final["cams"] - second["cams"]).max()
    poses = np.array([[float(v) for v in line.split()[2:]] for line in one[1].split("result frame %d " % window)[0].splitlines()
                      if line.startswith("pose ")]).reshape(-1, 3, 4)
    assert len(poses) == window
    want = np.stack([np.linalg.inv(se3.params_to_pose(cam))[:3, :] for cam in second["cams"]])
    assert np.abs(poses - want).max() <= 1e-5, np.abs(poses - want).max()


def test_track_frame_culls_and_add_frames_refuses(tmp_path, occluder_sequence):
    import cull_class_probe
    imgs, depths, _, local = occluder_sequence
    probe = cull_class_probe.CullClassProbe(tmp_path)
    try:
        probe.create(SMALL["size"], SMALL["K"], window=SEQ["window"], radius=1, min_score=0.65, passes=1)
        ran = [probe.add(im, z, T) for im, z, T in zip(imgs[:5], depths[:5], local[:5])]
        assert [r is not None for r in ran] == [False, False, False, True, True] and all(r["culled_blocks"] > 0 for r in ran[3:])
        T0, plain = probe.track(imgs[5], local[5], passes=0)
        T1, culled = probe.track(imgs[5], local[5], passes=1)
        print("trackFrame: %d points, culled %d blocks (%d points), cost %.6e -> %.6e (without the pass %.6e)"
              % (culled["num_points"], culled["culled_blocks"], culled["culled_points"], culled["initial_cost"], culled["final_cost"], plain["final_cost"]))
        assert plain["tracked"] and culled["tracked"] and plain["culled_blocks"] == plain["culled_points"] == 0
        assert culled["culled_blocks"] == culled["culled_points"] > 0 and culled["num_points"] == plain["num_points"]
        assert culled["initial_cost"] == plain["initial_cost"] and culled["final_cost"] < plain["final_cost"] and not np.array_equal(T0, T1)
        with pytest.raises(RuntimeError, match="addFrames: Options::outlierPasses solves alone"):
            probe.add_frames(imgs[5], depths[5], local[5])
    finally:
        probe.release()
