"""-m gpu: anchor frames (pba_set_cameras_anchored) against the numpy yardstick tests/lm_yardstick.py (Dense), which evaluates through the
unchanged oracle.

Tolerances are the project's own, as tests/test_gpu_points_only.py and tests/test_gpu_pose_only.py hold them: system entries 1e-9 of the
largest entry; traces: decisions equal, cost 1e-9 relative, step norm 1e-5, model cost change 1e-7, radius 1e-6, final parameters 1e-5."""
import contextlib
import copy
import functools
import os
import subprocess

import numpy as np
import pytest

from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

import anchors_cases as cases
import lm_yardstick as lm

pytestmark = pytest.mark.gpu

TIME_FIELDS = ("iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds", "total_time_in_seconds")
DRIVERS = {"resident": {"PBA_RESIDENT": "1"}, "pipelined": {"PBA_RESIDENT": "0"}, "host-stepped": {"PBA_ASYNC": "0"}}


@contextlib.contextmanager
def _env(env):
    """The driver switches are read when an engine is created."""
    old = {k: os.environ.get(k) for k in ("PBA_RESIDENT", "PBA_ASYNC")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _engine(p, slots=None, fixed_slot=None, keep=True, rays=None, rho=None, precision="exact"):
    """An engine loaded with p; the cameras set through the mask (slots) or through the one-slot call (fixed_slot)."""
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, precision=precision)
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    if rays is not None:
        e.set_inverse_depth(rays, rho)
    if slots is not None:
        e.set_cameras(p.cams, constant_slots=slots)
    else:
        e.set_cameras(p.cams, p.fixed_slot if fixed_slot is None else fixed_slot)
    return e


def _strip(res):
    out = {k: v for k, v in res.items() if k not in TIME_FIELDS and k not in ("iterations", "cams", "xyz")}
    its = [{k: v for k, v in it.items() if k not in TIME_FIELDS} for it in res["iterations"]]
    return out, its, res["cams"].tobytes(), res["xyz"].tobytes()


@functools.lru_cache(maxsize=None)
def _case(name):
    return cases.trace_case(name)


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """The yardstick's run of a trace case, computed once and shared: (result, compared iterations)."""
    p, slots, _, rays, rho = _case(name)
    res = lm.Dense(p, slots, rays, rho).solve(max_num_iterations=cases.REF_ITERATIONS)
    return res, lm.compared_iterations(res)


@functools.lru_cache(maxsize=None)
def _window5():
    return synthetic.make_window(n_frames=5, n_points=130, radius=1, huber=0.05, visibility="causal", size=(96, 128),
                                 K=(160.0, 160.0, 64.0, 48.0))


# ---- 1. the old call is the one-bit mask -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["resident", "pipelined", "host-stepped", "batched"])
def test_fixed_slot_call_equals_the_one_bit_mask(driver):
    p = _window5()
    o = default_solver_options(max_num_iterations=8)
    with _env(DRIVERS.get(driver, {})):
        for fixed in (0, 2, 4, -1):
            with _engine(p, fixed_slot=fixed, keep=False) as a, _engine(p, slots=[] if fixed < 0 else [fixed], keep=False) as b:
                assert a.n_free == b.n_free == p.n_frames - (1 if fixed >= 0 else 0)
                if driver == "batched":
                    ra, rb = solve_batch([a, b], o)
                else:
                    ra, rb = a.solve(o), b.solve(o)
                assert a.solve_driver() == b.solve_driver() == driver, (fixed, a.solve_driver(), b.solve_driver())
                assert _strip(ra) == _strip(rb), fixed
                assert len(ra["iterations"]) >= 3


# ---- 2. the reduced system of the first step -----------------------------------------------------------------------------------------
def _check_system(p, slots, tag):
    st = lm.Dense(p, slots).first_step(radius=1e4)
    with _engine(p, slots=slots) as e:
        assert e.n_free == len(st["free"])
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()             # (asserts n = 6 n_free as the C call reports it)
        e.accept()
        cams1, xyz1 = e.get_state()
    d_S, d_rhs = np.abs(S - st["S"]).max() / np.abs(st["S"]).max(), np.abs(rhs - st["rhs"]).max() / np.abs(st["rhs"]).max()
    print("%s: n %d, S %.3e, rhs %.3e of the largest entry; cost %.12e / %.12e, mcc %.9e / %.9e, step %.9e / %.9e, x %.12e / %.12e" % (
        tag, S.shape[0], d_S, d_rhs, info["cost"], st["cost"], info["model_cost_change"], st["model_cost_change"], info["step_norm"],
        st["step_norm"], info["x_norm"], st["x_norm"]))
    assert S.shape == st["S"].shape == (6 * len(st["free"]), 6 * len(st["free"]))
    assert d_S <= 1e-9 and d_rhs <= 1e-9
    assert info["linear_solver_ok"] == 1 and st["linear_solver_ok"]
    assert np.isclose(info["cost"], st["cost"], rtol=1e-9)
    assert np.isclose(info["model_cost_change"], st["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], st["step_norm"], rtol=1e-5)
    assert np.isclose(info["x_norm"], st["x_norm"], rtol=1e-12)
    # the candidate the step wrote: free cameras and points moved as the yardstick's did, anchored cameras not at all
    assert np.abs(cams1[st["free"]] - (p.cams[st["free"]] + st["delta_c"])).max() <= 1e-5
    assert np.abs(xyz1 - (p.xyz + st["delta_p"])).max() <= 1e-5
    for s in slots:
        assert cams1[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()
    return st, xyz1


@pytest.mark.parametrize("name", ["3x40-dense-r1-anchors-0-2", "4x50-dense-r2-anchors-1-3", "5x60-causal-huber-anchors-0-4",
                                  "5x60-causal-huber-anchors-0-1-2"])
def test_reduced_system_matches_the_yardstick(name):
    p, slots, _, _, _ = _case(name)
    st, _ = _check_system(p, slots, name)
    if name.startswith("3x40"):
        assert st["n_cam"] == 6          # one free camera: one pair block


def test_reduced_system_with_the_highest_slot_anchored():
    p = synthetic.make_window(n_frames=6, n_points=80, radius=1, visibility="causal", size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
    _check_system(p, (1, 3, 5), "6 slots, anchors {1, 3, 5}")


def test_points_seen_by_anchored_cameras_only_still_move():
    """Anchors {0, 1, 2} of 5 causal slots, and every third point keeps only its observations in the anchored slots: its W is empty, it
    has no part in the reduced system, and its own 3 x 3 solve still moves it."""
    p = copy.copy(_case("5x60-causal-huber-anchors-0-1-2")[0])
    slots = (0, 1, 2)
    only = np.zeros(p.n_points, bool)
    has_anchor = np.zeros(p.n_points, bool)
    has_anchor[p.obs_point[np.isin(p.obs_slot, slots)]] = True
    only[::3] = True
    only &= has_anchor
    keep = ~(only[p.obs_point] & ~np.isin(p.obs_slot, slots))
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    assert only.sum() >= 10 and len(np.unique(p.obs_point)) == p.n_points
    assert not np.isin(p.obs_slot[only[p.obs_point]], (3, 4)).any()
    st, xyz1 = _check_system(p, slots, "points of anchored cameras only")
    moved = np.abs(xyz1[only] - p.xyz[only]).max(axis=1)
    print("smallest step of a point seen by anchored cameras only: %.3e" % moved.min())
    # (a point left with its birth frame alone has a zero residual there, the patch its descriptor was cut from, and stays put on
    # the yardstick too: the ones that must move are those the yardstick moves)
    ref_moves = np.abs(st["delta_p"][only]).max(axis=1) > 1e-9
    assert ref_moves.sum() >= 10 and (moved[ref_moves] > 0).all()


def test_free_camera_without_a_residual_block():
    p = copy.copy(_window5())
    keep = p.obs_slot != 2
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    assert len(np.unique(p.obs_point)) == p.n_points
    st, _ = _check_system(p, (0, 4), "free camera 2 without residual blocks")
    assert lm.Dense(p, (0, 4)).live == [1, 3] and st["free"] == [1, 2, 3]
    assert not st["delta_c"][1].any()


# ---- 3. traces -------------------------------------------------------------------------------------------------------------------------
def _check_trace(name, res, res_ref, n_cmp, p, slots):
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
    assert np.isclose(res["initial_cost"], res_ref["initial_cost"], rtol=1e-9)


TRACES = [n for n in sorted(cases.TRACE_CASES) if "inverse-depth" not in cases.TRACE_CASES[n][2]]


@pytest.mark.parametrize("driver", ["default", "host-stepped"])
@pytest.mark.parametrize("name", TRACES)
def test_trace_matches_the_yardstick(name, driver):
    p, slots, _, _, _ = _case(name)
    res_ref, n_cmp = _yardstick(name)
    assert n_cmp >= 4, "the case must give 4 clear iterations on the yardstick alone"
    with _env({} if driver == "default" else DRIVERS[driver]):
        with _engine(p, slots=slots, keep=False) as e:
            cams_before = e.get_state()[0]
            res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
            if driver != "default":
                assert e.solve_driver() == driver
            else:
                assert e.solve_driver() != "host-stepped"
            cams_after, xyz_after = e.get_state()
    _check_trace(name, res, res_ref, n_cmp, p, slots)
    cams_ref, x_ref = res_ref["states"][n_cmp - 1]
    print(name, "max parameter difference: cameras %.3e, points %.3e" % (np.abs(cams_after - cams_ref).max(), np.abs(xyz_after - x_ref).max()))
    assert np.abs(cams_after - cams_ref).max() <= 1e-5 and np.abs(xyz_after - x_ref).max() <= 1e-5
    for s in slots:      # constancy: byte-identical to what was set, before and after
        assert cams_before[s].tobytes() == cams_after[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()
    moved = [c for c in range(p.n_frames) if c not in slots]
    assert all(cams_after[c].tobytes() != cams_before[c].tobytes() for c in moved)


@pytest.mark.parametrize("name", TRACES)
def test_resident_pipelined_and_batched_give_identical_bits(name):
    p, slots, _, _, _ = _case(name)
    o = default_solver_options(max_num_iterations=10)
    runs = {}
    for driver in ("resident", "pipelined"):
        with _env(DRIVERS[driver]):
            with _engine(p, slots=slots, keep=False) as e:
                runs[driver] = _strip(e.solve(o))
                assert e.solve_driver() == driver
    with _engine(p, slots=slots, keep=False) as a, _engine(p, slots=slots, keep=False) as b:
        ra, rb = solve_batch([a, b], o)
        assert a.solve_driver() == b.solve_driver() == "batched"
        runs["batched"], runs["batched-2"] = _strip(ra), _strip(rb)
    assert runs["resident"] == runs["pipelined"] == runs["batched"] == runs["batched-2"]


# ---- 4. the narrow / wide boundary --------------------------------------------------------------------------------------------------
def test_sixteen_slots_with_two_anchors_run_the_narrow_kernels():
    p = cases.boundary_window(16)
    slots = (0, 1)
    st, _ = _check_system(p, slots, "16 slots, 2 anchors")
    assert st["n_cam"] == 6 * 14
    with _engine(p, slots=slots, keep=False) as e:
        e.solve(default_solver_options(max_num_iterations=3))
        assert e.solve_driver() in ("resident", "pipelined")      # not the host-stepped driver of the wide chain


@pytest.mark.parametrize("name", sorted(cases.BOUNDARY_WIDE))
def test_wide_chain_with_anchors(name):
    n_frames, slots = cases.BOUNDARY_WIDE[name]
    p = cases.boundary_window(n_frames)
    assert p.n_points == 64
    st, _ = _check_system(p, slots, name)
    assert st["n_cam"] == 6 * (n_frames - len(slots))
    res_ref = lm.Dense(p, slots).solve(max_num_iterations=6)
    n_cmp = min(lm.compared_iterations(res_ref), 5)
    assert n_cmp >= 3
    with _engine(p, slots=slots, keep=False) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() == "host-stepped"                 # the wide chain
        cams_after, xyz_after = e.get_state()
    _check_trace(name, res, res_ref, n_cmp, p, slots)
    cams_ref, x_ref = res_ref["states"][n_cmp - 1]
    assert np.abs(cams_after - cams_ref).max() <= 1e-5 and np.abs(xyz_after - x_ref).max() <= 1e-5
    for s in slots:
        assert cams_after[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()


# ---- 5. the constant modes under a mask -----------------------------------------------------------------------------------------------
def test_pose_only_with_two_anchors():
    p = _window5()
    slots = (0, 3)
    st = lm.CameraBlocks(p, slots).first_step(radius=1e4)
    assert st["cols"] == [1, 2, 4]
    fixed_ref, prog_ref, n_prog = st["fixed_cost"], st["cost"], st["num_residual_blocks"]
    with _engine(p, slots=slots) as e:
        e.set_points_constant()
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
        res = e.solve(default_solver_options(max_num_iterations=4))
        assert e.solve_driver() == "host-stepped"
        cams_after, xyz_after = e.get_state()
    assert S.shape == (18, 18)
    S_ref, rhs_ref = np.zeros((18, 18)), st["rhs"].ravel()
    for k in range(3):
        S_ref[6 * k:6 * k + 6, 6 * k:6 * k + 6] = st["S"][k]
    print("pose-only: S %.3e of %.3e, rhs %.3e of %.3e; fixed cost %.15e / %.15e" % (np.abs(S - S_ref).max(), np.abs(S_ref).max(),
                                                                                     np.abs(rhs - rhs_ref).max(), np.abs(rhs_ref).max(),
                                                                                     res["fixed_cost"], fixed_ref))
    assert np.abs(S - S_ref).max() <= 1e-9 * np.abs(S_ref).max()
    assert np.abs(rhs - rhs_ref).max() <= 1e-9 * np.abs(rhs_ref).max()
    assert not S[S_ref == 0.0].any()
    assert np.isclose(info["cost"], prog_ref, rtol=1e-9)
    assert np.isclose(res["fixed_cost"], fixed_ref, rtol=1e-12)
    assert np.isclose(res["initial_cost"], prog_ref + fixed_ref, rtol=1e-9)
    assert res["num_residual_blocks"] == n_prog and res["num_residuals"] == n_prog * p.patch_len * p.channels
    assert res["final_cost"] < res["initial_cost"]
    for s in slots:
        assert cams_after[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()
    assert xyz_after.tobytes() == np.ascontiguousarray(p.xyz, np.float64).tobytes()


def test_structure_only_ignores_the_mask():
    p = _window5()
    o = default_solver_options(max_num_iterations=6)
    runs = []
    for slots in (None, (0, 3), range(5)):
        with _engine(p, fixed_slot=0) as e:
            e.set_cameras_constant()
            if slots is not None:
                e.set_cameras(p.cams, constant_slots=slots)      # (every slot: legal while a constant mode is on)
            runs.append(_strip(e.solve(o)))
    assert runs[0] == runs[1] == runs[2]


# ---- 6. inverse depths with two anchors ---------------------------------------------------------------------------------------------------
def test_inverse_depth_trace_matches_the_yardstick():
    name = "4x60-dense-r1-inverse-depth-anchors-0-3"
    p, slots, _, rays, rho = _case(name)
    res_ref, n_cmp = _yardstick(name)
    assert n_cmp >= 4 and res_ref["min_candidate"] > 0.0
    with _engine(p, slots=slots, keep=False, rays=rays, rho=rho) as e:
        res = e.solve(default_solver_options(max_num_iterations=n_cmp - 1))
        assert e.solve_driver() != "host-stepped"
        cams_after, x_after = e.get_state()
    _check_trace(name, res, res_ref, n_cmp, p, slots)
    cams_ref, x_ref = res_ref["states"][n_cmp - 1]
    print(name, "max parameter difference: cameras %.3e, inverse depths %.3e" % (np.abs(cams_after - cams_ref).max(),
                                                                                 np.abs(x_after[:, :1] - x_ref).max()))
    assert np.abs(cams_after - cams_ref).max() <= 1e-5 and np.abs(x_after[:, :1] - x_ref).max() <= 1e-5
    assert not x_after[:, 1:].any()
    for s in slots:
        assert cams_after[s].tobytes() == np.ascontiguousarray(p.cams[s], np.float64).tobytes()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    p = _window5()
    o = default_solver_options(max_num_iterations=5)
    with _engine(p, slots=(0, 4), keep=False) as e:
        fresh = _strip(e.solve(o))

    def solves_as_before(e):
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, constant_slots=(0, 4))
        assert _strip(e.solve(o)) == fresh

    # bits at or above n_frames; the engine keeps what it held
    with _engine(p, slots=(0, 4), keep=False) as e:
        with pytest.raises(EngineError, match="invalid argument.*anchor_mask 0x21 has bits at or above n_frames = 5"):
            e.set_cameras(p.cams, constant_slots=(0, 5))
        assert e.n_free == 3
        assert _strip(e.solve(o)) == fresh
    # every slot anchored in the full mode: the mask call second
    with _engine(p, slots=(0, 4), keep=False) as e:
        with pytest.raises(EngineError, match="invalid argument.*covers all 5 slots.*pba_set_cameras_constant"):
            e.set_cameras(p.cams, constant_slots=range(5))
        assert _strip(e.solve(o)) == fresh
    # ... legal while a constant mode is on, and then the switch back is what is refused (the mode switch second)
    for mode in ("set_cameras_constant", "set_points_constant"):
        with _engine(p, slots=(0, 4), keep=False) as e:
            getattr(e, mode)()
            e.set_cameras(p.cams, constant_slots=range(5))
            with pytest.raises(EngineError, match="invalid argument.*covers all 5 slots.*pba_set_cameras_constant"):
                getattr(e, mode)(False)
            e.set_cameras(p.cams, constant_slots=(0, 4))
            getattr(e, mode)(False)
            solves_as_before(e)
    # two or more anchors with a multi-rank transport, either order; one anchor goes through
    with _engine(p, slots=(0, 4), keep=False) as e:
        with pytest.raises(EngineError, match="invalid argument.*multi-rank solves take at most one constant slot"):
            e.comm_init_callback(lambda v, op: None, 0, 2)
        assert _strip(e.solve(o)) == fresh
    with _engine(p, fixed_slot=0, keep=False) as e:
        e.comm_init_callback(lambda v, op: None, 0, 2)
        with pytest.raises(EngineError, match="invalid argument.*2 constant slots: multi-rank solves .* at most one constant slot"):
            e.set_cameras(p.cams, constant_slots=(0, 4))
        e.set_cameras(p.cams, constant_slots=(3,))
        assert e.n_free == 4
    # ... and with the precision-sweep flags (the flags are set when the engine is created, so the mask call is always second)
    with _engine(p, fixed_slot=0, keep=False, precision="fp32") as e:
        with pytest.raises(EngineError, match="invalid argument.*2 constant slots: the precision-sweep sampler modes .* at most one"):
            e.set_cameras(p.cams, constant_slots=(0, 4))
        e.set_cameras(p.cams, constant_slots=(4,))
        assert e.solve(o)["final_cost"] > 0.0
    # a wide window keeps the wide refusals: inverse depths on 17 slots, however few cameras are free
    pw = cases.boundary_window(17)
    rays, rho = synthetic.inverse_depth_rays(pw)
    with _engine(pw, slots=range(16), keep=False) as e:
        with pytest.raises(EngineError, match="invalid argument.*inverse-depth mode is not built for wide windows"):
            e.set_inverse_depth(rays, rho)
    # the Python form: slots outside 0..31
    with _engine(p, fixed_slot=0, keep=False) as e:
        with pytest.raises(ValueError, match="constant_slots"):
            e.set_cameras(p.cams, constant_slots=(0, 32))


# ---- 8. the host class: Options::numConstantFrames -------------------------------------------------------------------------------------
SEQ_SIZE, SEQ_K = (120, 160), (200.0, 200.0, 80.0, 60.0)


def _sequence(n):
    """The synthetic sequence of tests/test_gpu_points_only.py: exactly photo-consistent frames, depth maps scaled by a smooth +-2 % field."""
    import host_class_probe
    imgs, depths, T_gt, local = host_class_probe.sequence(n, SEQ_SIZE, SEQ_K)
    rows, cols = depths[0].shape
    y, x = np.mgrid[0:rows, 0:cols]
    field = 1.0 + 0.02 * np.sin(2 * np.pi * x / cols) * np.cos(2 * np.pi * y / rows)
    return imgs, [np.where(z > 0, z * field, z).astype(np.float32) for z in depths], local


def test_host_class_leaves_the_anchor_frames_alone(tmp_path):
    import host_class_probe
    n, window = 8, 4
    imgs, depths, local = _sequence(n)
    probe = host_class_probe.HostClassProbe(tmp_path)
    runs = {}
    for key in (2, 1, None):
        probe.create(1, SEQ_SIZE, SEQ_K, window=window, radius=1, min_score=0.65, num_constant=key)
        out = [(i, probe.add(imgs[i], depths[i], local[i])) for i in range(n)]
        runs[key] = [(i, r) for i, r in out if r is not None]
        assert len(runs[key]) == n - (window - 1)
    probe.release()
    # 2: the two oldest poses of every window are byte-identical across the optimisation; the younger ones move
    moved = 0
    for (_, prev), (i, r) in zip(runs[2][:-1], runs[2][1:]):
        assert len(r["poses"]) == i + 1 and len(prev["poses"]) == i
        first = i - (window - 1)
        assert r["poses"][first:first + 2].tobytes() == prev["poses"][first:first + 2].tobytes(), i
        assert r["poses"][:first].tobytes() == prev["poses"][:first].tobytes()
        moved += int(r["poses"][first + 2].tobytes() != prev["poses"][first + 2].tobytes())
        assert r["fixed_cost"] == 0.0
    assert moved == len(runs[2]) - 1
    # 1 is the behaviour without the key, to the last bit
    assert len(runs[1]) == len(runs[None])
    for (_, a), (_, b) in zip(runs[1], runs[None]):
        assert a["poses"].tobytes() == b["poses"].tobytes()
    assert runs[2][-1][1]["poses"].tobytes() != runs[1][-1][1]["poses"].tobytes()


def test_run_kitti_runs_with_the_key(tmp_path):
    import host_class_probe
    run = os.path.join(host_class_probe.PKG, "bin", "run_kitti")
    n_frames = 8
    imgs, depths, local = _sequence(n_frames)
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

    out_2, res_2 = go("two", "numConstantFrames = 2\n")
    assert np.array(out_2.split(), np.float64).reshape(-1, 3, 4).shape[0] == n_frames
    out_1, res_1 = go("one", "numConstantFrames = 1\n")
    out_absent, res_absent = go("absent", "")
    assert (out_1, res_1) == (out_absent, res_absent)
    assert out_2 != out_1
    # -b with two such sequences writes what the solo run writes
    specs = []
    for name in ("batch-a", "batch-b"):
        d, cfg = prepare(name, "numConstantFrames = 2\n")
        specs.append((d, "%s:%s:%s" % (cfg, os.path.join(d, "refined.txt"), os.path.join(d, "results.txt"))))
    r = subprocess.run([run, "-p", "-b", specs[0][1], "-b", specs[1][1]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for d, _ in specs:
        assert read(d) == (out_2, res_2)
