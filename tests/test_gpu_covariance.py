"""-m gpu: the covariance output (pba_covariance) against the extended-precision inverse of the yardstick's normal matrix
(tests/covariance_cases.py: reference, error measure in correlation units, the bar 10 x kappa x 1e-12 of every case)."""
import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options

import covariance_cases as cc

pytestmark = pytest.mark.gpu

PBA_ERR_INVALID, PBA_ERR_STATE, PBA_ERR_NUMERIC = -1, -4, -6
TIME_FIELDS = ("iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds", "total_time_in_seconds")
DRIVERS = {"resident": {"PBA_RESIDENT": "1"}, "pipelined": {"PBA_RESIDENT": "0"}, "host-stepped": {"PBA_ASYNC": "0"}}
# a unit-diagonal pivot is 1 minus squares of correlations; each correlation carries the record bar 1e-12 with the margin 10, a pivot
# of a 3 x 3 block has three such terms, doubled by the square, and the margin 10 again: 6e-10 absolute
POINT_PIVOT_ABS = 6e-10


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


def _engine(p, slots, keep=False, rays=None, rho=None, mode="full", precision="exact"):
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, precision=precision)
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    if rays is not None:
        e.set_inverse_depth(rays, rho)
    if mode == "pose":
        e.set_points_constant()
    elif mode == "structure":
        e.set_cameras_constant()
    e.set_cameras(p.cams, constant_slots=slots)
    return e


@functools.lru_cache(maxsize=None)
def _reference(name):
    return cc.full_reference(cc.window(name), cc.slots_of(name))


def _check_full(tag, p, slots, cov, ref):
    nc = ref["n_cam"]
    e_c, e_p = cc.correlation_error(cov["cam_cov"], ref["cam_cov"]), cc.correlation_error(cov["point_cov"], ref["point_cov"])
    d_piv = abs(cov["min_cam_pivot"] - ref["min_cam_pivot"]) / ref["min_cam_pivot"]
    print("%s: n %d, kappa %.3e, bar %.3e, camera %.3e (%.3f of the bar), points %.3e (%.3f), pivots %.6e / %.6e (rel %.1e), point pivots "
          "%.6e / %.6e" % (tag, nc, ref["kappa"], ref["bar"], e_c, e_c / ref["bar"], e_p, e_p / ref["bar"], cov["min_cam_pivot"],
                           ref["min_cam_pivot"], d_piv, cov["min_point_pivot"], ref["min_point_pivot"]))
    assert cov["cam_cov"].shape == (nc, nc) and cov["point_cov"].shape == (p.n_points, 3, 3)
    assert cov["cam_cov"].tobytes() == np.ascontiguousarray(cov["cam_cov"].T).tobytes()           # symmetric bit for bit
    assert cov["point_cov"].tobytes() == np.ascontiguousarray(cov["point_cov"].transpose(0, 2, 1)).tobytes()
    assert e_c <= ref["bar"] and e_p <= ref["bar"]
    assert cov["n_cam"] == nc and cov["point_dim"] == 3
    assert cov["num_residuals"] == p.n_obs * p.patch_len and cov["num_parameters"] == nc + 3 * p.n_points
    assert np.isclose(cov["cost"], ref["cost"], rtol=1e-9)
    assert d_piv <= 1e-6
    assert abs(cov["min_point_pivot"] - ref["min_point_pivot"]) <= POINT_PIVOT_ABS
    assert cov["failed_is_point"] == 0 and cov["failed_index"] == -1


# ---- 1. + 2. the full mode against the yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.FULL_CASES))
def test_full_mode_at_the_start(name):
    p, slots = cc.window(name), cc.slots_of(name)
    with _engine(p, slots) as e:
        _check_full(name, p, slots, e.covariance(), _reference(name))


@pytest.mark.parametrize("name", cc.TRACE_NAMES)
def test_full_mode_after_a_solve(name):
    """At the state pba_solve leaves (the Huber cases then have corrected blocks): the reference is linearised at pba_get_state."""
    p, slots = cc.window(name), cc.slots_of(name)
    with _engine(p, slots) as e:
        res = e.solve(default_solver_options(max_num_iterations=12))
        cov = e.covariance()
        cams, xyz = e.get_state()
    assert cams.tobytes() == res["cams"].tobytes() and xyz.tobytes() == res["xyz"].tobytes()
    _check_full(name + " after %d iterations" % len(res["iterations"]), p, slots, cov, cc.full_reference(p, slots, (cams, xyz)))


def _sparse_kappa(free, U, W, V):
    """2-norm condition number of the unit-diagonal H of a large window from its extreme eigenvalues (Lanczos; the smallest by
    shift-invert at zero)."""
    nc, n = 6 * len(free), 6 * len(free) + 3 * len(V)
    H = sp.lil_matrix((n, n))
    for a in range(len(free)):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = U[a]
    for i in range(len(V)):
        H[nc + 3 * i:nc + 3 * i + 3, nc + 3 * i:nc + 3 * i + 3] = V[i]
    for (a, i), w in W.items():
        H[6 * a:6 * a + 6, nc + 3 * i:nc + 3 * i + 3] = w
        H[nc + 3 * i:nc + 3 * i + 3, 6 * a:6 * a + 6] = w.T
    H = sp.csc_matrix(H)
    d = sp.diags(1 / np.sqrt(H.diagonal()))
    Hu = sp.csc_matrix(d @ H @ d)
    hi = spl.eigsh(Hu, k=1, which="LA", return_eigenvectors=False)[0]
    lo = spl.eigsh(Hu, k=1, sigma=0, which="LM", return_eigenvectors=False)[0]
    return float(hi / lo)


def test_full_mode_beyond_one_chunk_of_points():
    """3 dense frames, 2 100 points, anchors {0, 2}: more points than one workgroup pass of the pair stage (and than kWideChunk = 2 048
    co-observations of the one diagonal pair).  Reference at this size: the float64 Schur-form covariance from the block sums."""
    p = synthetic.make_window(n_frames=3, n_points=2100, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
    slots = (0, 2)
    free, U, W, V = cc.block_sums(p, slots)
    Scc, Spp, S = cc.schur_covariance(free, U, W, V)
    kappa = _sparse_kappa(free, U, W, V)
    bar = 10 * kappa * cc.RECORD_BAR
    piv = cc.min_pivot(S)
    with _engine(p, slots) as e:
        cov = e.covariance()
    e_c, e_p = cc.correlation_error(cov["cam_cov"], Scc), cc.correlation_error(cov["point_cov"], Spp)
    print("2100 points: kappa %.3e, bar %.3e, camera %.3e, points %.3e, pivot %.6e / %.6e" % (kappa, bar, e_c, e_p, cov["min_cam_pivot"], piv))
    assert kappa <= cc.KAPPA_MAX and piv >= cc.PIVOT_MIN
    assert e_c <= bar and e_p <= bar
    assert abs(cov["min_cam_pivot"] - piv) <= 1e-6 * piv
    assert cov["cam_cov"].tobytes() == np.ascontiguousarray(cov["cam_cov"].T).tobytes()


def test_point_seen_by_anchored_cameras_only_gets_its_own_inverse():
    """Anchors {0, 1, 2} of 5 causal slots; every third point keeps only its observations in the anchored slots: W_i is empty and
    Sigma_pp(i) = V_i^-1."""
    p = copy.copy(cc.window("5x60-causal-huber-anchors-0-1-2"))
    slots = (0, 1, 2)
    # (a point left with one observation would have a rank-2 block: only points with two anchored observations lose the others)
    has_anchor = np.bincount(p.obs_point[np.isin(p.obs_slot, slots)], minlength=p.n_points) >= 2
    only = np.zeros(p.n_points, bool)
    only[::3] = True
    only &= has_anchor
    keep = ~(only[p.obs_point] & ~np.isin(p.obs_slot, slots))
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    assert only.sum() >= 10 and len(np.unique(p.obs_point)) == p.n_points
    assert (np.bincount(p.obs_point, minlength=p.n_points)[only] >= 2).all()
    assert not np.isin(p.obs_slot[only[p.obs_point]], (3, 4)).any()
    ref = cc.full_reference(p, slots)
    assert ref["kappa"] <= cc.KAPPA_MAX and ref["min_cam_pivot"] >= cc.PIVOT_MIN
    with _engine(p, slots) as e:
        cov = e.covariance()
    _check_full("points of anchored cameras only", p, slots, cov, ref)
    Pv = cc.structure_reference(p)[0]
    assert cc.correlation_error(cov["point_cov"][only], Pv[only]) <= ref["bar"]


# ---- 3. the two constant modes ---------------------------------------------------------------------------------------------------------
def test_pose_only_mode():
    name = "5x60-causal-huber-anchors-0-4"
    p, slots = cc.window(name), (0, 3)
    cols, ref, U, cost = cc.pose_reference(p, slots)
    kappa = max(np.linalg.cond(cc.unit_diagonal(u)[0]) for u in U)
    bar = 10 * kappa * cc.RECORD_BAR
    piv = min(cc.min_pivot(u) for u in U)
    with _engine(p, slots, mode="pose") as e:
        cov = e.covariance(points=False)
        with pytest.raises(EngineError, match="point_cov must be NULL") as ei:
            e.covariance()
        assert ei.value.status == PBA_ERR_INVALID
    err = cc.correlation_error(cov["cam_cov"], ref)
    print("pose-only: columns %r, kappa %.3e, bar %.3e, error %.3e, pivot %.6e / %.6e" % (cols, kappa, bar, err, cov["min_cam_pivot"], piv))
    assert cols == [1, 2, 4] and cov["n_cam"] == 18 and cov["point_dim"] == 0 and cov["point_cov"] is None
    assert err <= bar
    off = cov["cam_cov"].copy()
    for k in range(3):
        off[6 * k:6 * k + 6, 6 * k:6 * k + 6] = 0
    assert not off.any()                                                    # block diagonal, exact zeros
    assert cov["cam_cov"].tobytes() == np.ascontiguousarray(cov["cam_cov"].T).tobytes()
    in_program = ~np.isin(p.obs_slot, slots)
    assert cov["num_residuals"] == int(in_program.sum()) * p.patch_len and cov["num_parameters"] == 18
    assert np.isclose(cov["cost"], cost, rtol=1e-9)
    assert abs(cov["min_cam_pivot"] - piv) <= 1e-6 * piv and cov["min_point_pivot"] == 1.0


def _check_structure(tag, p, cov, ref, V, cost, dim):
    kappa = max(np.linalg.cond(cc.unit_diagonal(v)[0]) for v in V)
    bar = 10 * kappa * cc.RECORD_BAR
    got = cov["point_cov"][:, :dim, :dim]
    err = cc.correlation_error(got, ref)
    piv = min(cc.min_pivot(v) for v in V)
    print("%s: kappa %.3e, bar %.3e, error %.3e, pivot %.6e / %.6e" % (tag, kappa, bar, err, cov["min_point_pivot"], piv))
    assert err <= bar
    rest = cov["point_cov"].copy()
    rest[:, :dim, :dim] = 0
    assert not rest.any()
    assert cov["cam_cov"] is None and cov["n_cam"] == 0 and cov["point_dim"] == dim and cov["min_cam_pivot"] == 1.0
    assert cov["num_residuals"] == p.n_obs * p.patch_len and cov["num_parameters"] == dim * p.n_points
    assert np.isclose(cov["cost"], cost, rtol=1e-9)
    assert abs(cov["min_point_pivot"] - piv) <= POINT_PIVOT_ABS


@pytest.mark.parametrize("n_points", cc.EDGE_POINTS)
def test_structure_only_mode_world_points(n_points):
    p = synthetic.make_window(n_frames=3, n_points=n_points, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
    ref, V, cost = cc.structure_reference(p)
    with _engine(p, (0,), mode="structure") as e:
        cov = e.covariance(cameras=False)
        with pytest.raises(EngineError, match="cam_cov must be NULL") as ei:
            e.covariance()
        assert ei.value.status == PBA_ERR_INVALID
    _check_structure("structure-only, %d points" % n_points, p, cov, ref, V, cost, 3)


@pytest.mark.parametrize("n_points", cc.EDGE_POINTS)
def test_structure_only_mode_inverse_depths(n_points):
    p = synthetic.make_window(n_frames=3, n_points=n_points, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
    rays, rho = synthetic.inverse_depth_rays(p)
    ref, V, cost = cc.structure_reference(p, rays, rho)
    with _engine(p, (0,), rays=rays, rho=rho, mode="structure") as e:
        cov = e.covariance(cameras=False)
    _check_structure("structure-only with inverse depths, %d points" % n_points, p, cov, ref, V, cost, 1)


# ---- 4. rank deficiency ----------------------------------------------------------------------------------------------------------------
def _rank_deficient_outcome(tag, e, n_points):
    """PBA_ERR_NUMERIC with nothing returned, or success with a pivot below 1e-9.  Never a fault."""
    try:
        cov = e.covariance()
    except EngineError as err:
        print("%s: %s; info %r" % (tag, err, err.info))
        assert err.status == PBA_ERR_NUMERIC
        assert err.info["failed_index"] >= 0
        return None
    print("%s: passed by rounding, pivots camera %.3e point %.3e" % (tag, cov["min_cam_pivot"], cov["min_point_pivot"]))
    assert min(cov["min_cam_pivot"], cov["min_point_pivot"]) < 1e-9
    return cov


@pytest.mark.parametrize("name", sorted(cc.ONE_ANCHOR))
def test_one_anchor_windows_report_the_open_gauge(name):
    p, slots = cc.window(name), cc.slots_of(name)
    with _engine(p, slots) as e:
        _rank_deficient_outcome(name, e, p.n_points)
        # ... and the engine solves as before afterwards
        res = e.solve(default_solver_options(max_num_iterations=3))
        assert len(res["iterations"]) >= 2


def test_one_point_window_is_singular_by_counting():
    p = synthetic.make_window(**cc.ONE_POINT)
    with _engine(p, (0, 2)) as e:
        _rank_deficient_outcome("one point, one free camera", e, 1)


def test_outputs_are_untouched_after_a_numeric_failure():
    """Through the C call: the caller's buffers keep their bytes when the status is PBA_ERR_NUMERIC."""
    import ctypes as C
    from photobundle_amd import _lib
    p = synthetic.make_window(**cc.ONE_POINT)
    with _engine(p, (0, 2)) as e:
        cam = np.full((6, 6), 7.25)
        pts = np.full((1, 9), -3.5)
        info = _lib.CovarianceInfo()
        rc = e._L.pba_covariance(e._h, cam.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), C.byref(info))
        print("one point: status %d, min pivots %.3e %.3e, failed %d %d" % (rc, info.min_cam_pivot, info.min_point_pivot, info.failed_is_point,
                                                                            info.failed_index))
        if rc == PBA_ERR_NUMERIC:
            assert (cam == 7.25).all() and (pts == -3.5).all()
            assert info.failed_index >= 0
        else:
            assert rc == 0 and min(info.min_cam_pivot, info.min_point_pivot) < 1e-9


@pytest.mark.parametrize("name", ["32-slots-anchor-0", "5x60-causal-huber-anchor-0"])
def test_raw_call_keeps_the_callers_bytes_on_a_gauge_open_window(name):
    """The C call itself with poisoned caller buffers on one-anchor windows (n = 186 and n = 24): whatever the status, PBA_ERR_NUMERIC
    leaves every byte, and success comes with a pivot below 1e-9."""
    import ctypes as C
    from photobundle_amd import _lib
    p, slots = cc.window(name), cc.slots_of(name)
    n = 6 * (p.n_frames - len(slots))
    with _engine(p, slots) as e:
        cam = np.full((n, n), 7.25)
        pts = np.full((p.n_points, 9), -3.5)
        info = _lib.CovarianceInfo()
        rc = e._L.pba_covariance(e._h, cam.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), C.byref(info))
        print("%s: status %d, n_cam %d, min pivots %.3e %.3e, failed %d %d" % (name, rc, info.n_cam, info.min_cam_pivot, info.min_point_pivot,
                                                                             info.failed_is_point, info.failed_index))
        assert info.n_cam == n
        if rc == PBA_ERR_NUMERIC:
            assert (cam == 7.25).all() and (pts == -3.5).all()
            assert info.failed_is_point == 0 and 0 <= info.failed_index < n
        else:
            assert rc == 0 and info.min_cam_pivot < 1e-9


def test_structure_only_point_with_a_single_observation():
    """One point keeps a single observation: its V has rank 2.  PBA_ERR_NUMERIC, failed_is_point = 1 and that point's index."""
    p = copy.copy(synthetic.make_window(n_frames=3, n_points=65, radius=1, size=(96, 128), K=(160.0, 160.0, 64.0, 48.0)))
    victim = 37
    first = np.flatnonzero(p.obs_point == victim)[0]
    keep = (p.obs_point != victim)
    keep[first] = True
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    assert (p.obs_point == victim).sum() == 1
    with _engine(p, (0,), mode="structure") as e:
        with pytest.raises(EngineError) as ei:
            e.covariance(cameras=False)
        print("single observation: %s; info %r" % (ei.value, ei.value.info))
        assert ei.value.status == PBA_ERR_NUMERIC
        assert ei.value.info["failed_is_point"] == 1 and ei.value.info["failed_index"] == victim


# ---- 5. non-interference ----------------------------------------------------------------------------------------------------------------
def _strip(res):
    out = {k: v for k, v in res.items() if k not in TIME_FIELDS and k not in ("iterations", "cams", "xyz")}
    its = [{k: v for k, v in it.items() if k not in TIME_FIELDS} for it in res["iterations"]]
    return out, its, res["cams"].tobytes(), res["xyz"].tobytes()


NARROW, WIDE = "5x60-causal-huber-anchors-0-4", "17-slots-anchors-0-1"
_SHAPES = [(NARROW, "resident"), (NARROW, "pipelined"), (NARROW, "host-stepped"), (WIDE, "host-stepped")]


@pytest.mark.parametrize("name,driver", _SHAPES)
def test_solve_then_covariance_leaves_the_state(name, driver):
    p, slots = cc.window(name), cc.slots_of(name)
    o = default_solver_options(max_num_iterations=6)
    with _env(DRIVERS[driver]):
        with _engine(p, slots) as a, _engine(p, slots) as b:
            ra, rb = a.solve(o), b.solve(o)
            assert a.solve_driver() == b.solve_driver() == driver
            a.covariance()
            assert a.solve_driver() == driver
            ca, xa = a.get_state()
            assert ca.tobytes() == ra["cams"].tobytes() == rb["cams"].tobytes() and xa.tobytes() == ra["xyz"].tobytes() == rb["xyz"].tobytes()
            # a second solve of the re-loaded problem equals that of the engine that never called covariance
            for e in (a, b):
                e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
                e.set_cameras(p.cams, constant_slots=slots)
            assert _strip(a.solve(o)) == _strip(b.solve(o))
            # ... and so does a solve that goes on from where the first ended
            assert _strip(a.solve(o)) == _strip(b.solve(o))


@pytest.mark.parametrize("name", [NARROW, WIDE])
def test_linearize_covariance_step_equals_linearize_step(name):
    p, slots = cc.window(name), cc.slots_of(name)
    with _engine(p, slots, keep=True) as a, _engine(p, slots, keep=True) as b:
        ca, cb = a.linearize(), b.linearize()
        a.covariance()
        ia, ib = a.step(1e4, init_scale=True), b.step(1e4, init_scale=True)
        assert ca == cb and ia == ib
        (Sa, ra), (Sb, rb) = a.reduced_system(), b.reduced_system()
        assert Sa.tobytes() == Sb.tobytes() and ra.tobytes() == rb.tobytes()
        # a second, re-solved step (the scales fixed at the first) and the accepted state
        a.covariance()
        assert a.step(1e2) == b.step(1e2)
        a.accept(); b.accept()
        assert a.get_state()[0].tobytes() == b.get_state()[0].tobytes() and a.get_state()[1].tobytes() == b.get_state()[1].tobytes()


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [NARROW, "32-slots-anchors-0-31"])
def test_two_fresh_engines_give_the_same_bits(name):
    p, slots = cc.window(name), cc.slots_of(name)
    out = []
    for _ in range(2):
        with _engine(p, slots) as e:
            out.append(e.covariance())
    a, b = out
    assert a["cam_cov"].tobytes() == b["cam_cov"].tobytes() and a["point_cov"].tobytes() == b["point_cov"].tobytes()
    assert {k: v for k, v in a.items() if k not in ("cam_cov", "point_cov")} == {k: v for k, v in b.items() if k not in ("cam_cov", "point_cov")}


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was():
    p, slots = cc.window(NARROW), cc.slots_of(NARROW)
    o = default_solver_options(max_num_iterations=5)
    with _engine(p, slots) as plain:
        want = _strip(plain.solve(o))

    def refused(e, match, status=PBA_ERR_INVALID, **kw):
        with pytest.raises(EngineError, match=match) as ei:
            e.covariance(**kw)
        assert ei.value.status == status

    # a free camera of the full mode without a residual block: the message names the slot
    q = copy.copy(p)
    keep = q.obs_slot != 2
    q.obs_point, q.obs_slot = q.obs_point[keep], q.obs_slot[keep]
    assert len(np.unique(q.obs_point)) == q.n_points
    with _engine(q, slots) as e:
        refused(e, "slot 2 has no residual block")
        assert len(e.solve(o)["iterations"]) >= 2
    # the precision-sweep flags (unit patch weights: the cases' own)
    with _engine(p, (0,), precision="fp32") as e:
        refused(e, "precision-sweep")
    # the inverse-depth parameterisation in the full mode
    pi = cc.window(cc.INVERSE_DEPTH)
    rays, rho = synthetic.inverse_depth_rays(pi)
    with _engine(pi, (0, 3), rays=rays, rho=rho) as e:
        refused(e, "inverse-depth")
        assert len(e.solve(default_solver_options(max_num_iterations=3))["iterations"]) >= 2
    # multi-rank engines (a transport takes at most one constant slot, so a one-anchor window; the refusal comes before any launch and
    # before the gauge could matter); afterwards the engine solves as one with the same transport that never asked
    with _engine(p, (0,)) as e, _engine(p, (0,)) as twin:
        for x in (e, twin):
            x.comm_init_callback(lambda v, op: None, 0, 2)
        refused(e, "multi-rank")
        o3 = default_solver_options(max_num_iterations=3)
        assert _strip(e.solve(o3)) == _strip(twin.solve(o3))
    # call order: PBA_ERR_STATE as pba_linearize gives it
    _, _, rows, cols = p.planes.shape
    with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber) as e:
        refused(e, "call order violated", status=PBA_ERR_STATE)
    # the constant families, then the engine solves as the plain one does
    with _engine(p, slots) as e:
        e.set_points_constant()
        refused(e, "point_cov must be NULL")
        e.set_points_constant(False)
        e.set_cameras_constant()
        refused(e, "cam_cov must be NULL")
        e.set_cameras_constant(False)
        e.set_cameras(p.cams, constant_slots=slots)
        assert _strip(e.solve(o)) == want


# ---- 8. the host classes ------------------------------------------------------------------------------------------------------------------
SEQ_SIZE, SEQ_K = (120, 160), (200.0, 200.0, 80.0, 60.0)


@functools.lru_cache(maxsize=None)
def _sequence(n):
    """The synthetic sequence of tests/test_gpu_anchors.py: exactly photo-consistent frames, depth maps scaled by a smooth +-2 % field."""
    import host_class_probe
    imgs, depths, T_gt, local = host_class_probe.sequence(n, SEQ_SIZE, SEQ_K)
    rows, cols = depths[0].shape
    y, x = np.mgrid[0:rows, 0:cols]
    field = 1.0 + 0.02 * np.sin(2 * np.pi * x / cols) * np.cos(2 * np.pi * y / rows)
    return imgs, [np.where(z > 0, z * field, z).astype(np.float32) for z in depths], local


def test_add_frame_with_compute_covariance(tmp_path):
    import covariance_class_probe
    n, window = 8, 4
    imgs, depths, local = _sequence(n)
    probe = covariance_class_probe.CovarianceClassProbe(tmp_path)
    runs = {}
    for on in (True, False):
        probe.create(SEQ_SIZE, SEQ_K, window=window, radius=1, min_score=0.65, num_constant=2, compute_covariance=on)
        out = [(i, probe.add(imgs[i], depths[i], local[i])) for i in range(n)]
        runs[on] = [(i, r) for i, r in out if r is not None]
        assert len(runs[on]) == n - (window - 1)
    probe.release()
    n_point_blocks = 0
    for (i, a), (_, b) in zip(runs[True], runs[False]):
        # poses and points are byte-identical to the run without the option
        assert a["poses"].tobytes() == b["poses"].tobytes() and a["refined"].tobytes() == b["refined"].tobytes()
        assert not b["covariance_ok"] and b["frame_ids"] == [] and b["pose_cov"].size == 0 and len(b["point_cov"]) == 0
        assert a["covariance_ok"], a["message"]
        first = i - (window - 1)
        assert a["frame_ids"] == [first + 2, first + 3]                       # the free frames, ascending
        C6 = a["pose_cov"]
        assert C6.shape == (12, 12) and C6.tobytes() == np.ascontiguousarray(C6.T).tobytes()
        assert np.linalg.eigvalsh(cc.unit_diagonal(C6)[0]).min() > 0           # symmetric positive definite
        assert 0 < a["min_camera_pivot"] <= 1 and 0 < a["min_point_pivot"] <= 1
        assert len(a["point_cov"]) == len(a["refined"])
        for blk in a["point_cov"]:
            if blk.any():                                                     # (all-zero: the point was not in the optimisation)
                n_point_blocks += 1
                assert blk.tobytes() == np.ascontiguousarray(blk.T).tobytes() and np.linalg.eigvalsh(cc.unit_diagonal(blk)[0]).min() > 0
        print("frame %d: pivots %.3e %.3e, sigma of the youngest frame's translation %r, %d points left" % (
            i, a["min_camera_pivot"], a["min_point_pivot"], np.sqrt(np.diag(C6)[9:12]), len(a["refined"])))
    assert n_point_blocks > 0


def test_track_frame_with_compute_covariance(tmp_path):
    import covariance_class_probe
    n, window = 6, 4
    imgs, depths, local = _sequence(n)
    probe = covariance_class_probe.CovarianceClassProbe(tmp_path)
    probe.create(SEQ_SIZE, SEQ_K, window=window, radius=1, min_score=0.65, num_constant=1)
    for i in range(n - 1):
        probe.add(imgs[i], depths[i], local[i])
    T_with, r_with = probe.track(imgs[n - 1], local[n - 1], True)
    T_without, r_without = probe.track(imgs[n - 1], local[n - 1], False)
    probe.release()
    assert r_with["tracked"] and r_without["tracked"]
    assert T_with.tobytes() == T_without.tobytes()
    assert not r_without["covariance_ok"] and not r_without["covariance"].any()
    C6 = r_with["covariance"]
    print("trackFrame: pivot %.3e, sigmas %r" % (r_with["min_pivot"], np.sqrt(np.diag(C6))))
    assert r_with["covariance_ok"] and 0 < r_with["min_pivot"] <= 1
    assert C6.tobytes() == np.ascontiguousarray(C6.T).tobytes() and np.linalg.eigvalsh(cc.unit_diagonal(C6)[0]).min() > 0


def test_run_kitti_with_the_key_runs_to_the_same_trajectory(tmp_path):
    import subprocess
    import host_class_probe
    run = os.path.join(host_class_probe.PKG, "bin", "run_kitti")
    imgs, depths, local = _sequence(8)
    common = "maxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\nnumConstantFrames = 2\n"
    out = {}
    for name, extra in (("with", "computeCovariance = 1\n"), ("without", "")):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        host_class_probe.write_sequence(d, imgs, depths, SEQ_K, local)
        cfg = os.path.join(d, "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n%s%s" % (d, d, common, extra))
        r = subprocess.run([run, "-c", cfg, "-o", os.path.join(d, "refined.txt"), "-r", os.path.join(d, "results.txt"), "-p"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = (open(os.path.join(d, "refined.txt"), "rb").read(), open(os.path.join(d, "results.txt"), "rb").read())
    assert out["with"] == out["without"] and len(out["with"][0]) > 0
