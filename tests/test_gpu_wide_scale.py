"""-m gpu: wide windows (16 to 32 free cameras, csrc/pba_wide.h) at the sizes where the pair stage has more than one chunk per camera
pair.  The windows of test_gpu_wide_window.py have 100 to 400 points: their largest camera pair has ~200 co-observations, so every pair
is one chunk of k_wide_pairs (kWideChunk entries), one trip of its entry loop, and k_wide_assemble adds one chunk sum.  Here:

  window A  20 frames x 11 000 points, banded and trimmed: pairs of 2 chunks, a pair of exactly kWideChunk entries (a full chunk), one of
            kWideChunk + 1 (a second chunk of one entry), a diagonal pair of exactly 2 x kWideChunk, and pairs without a common point;
  window B  32 frames x 8 000 points, no constant camera (32 free cameras, n = 192);
  window C  17 frames x 5 000 points, 5x5 patches, the constant camera in the middle (slot 9) -- and swept over (0, 1, 9, 16, none);
  window D  the source of A as generated, the constant camera last (slot 19), Gaussian patch weights: pairs of 3 chunks;
  a BitPlanes (8 channels) window, a 7x7-patch window, and the operating point of tools/wide_window_timing.py: 17 frames x 50 000
  points at KITTI size (more than 128 point blocks and more than 128 cost blocks in the tail workgroup of k_wide_assemble).

The structure every test relies on is asserted where the window is built (wide_util.structure, from the generated observation lists
and kWideChunk as the header states it), so another generator, seed or chunk size that empties a case fails instead of passing.

The referee of the reduced system is gpu_util.block_step_full in x87 extended precision on the oracle's per-block products (point by point,
no dense Jacobian).  Tolerances: those of test_gpu_wide_window.py -- records and costs 1e-12 relative, S and rhs 1e-9 of the largest entry,
step accuracy <= 10 x the float64 band, LM traces through its _compare_traces, poses 1e-5.  These windows separate from the referee
within a few iterations (cond(S) 1e5 .. 4e6 from the second iteration on), so _compare_traces takes its referee branch; next to it every
cost on the engine's own path is held to the oracle's value at that state (trajectory_consistency, 1e-12: not chaotic).  The referee branch
runs with restated_twins = 3: on window D, the BitPlanes and the 7x7 window the engine left the referee sooner than the oracle's two
twins (1.05e-9 at iteration 5 against 2e-12), while each of its steps lay inside the float64 band of step_accuracy and an independently
written float64 loop left the referee by the same amounts -- the oracle's twins share one solver.

Cost blocks: the tail of k_wide_assemble takes a second trip through them above wide_util.cost_block_stride_obs() = 128 x 4 x 64 = 32 768
observations (the sampling grid has one workgroup per 256 observations).  Windows A (~80 000), B, C, D and the operating point (~415 000)
are above it, the BitPlanes and 7x7 windows below."""
import dataclasses
import functools
import time

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import imgproc, synthetic
from photobundle_amd.engine import Engine, default_solver_options

import gpu_util
import wide_util
from gpu_util import check_obs_records, step_accuracy, trajectory_consistency
from test_gpu_wide_window import _compare_traces, _its

pytestmark = pytest.mark.gpu
SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
MID = dict(size=(240, 320), K=(400.0, 400.0, 160.0, 120.0))


def _make(n_frames, n_points, radius, seed, **kw):
    p = synthetic.make_window(n_frames=n_frames, n_points=n_points, radius=radius, huber=0.05, visibility="causal", seed_offset=seed, **kw)
    assert len(np.unique(p.obs_slot)) == n_frames
    return p


@functools.lru_cache(maxsize=None)
def _source_a():
    return _make(20, 11000, 1, 1, **MID)


@functools.lru_cache(maxsize=None)
def _window(name):
    """Windows A to D with the structure they are here for (asserted).  Returns (problem, structure)."""
    chunk = wide_util.wide_chunk()
    if name == "A":
        src = _source_a()
        exact = wide_util.pick_exact_pairs(wide_util.co_observation_counts(wide_util.shape_window(src, band=9)), chunk)
        p = wide_util.shape_window(src, band=9, exact=exact)
        st = wide_util.structure(p, chunk)
        C = st["C"]
        (full, _), (plus1, _), (dia, _) = exact
        assert full[0] < full[1] and C[full] == chunk                    # an off-diagonal pair whose only chunk is exactly full
        assert plus1[0] < plus1[1] and C[plus1] == chunk + 1             # a second chunk of one entry
        assert dia[0] == dia[1] and C[dia] == 2 * chunk                  # a diagonal pair of two full chunks
        assert st["multi"] >= 40 and st["empty"] >= 30, st
        assert wide_util.obs_per_point(p).min() >= 3
    elif name == "B":
        p = _make(32, 8000, 1, 0, **MID)
        p.fixed_slot = -1
        st = wide_util.structure(p, chunk)
        assert len(st["C"]) == 32 and st["multi"] >= 100, st
    elif name == "C":
        p = _make(17, 5000, 2, 0, **MID)
        p.fixed_slot = 9
        st = wide_util.structure(p, chunk)
        assert len(st["C"]) == 16 and st["multi"] >= 30, st
    elif name == "D":
        src = _source_a()
        p = dataclasses.replace(src, cams=src.cams.copy(), xyz=src.xyz.copy(), fixed_slot=19,
                                weights=imgproc.make_patch_weights(src.radius, True))
        st = wide_util.structure(p, chunk)
        assert len(st["C"]) == 19 and st["max_chunks"] >= 3, st
    else:
        raise KeyError(name)
    assert p.n_obs > wide_util.cost_block_stride_obs()                   # (module docstring: the cost-block loop of the tail strides)
    assert st["largest"] > 256                                           # the entry loop of k_wide_pairs takes more than one trip
    assert p.n_points > 2 * 256                                          # k_wide_point: more than two workgroups
    print("WIDE-SCALE window %s: %d frames, %d points, %d observations, %d free cameras, pairs %d (2+ chunks %d, empty %d), largest pair %d"
          % (name, p.n_frames, p.n_points, p.n_obs, len(st["C"]), st["n_pairs"], st["multi"], st["empty"], st["largest"]))
    return p, st


def _referee(p):
    """Extended-precision reduced system and step statistics of a window at its initial state."""
    return gpu_util.block_step_full(p, oracle.block_products(p, autodiff=True, threads=8), 1e4, None, np.longdouble)


def _engine(p, keep=True):
    _, _, rows, cols = p.planes.shape
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, channels=getattr(p, "channels", 1))
    return e.load(p)


def _check_linearize(p, tag):
    with _engine(p) as e:
        cost = e.linearize()
        rec = e.obs_records()
    lin = oracle.linearize(p, blocks=False)
    print("WIDE-SCALE %s: cost %.10e, relative distance to the oracle %.2e" % (tag, cost, abs(cost - lin["cost"]) / lin["cost"]))
    assert np.isclose(cost, lin["cost"], rtol=1e-12)
    s = lin["block_sqnorm"]
    rho = np.where(s > p.huber ** 2, 2 * p.huber * np.sqrt(s) - p.huber ** 2, s) if p.huber > 0 else s      # Huber, as Ceres states it
    assert np.allclose(rec[:, 5], 0.5 * rho, rtol=1e-12, atol=0)
    worst = check_obs_records(p, rec, threads=8)
    print("WIDE-SCALE %s: worst record distances %s" % (tag, {k: "%.1e" % v for k, v in worst.items()}))


def _check_reduced_system(p, ref, tag):
    """Item 2: S, rhs and the step statistics of pba_step(1e4, init_scale) against the extended-precision referee; the blocks of camera
    pairs without a common point are exactly zero."""
    free = wide_util.free_slots(p)
    n = 6 * len(free)
    with _engine(p) as e:
        e.linearize()
        info = e.step(1e4, init_scale=True)
        S, rhs = e.reduced_system()
    S_ref, rhs_ref = ref["S"].astype(np.float64), ref["rhs"].astype(np.float64)
    assert S.shape == (n, n) and S_ref.shape == (n, n)
    d_S = np.abs(S - S_ref).max() / np.abs(S_ref).max()
    d_rhs = np.abs(rhs - rhs_ref).max() / np.abs(rhs_ref).max()
    print("WIDE-SCALE %s: S distance %.2e, rhs distance %.2e (of the largest entry)" % (tag, d_S, d_rhs))
    assert d_S <= 1e-9, d_S
    assert d_rhs <= 1e-9, d_rhs
    C = wide_util.co_observation_counts(p)
    n_empty = 0
    for a in range(len(free)):
        for b in range(a + 1, len(free)):
            if C[a, b] == 0:
                n_empty += 1
                assert not S[6 * a:6 * a + 6, 6 * b:6 * b + 6].any() and not S[6 * b:6 * b + 6, 6 * a:6 * a + 6].any(), (a, b)
                assert not S_ref[6 * a:6 * a + 6, 6 * b:6 * b + 6].any()
            else:
                assert S[6 * a:6 * a + 6, 6 * b:6 * b + 6].any(), (a, b)
    assert np.array_equal(S, S.T)
    assert info["linear_solver_ok"] and info["eval_ok"]
    assert np.isclose(info["gradient_max_norm"], ref["gradient_max_norm"], rtol=1e-10)
    assert np.isclose(info["gradient_norm"], ref["gradient_norm"], rtol=1e-10)
    assert np.isclose(info["model_cost_change"], ref["model_cost_change"], rtol=1e-7)
    assert np.isclose(info["step_norm"], ref["step_norm"], rtol=1e-7)
    return n_empty


def _check_solve(p, n_it, ks, tag):
    """Item 4: the LM trace against the oracle (_compare_traces; its referee branch where the traces separate), and every cost along the
    engine's own path against the oracle's value at that state (not chaotic: 1e-12)."""
    kw = dict(max_num_iterations=n_it)
    ref = oracle.solve(p, oracle.default_options(**kw))
    assert ref["final_cost"] < ref["iterations"][0]["cost"]
    with _engine(p, keep=False) as e:
        res = e.solve(default_solver_options(**kw))
        assert e.solve_driver() == "host-stepped"
        _compare_traces(p, res, ref, kw, restated_twins=3)
        if p.fixed_slot >= 0:
            assert np.array_equal(res["cams"][p.fixed_slot], p.cams[p.fixed_slot])
        free = wide_util.free_slots(p)
        assert (np.abs(res["cams"][free] - p.cams[free]).max(1) > 0).all()          # every free camera moved
        worst = trajectory_consistency(p, e, ks, lambda k: default_solver_options(max_num_iterations=k))
    d = [abs(a["cost"] - b["cost"]) / a["cost"] for a, b in zip(ref["iterations"], res["iterations"])]
    print("WIDE-SCALE %s: cost %.6e -> %.6e in %d iterations; distance to the double oracle per iteration %s; trajectory consistency %.1e"
          % (tag, res["iterations"][0]["cost"], res["final_cost"], len(res["iterations"]) - 1, ["%.1e" % x for x in d], worst))


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_linearize_and_records(name):
    _check_linearize(_window(name)[0], name)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_reduced_system_and_step(name):
    p, st = _window(name)
    n_empty = _check_reduced_system(p, _referee(p), name)
    iu = np.triu_indices(len(st["C"]))
    assert n_empty == st["empty"] == int((st["C"][iu] == 0).sum())
    if name == "A":
        assert n_empty >= 30


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_step_accuracy(name):
    p, _ = _window(name)
    for row in step_accuracy(p, 2):
        print("WIDE-SCALE %s step accuracy it %d: cond %.1e, backward engine %.2e / band %.2e, forward engine %.2e / band %.2e"
              % (name, row["it"], row["cond"], row["bwd_engine"], row["bwd_f64_band"], row["fwd_engine"], row["fwd_f64_band"]))
        assert row["bwd_engine"] <= 10.0 * row["bwd_f64_band"] + 1e-14, row
        assert row["fwd_engine"] <= 10.0 * row["fwd_f64_band"] + 1e-13, row


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_solve_matches_oracle(name):
    _check_solve(_window(name)[0], 8, (1, 3, 8), name)


@pytest.mark.parametrize("name", ["A", "B"])
def test_run_to_run_bits(name):
    """Chunk order is fixed: two fresh engines give the same bytes."""
    p, _ = _window(name)
    runs = []
    for _ in range(2):
        with _engine(p, keep=True) as e:
            e.linearize()
            e.step(1e4, init_scale=True)
            S, rhs = e.reduced_system()
            e.load(p)
            res = e.solve(default_solver_options(max_num_iterations=8))
            runs.append((S.tobytes(), rhs.tobytes(), res["cams"].tobytes(), res["xyz"].tobytes(), _its(res)))
    assert runs[0] == runs[1]
    assert len(runs[0][4]) >= 3


@pytest.mark.parametrize("fixed", [0, 1, 9, 16, -1])
def test_constant_slot_sweep(fixed):
    """The host (free_of in wide_prepare) and the device (CamGeom::free_index) each map slots to free indices; the constant slot of a
    sliding window moves through the ring.  Window C with the constant camera first, second, in the middle, last and absent."""
    src, _ = _window("C")
    p = dataclasses.replace(src, cams=src.cams.copy(), xyz=src.xyz.copy(), fixed_slot=fixed)
    st = wide_util.structure(p)
    assert len(st["C"]) == (17 if fixed < 0 else 16) and st["multi"] >= 30, st
    key = "C/fixed=%d" % fixed
    _check_linearize(p, key)
    _check_reduced_system(p, _referee(p), key)


def _small_checks(p, tag, n_it=5, ks=(1, 5)):
    _check_linearize(p, tag)
    _check_reduced_system(p, _referee(p), tag)
    _check_solve(p, n_it, ks, tag)


def test_bitplanes_window():
    """Eight descriptor channels (BitPlanes) on a wide window: only three channels are covered in test_gpu_wide_window.py."""
    p = _make(20, 3000, 1, 6, channel_fn=synthetic.channel_fn("BitPlanes"), **SMALL)
    assert p.channels == 8 and p.desc.shape[1] == 8 * 9
    st = wide_util.structure(p)
    assert st["largest"] > 256 and p.n_points > 2 * 256, st
    _small_checks(p, "BitPlanes")


def test_radius3_window():
    """7x7 patches at 24 frames (23 free cameras)."""
    p = _make(24, 1500, 3, 8, **SMALL)
    st = wide_util.structure(p)
    assert len(st["C"]) == 23 and st["largest"] > 256 and p.n_points > 2 * 256, st
    _small_checks(p, "radius 3")


@pytest.mark.timeout(2400)
def test_operating_point():
    """The first row of profiles/wide/timing.json: 17 frames x 50 000 points at KITTI size, 5x5 patches, causal.  More than 128 x 256 points:
    the point-block loop of k_wide_assemble's tail strides; ~415 000 observations: its cost-block loop strides (threshold 32 768) and
    every diagonal pair has ten or more chunks."""
    t0 = time.time()
    p = _make(17, 50000, 2, 0)
    st = wide_util.structure(p)
    assert p.n_points > 128 * 256
    assert p.n_obs > wide_util.cost_block_stride_obs()
    assert len(st["C"]) == 16 and st["multi"] >= 100 and st["max_chunks"] >= 10, {k: v for k, v in st.items() if k != "C"}
    print("WIDE-SCALE operating point: %d observations, %d chunks, pairs with 2+ chunks %d of %d, largest pair %d (generated in %.0f s)"
          % (p.n_obs, st["chunks"], st["multi"], st["n_pairs"], st["largest"], time.time() - t0))
    _small_checks(p, "operating point")
    print("WIDE-SCALE operating point: %.0f s" % (time.time() - t0))
