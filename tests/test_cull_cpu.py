"""CPU side of the outlier culling (include/pba.h "outlier culling"): the ABI, the numpy restatement of the rule against hand-written
cases, the class's five keys, and what the step is for -- on the CPU yardstick a window with an occluder ends closer to the ground
truth after solve -> cull -> solve than after the solve alone."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cull_cases as cc
from photobundle_amd import _lib, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_mirrored():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"int\s+pba_get_block_costs\s*\(\s*pba_engine\s*\*\s*e\s*,\s*double\s*\*\s*cost[^)]*\)\s*;", header)
    assert re.search(r"int\s+pba_cull\s*\(\s*pba_engine\s*\*\s*e\s*,\s*const\s+pba_cull_options\s*\*\s*o\s*,\s*uint8_t\s*\*\s*block_keep[^;]*"
                     r"int32_t\s*\*\s*point_map[^;]*pba_cull_info\s*\*\s*info[^;]*\)\s*;", header)
    for name in ("pba_cull", "pba_get_block_costs"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert hasattr(L, "pba_internal_select_u64order") and "pba_internal_select_u64order" not in header
    assert [f for f, _ in _lib.CullOptions._fields_] == ["min_cost", "factor", "quantile", "min_observations", "apply"]
    assert [f for f, _ in _lib.CullInfo._fields_] == ["n_blocks_before", "n_blocks_after", "n_points_before", "n_points_after", "n_blocks_over_threshold",
                                                     "n_blocks_by_point_rule", "quantile_cost", "threshold", "applied"]


def test_struct_sizes_match_the_header():
    src = ('#include "pba.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pba_cull_options), '
           'offsetof(pba_cull_options, min_observations), sizeof(pba_cull_info), offsetof(pba_cull_info, n_blocks_by_point_rule), '
           'offsetof(pba_cull_info, quantile_cost), offsetof(pba_cull_info, applied)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), c])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    O, I = _lib.CullOptions, _lib.CullInfo
    assert got == [C.sizeof(O), O.min_observations.offset, C.sizeof(I), I.n_blocks_by_point_rule.offset, I.quantile_cost.offset, I.applied.offset]
    assert C.sizeof(O) == 3 * 8 + 2 * 4 and C.sizeof(I) == 6 * 4 + 2 * 8 + 4 + 4      # (4 bytes of tail padding)


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    o, info, buf = _lib.CullOptions(0.0, 0.0, 0.5, 2, 0), _lib.CullInfo(), (C.c_double * 4)()
    assert L.pba_cull(None, C.byref(o), None, None, C.byref(info)) == -1       # PBA_ERR_INVALID
    assert L.pba_get_block_costs(None, buf) == -1
    assert L.pba_internal_select_u64order(None, buf, 4, 0, C.byref(C.c_double())) == -1


# ---- the rule, by hand ---------------------------------------------------------------------------------------------------------------
def _cull(c, obs_point, **kw):
    keep, pmap, info = cc.reference_cull(np.array(c, np.float64), obs_point, **kw)
    return list(keep), list(pmap), info


def test_a_tie_at_the_threshold_is_kept():
    # threshold = min_cost = 2: the blocks at exactly 2 stay, 2 + 1 ulp goes
    c = [1.0, 2.0, 2.0, np.nextafter(2.0, 3.0), 0.5, 2.0]
    keep, pmap, info = _cull(c, [0, 0, 1, 1, 2, 2], min_cost=2.0, factor=0.0, min_observations=1)
    assert keep == [1, 1, 1, 0, 1, 1] and pmap == [0, 1, 2]
    assert info["threshold"] == 2.0 and info["n_blocks_over_threshold"] == 1 and info["n_blocks_by_point_rule"] == 0 and info["n_blocks_after"] == 5
    # ... and through the quantile: factor 1 x the median (k = floor(0.5 * 5) = 2 -> sorted[2] = 2.0)
    keep, _, info = _cull(c, [0, 0, 1, 1, 2, 2], factor=1.0, quantile=0.5, min_observations=1)
    assert info["quantile_cost"] == 2.0 and info["threshold"] == 2.0 and keep == [1, 1, 1, 0, 1, 1]


def test_nan_and_inf_costs_are_always_over_and_order_last():
    c = [1.0, NAN, INF, 3.0, 2.0, NAN]
    obs_point = [0, 0, 1, 1, 2, 2]
    keep, pmap, info = _cull(c, obs_point, min_cost=1e300, factor=0.0, min_observations=1)
    assert keep == [1, 0, 0, 1, 1, 0] and pmap == [0, 1, 2] and info["n_blocks_over_threshold"] == 3
    # order by bit pattern: 1 2 3 inf nan nan -- quantile 0.6 -> k = 3 -> +inf, and factor * inf is the numeric error
    assert cc.u64_order_statistic(c, 3) == INF and np.isnan(cc.u64_order_statistic(c, 4)) and cc.u64_order_statistic(c, 2) == 3.0
    with pytest.raises(cc.CullNumericError):
        _cull(c, obs_point, factor=1.0, quantile=0.6)
    with pytest.raises(cc.CullNumericError):
        _cull(c, obs_point, factor=1.0, quantile=1.0)       # NaN
    # min_observations = 2: every point has one block over, so every point leaves
    keep, pmap, info = _cull(c, obs_point, min_cost=1e300, factor=0.0, min_observations=2)
    assert keep == [0] * 6 and pmap == [-1] * 3 and info["n_blocks_by_point_rule"] == 3 and info["n_points_after"] == 0


def test_quantile_zero_and_one():
    c = [4.0, 1.0, 3.0, 2.0]
    obs_point = [0, 0, 1, 1]
    _, _, lo = _cull(c, obs_point, factor=1.0, quantile=0.0, min_observations=1)
    _, _, hi = _cull(c, obs_point, factor=1.0, quantile=1.0, min_observations=1)
    assert lo["quantile_cost"] == 1.0 and lo["n_blocks_after"] == 1 and hi["quantile_cost"] == 4.0 and hi["n_blocks_after"] == 4
    # k = floor(q (n - 1)): 0.34 * 3 = 1.02 -> 1, 0.33 * 3 = 0.99 -> 0
    assert _cull(c, obs_point, factor=1.0, quantile=0.34)[2]["quantile_cost"] == 2.0 and _cull(c, obs_point, factor=1.0, quantile=0.33)[2]["quantile_cost"] == 1.0
    # the floor: factor x quantile below min_cost
    assert _cull(c, obs_point, min_cost=3.5, factor=1.0, quantile=0.0)[2]["threshold"] == 3.5


def test_factor_zero_ignores_the_quantile():
    c = [4.0, 1.0, 3.0, INF]
    keep, _, info = _cull(c, [0, 0, 1, 1], min_cost=3.0, factor=0.0, quantile=1.0, min_observations=1)
    assert info["threshold"] == 3.0 and info["quantile_cost"] == INF and keep == [0, 1, 1, 0]


def test_a_point_at_exactly_min_observations_stays():
    c = [1.0, 1.0, 9.0, 1.0, 9.0, 9.0, 1.0, 1.0, 1.0]
    obs_point = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    keep, pmap, info = _cull(c, obs_point, min_cost=5.0, factor=0.0, min_observations=2)
    assert keep == [1, 1, 0, 0, 0, 0, 1, 1, 1] and pmap == [0, -1, 1]      # point 0 keeps exactly 2, point 1 only 1
    assert info["n_blocks_over_threshold"] == 3 and info["n_blocks_by_point_rule"] == 1 and info["n_points_after"] == 2 and info["n_blocks_after"] == 5
    keep, pmap, _ = _cull(c, obs_point, min_cost=5.0, factor=0.0, min_observations=3)
    assert keep == [0, 0, 0, 0, 0, 0, 1, 1, 1] and pmap == [-1, -1, 0]


def test_everything_culled():
    keep, pmap, info = _cull([2.0, 3.0, 4.0], [0, 0, 1], min_cost=1.0, factor=0.0, min_observations=1)
    assert keep == [0, 0, 0] and pmap == [-1, -1] and info["n_blocks_after"] == 0 and info["n_points_after"] == 0
    assert info["n_blocks_over_threshold"] == 3 and info["n_blocks_by_point_rule"] == 0


# ---- the class ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import cull_class_probe
    return cull_class_probe.CullClassProbe(tmp_path_factory.mktemp("cull_probe"))


def test_class_fields_defaults_and_keys(probe):
    header = open(os.path.join(ROOT, "photobundle_amd", "host", "photobundle.h")).read()
    for field in ("int outlierPasses = 0;", "double outlierQuantile = 0.5;", "double outlierFactor = 3.0;", "double outlierMinCost = 0.0;",
                  "int outlierMinObservations = 2;", "int numCulledBlocks = 0, numCulledPoints = 0;"):
        assert field in header, field
    assert header.count("int outlierPasses = 0;") == 2 and header.count("int numCulledBlocks = 0, numCulledPoints = 0;") == 2      # + TrackOptions / TrackResult
    assert probe.defaults() == ((0.0, 0.5, 3.0, 0.0, 2.0), 0)
    text = probe.parse_and_print("slidingWindowSize = 4\n")
    for line in ("outlierPasses = 0\n", "outlierQuantile = 0.5\n", "outlierFactor = 3\n", "outlierMinCost = 0\n", "outlierMinObservations = 2\n"):
        assert line in text, line
    text = probe.parse_and_print("outlierPasses = 2\noutlierQuantile = 0.75\noutlierFactor = 2.5\noutlierMinCost = 0.125\noutlierMinObservations = 3\n")
    for line in ("outlierPasses = 2\n", "outlierQuantile = 0.75\n", "outlierFactor = 2.5\n", "outlierMinCost = 0.125\n", "outlierMinObservations = 3\n"):
        assert line in text, line
    assert probe.parse_and_print(text) == text      # the output of one run configures the next


def test_constructor_refuses_out_of_range_values(probe):
    size, K = (96, 128), (160.0, 160.0, 64.0, 48.0)
    for kw, match in ((dict(passes=-1), "outlierPasses = -1"), (dict(passes=1, quantile=1.5), "outlierQuantile = 1.5"),
                      (dict(passes=1, quantile=NAN), "outlierQuantile"), (dict(passes=1, factor=-1.0), "outlierFactor = -1"),
                      (dict(passes=1, factor=INF), "outlierFactor"), (dict(passes=1, min_cost=-0.5), "outlierMinCost = -0.5"),
                      (dict(passes=1, min_cost=INF), "outlierMinCost"), (dict(passes=1, min_observations=0), "outlierMinObservations = 0")):
        with pytest.raises(RuntimeError, match=match):
            probe.create(size, K, window=5, radius=1, **kw)
    import torch
    if not torch.cuda.is_available():
        # values in range pass the checks, and the four companions are not read while the passes are off: the constructor gets as far as the device
        for kw in (dict(passes=1), dict(passes=0, quantile=7.0, factor=-1.0, min_cost=-1.0, min_observations=0)):
            with pytest.raises(RuntimeError, match="pba_create"):
                probe.create(size, K, window=5, radius=1, **kw)


def test_run_kitti_reads_the_keys(tmp_path):
    """run_kitti on a one-frame sequence with every device hidden: the range check comes before any device call."""
    import host_class_probe
    run = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    assert os.path.exists(run), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    tmp = str(tmp_path)
    host_class_probe.write_sequence(tmp, [np.zeros((32, 48), np.uint8)], [np.ones((32, 48), np.float32)], (50.0, 50.0, 24.0, 16.0), [np.eye(4)])

    def run_with(extra):
        cfg = os.path.join(tmp, "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\nslidingWindowSize = 4\n%s" % (tmp, tmp, extra))
        return subprocess.run([run, "-c", cfg, "-o", os.path.join(tmp, "out.txt")], capture_output=True, text=True, timeout=120,
                              env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    r = run_with("outlierPasses = 1\noutlierQuantile = 2\n")
    assert r.returncode == 1 and "outlierQuantile = 2" in r.stderr and "pba_create" not in r.stderr
    r = run_with("outlierPasses = 1\n")
    assert r.returncode == 1 and "pba_create" in r.stderr


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------
def test_culling_an_occluder_brings_the_window_closer_to_the_ground_truth():
    """Figures of this case (recorded in DESIGN 4.17): pose error clean 9.25e-3, contaminated 5.37e-2, after the cull and the second solve
    2.63e-2; 98.5 % of the blocks inside the occluder culled, 24.6 % of the others."""
    from oracle import oracle
    clean, dirty, inside = cc.occluded_window(synthetic.make_window, dataclasses.replace)
    assert 550 <= clean.n_points <= 650 and clean.n_frames == 5 and inside.sum() > 200
    gt = clean.meta["cams_gt"]
    o = oracle.default_options(max_num_iterations=100)
    e_clean = cc.pose_error(oracle.solve(clean, o)["cams"], gt)
    first = oracle.solve(dirty, o)
    e_dirty = cc.pose_error(first["cams"], gt)
    c = cc.yardstick_block_costs(dirty, first["cams"], first["xyz"])
    keep, pmap, info = cc.reference_cull(c, dirty.obs_point, **cc.DEFAULTS)
    second = oracle.solve(cc.surviving_window(dirty, dataclasses.replace, first["cams"], first["xyz"], keep, pmap), o)
    e_culled = cc.pose_error(second["cams"], gt)
    culled = keep == 0
    f_in, f_out = float(culled[inside].mean()), float(culled[~inside].mean())
    print("pose error: clean %.4e, contaminated %.4e, solve -> cull -> solve %.4e; culled %.1f %% of the %d blocks inside the occluder, %.1f %% of the others"
          % (e_clean, e_dirty, e_culled, 100 * f_in, inside.sum(), 100 * f_out))
    assert e_dirty >= 2.0 * e_clean      # the occluder matters, else the case shows nothing
    assert e_culled < e_dirty
    assert f_in >= 0.90
