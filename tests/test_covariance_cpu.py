"""CPU side of the covariance output (pba_covariance): the cases qualify, the test helper's extended-precision inverse is right, the block
formulas of include/pba.h are the blocks of the dense inverse, the gauge-open variants are what the pivot says they are, and the ABI is
declared, exported and mirrored."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from photobundle_amd import _lib

import covariance_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", sorted(cc.FULL_CASES))
def test_case_qualifies(name):
    """Condition, not measurement: kappa <= 1e8 and a camera pivot >= 1e-5 for every covariance case."""
    ref = cc.full_reference(cc.window(name), cc.slots_of(name))
    print("%s: n_cam %d, kappa %.3e, bar %.3e, min pivots camera %.3e point %.3e" % (
        name, ref["n_cam"], ref["kappa"], ref["bar"], ref["min_cam_pivot"], ref["min_point_pivot"]))
    assert ref["kappa"] <= cc.KAPPA_MAX
    assert ref["min_cam_pivot"] >= cc.PIVOT_MIN
    assert 0 < ref["min_point_pivot"] <= 1 and 0 < ref["min_cam_pivot"] <= 1


@pytest.mark.parametrize("name", ["3x40-dense-r1-anchors-0-2", "5x60-causal-huber-anchors-0-4", "17-slots-anchors-0-1"])
def test_extended_precision_inverse_against_numpy(name):
    """The helper's longdouble inverse and np.linalg.inv agree within the float64 band of numpy's own inverse, kappa x eps with the
    x 10 margin, and H times the helper's inverse is the identity to the same band."""
    ref = cc.full_reference(cc.window(name), cc.slots_of(name))
    H = ref["H"]
    inv, piv = cc.inverse_ld(H)
    band = 10 * ref["kappa"] * EPS
    err = cc.correlation_error(np.linalg.inv(H), inv)
    Hu, d = cc.unit_diagonal(np.asarray(H, cc.LD))
    resid = float(np.abs(Hu @ (np.asarray(inv, cc.LD) / d[:, None] / d[None, :]) - np.eye(len(H))).max())
    print("%s: numpy vs longdouble %.3e (band %.3e), residual %.3e, pivot %.3e" % (name, err, band, resid, piv))
    assert err <= band
    assert resid <= band
    assert 0 < piv <= 1


@pytest.mark.parametrize("name", ["3x40-dense-r1-anchors-0-2", "5x60-causal-huber-anchors-0-1-2", "17-slots-16-anchors"])
def test_block_formulas_are_the_blocks_of_the_dense_inverse(name):
    """Sigma_cc = S^-1 and Sigma_pp(i) = V^-1 + (V^-1 W^T) Sigma_cc (W V^-1), float64 from the block sums, against the blocks of the
    longdouble inverse of the dense H: the float64 band kappa x eps x 10.  (5 slots with anchors {0, 1, 2}: causal points born late are
    seen by free cameras only, early ones by anchors too.)"""
    p, slots = cc.window(name), cc.slots_of(name)
    ref = cc.full_reference(p, slots)
    Scc, Spp, _ = cc.schur_covariance(*cc.block_sums(p, slots))
    band = 10 * ref["kappa"] * EPS
    e_c, e_p = cc.correlation_error(Scc, ref["cam_cov"]), cc.correlation_error(Spp, ref["point_cov"])
    print("%s: camera %.3e, points %.3e, band %.3e" % (name, e_c, e_p, band))
    assert e_c <= band and e_p <= band


def test_constant_mode_formulas():
    """Pose-only: blockdiag(U_a^-1) is the inverse of the camera columns' J^T J with the points held; structure-only: V_i^-1, and with
    inverse depths the 1 x 1 blocks through the chain rule."""
    name = "5x60-causal-huber-anchors-0-4"
    p = cc.window(name)
    cols, cov, U, cost = cc.pose_reference(p, (0, 3))
    assert cols == [1, 2, 4] and cov.shape == (18, 18) and cost > 0
    for k in range(3):
        assert np.abs(cov[6 * k:6 * k + 6, 6 * k:6 * k + 6] @ U[k] - np.eye(6)).max() <= 10 * np.linalg.cond(U[k]) * EPS
    assert not cov[:6, 6:].any()
    Pv, V, _ = cc.structure_reference(p)
    # (the product of a float64-rounded inverse with V leaves the identity by the block's condition number x eps)
    assert np.abs(np.einsum("nij,njk->nik", Pv, V) - np.eye(3)).max() <= 10 * np.linalg.cond(V).max() * EPS
    from photobundle_amd import synthetic
    q = cc.window(cc.INVERSE_DEPTH)
    rays, rho = synthetic.inverse_depth_rays(q)
    P1, V1, _ = cc.structure_reference(q, rays, rho)
    assert P1.shape == (q.n_points, 1, 1) and np.allclose(P1 * V1, 1.0, rtol=1e-12)


@pytest.mark.parametrize("name", sorted(cc.ONE_ANCHOR))
def test_one_anchor_variants_are_gauge_open(name):
    """With one constant frame the scale of the window is free: the reference pivot of the unit-diagonal reduced matrix is below 1e-9 or
    not positive, eight orders of magnitude from the two-anchor windows."""
    p, slots = cc.window(name), cc.slots_of(name)
    free, U, W, V = cc.block_sums(p, slots)
    nc = 6 * len(free)
    S = np.zeros((nc, nc), cc.LD)
    for a in range(len(free)):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = U[a]
    by_point = {}
    for (a, i), w in W.items():
        by_point.setdefault(i, []).append((a, np.asarray(w, cc.LD)))
    for i, lst in by_point.items():
        Pi = np.asarray(cc.inverse_ld(V[i])[0], cc.LD)
        for a, wa in lst:
            for b, wb in lst:
                S[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= wa @ Pi @ wb.T
    piv = cc.min_pivot(S, np.float64)
    print("%s: n %d, float64 pivot of the unit-diagonal S %.3e" % (name, nc, piv))
    assert piv < 1e-9


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_mirrored():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"int\s+pba_covariance\s*\(\s*pba_engine\s*\*\s*e\s*,\s*double\s*\*\s*cam_cov\s*,\s*double\s*\*\s*point_cov\s*,"
                     r"\s*pba_covariance_info\s*\*\s*info\s*\)\s*;", header)
    assert hasattr(L, "pba_covariance") and "pba_covariance" in _lib.SYMBOLS
    assert [f for f, _ in _lib.CovarianceInfo._fields_] == ["n_cam", "point_dim", "num_residuals", "num_parameters", "cost", "min_cam_pivot",
                                                          "min_point_pivot", "failed_is_point", "failed_index"]


def test_info_struct_size_matches_the_header():
    """sizeof and the offsets the C compiler gives pba_covariance_info against the ctypes mirror."""
    src = ('#include "pba.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pba_covariance_info), '
           'offsetof(pba_covariance_info, cost), offsetof(pba_covariance_info, min_point_pivot), offsetof(pba_covariance_info, failed_index)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), c])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    I = _lib.CovarianceInfo
    assert got == [C.sizeof(I), I.cost.offset, I.min_point_pivot.offset, I.failed_index.offset]
    assert C.sizeof(I) == 4 * 4 + 3 * 8 + 2 * 4


def test_null_engine_is_refused_without_a_device():
    info = _lib.CovarianceInfo()
    buf = (C.c_double * 36)()
    assert _lib.lib().pba_covariance(None, buf, None, C.byref(info)) == -1       # PBA_ERR_INVALID
    assert not any(buf)


# ---- the host class ----------------------------------------------------------------------------------------------------------------------
def test_class_header_fields_and_the_open_gauge_refusal(tmp_path):
    """The new Options / Result / TrackOptions / TrackResult fields exist with their defaults (the probe does not compile otherwise), the
    key is printed, and the constructor refuses computeCovariance with one constant frame before it touches a device."""
    import covariance_class_probe
    header = open(os.path.join(ROOT, "photobundle_amd", "host", "photobundle.h")).read()
    for field in ("bool computeCovariance = false;", "bool covarianceOk = false;", "std::string covarianceMessage;", "minCameraPivot", "minPointPivot",
                  "covarianceFrameIds;", "poseCovariance;", "refinedPointCovariances;", "double covariance[36]", "double minPivot"):
        assert field in header, field
    assert header.count("bool computeCovariance = false;") == 2 and header.count("bool covarianceOk = false;") == 2
    assert header.count("std::string covarianceMessage;") == 2      # Result and TrackResult
    assert "WORLD->CAMERA" in header
    probe = covariance_class_probe.CovarianceClassProbe(tmp_path)
    assert probe.defaults() == 0
    assert "computeCovariance = 0\n" in probe.print_options(False) and "computeCovariance = 1\n" in probe.print_options(True)
    size, K = (96, 128), (160.0, 160.0, 64.0, 48.0)
    with pytest.raises(RuntimeError, match="computeCovariance needs numConstantFrames >= 2 or camerasConstant.*gauge is open"):
        probe.create(size, K, window=5, radius=1, num_constant=1, compute_covariance=True)
    import torch
    if not torch.cuda.is_available():
        # two constant frames, or constant cameras, pass the check: the constructor gets as far as the device
        for kw in (dict(num_constant=2), dict(num_constant=1, cameras_constant=True)):
            with pytest.raises(RuntimeError, match="pba_create"):
                probe.create(size, K, window=5, radius=1, compute_covariance=True, **kw)


def _run_kitti(tmp, extra):
    """run_kitti on a one-frame sequence with every device hidden: whatever is refused is refused before any device call."""
    import host_class_probe
    run = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    assert os.path.exists(run), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    host_class_probe.write_sequence(str(tmp), [np.zeros((32, 48), np.uint8)], [np.ones((32, 48), np.float32)], (50.0, 50.0, 24.0, 16.0), [np.eye(4)])
    cfg = os.path.join(str(tmp), "test.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\nslidingWindowSize = 4\n%s" % (tmp, tmp, extra))
    return subprocess.run([run, "-c", cfg, "-o", os.path.join(str(tmp), "out.txt")], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_run_kitti_reads_the_key(tmp_path):
    r = _run_kitti(tmp_path, "computeCovariance = 1\n")
    assert r.returncode == 1 and "gauge is open" in r.stderr and "pba_create" not in r.stderr
    r = _run_kitti(tmp_path, "computeCovariance = 1\nnumConstantFrames = 2\n")
    assert r.returncode == 1 and "pba_create" in r.stderr and "gauge is open" not in r.stderr
