"""The point prior (pba_set_point_prior) without a device: the yardsticks of tests/point_prior_cases.py against central differences of
their own cost, the gauge case in the reference alone (one constant camera: the reduced matrix is singular without the depth priors and
well conditioned with them), the new rows of the feature-conflict table, and the call's declaration, binding and export."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_cases as cc
import lm_yardstick as lm
import marginal_cases as mc
import point_prior_cases as pp
from test_mode_rules_cpu import EXPECTED as OLD_EXPECTED, FEATURES as OLD_FEATURES, ONE_WAY as OLD_ONE_WAY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the yardsticks -----------------------------------------------------------------------------------------------------------------------
def _central_differences(cost, x, idx, h):
    g = np.zeros(len(idx))
    for k, i in enumerate(idx):
        a, b = x.copy(), x.copy()
        a.flat[i] += h
        b.flat[i] -= h
        g[k] = (cost(a) - cost(b)) / (2 * h)
    return g


@pytest.mark.parametrize("kind", pp.KINDS)
def test_prior_gradient_is_the_derivative_of_the_prior_cost(kind):
    """E is quadratic: central differences are exact up to rounding, so the bar is a rounding bar (1e-9 of the largest entry)."""
    name = "3-dense-65-points-anchor-0"
    p = pp.window(name)
    x0, L6 = pp.prior(name, kind)
    x = np.array(p.xyz, np.float64)
    g = np.einsum("nij,nj->ni", pp.sym3(L6), x - x0).ravel()
    idx = np.arange(x.size)
    fd = _central_differences(lambda y: pp.energy(x0, L6, y), x, idx, 1e-3)
    print("%s: E %.6e, |g| max %.3e, difference %.3e" % (kind, pp.energy(x0, L6, x), np.abs(g).max(), np.abs(g - fd).max()))
    assert pp.energy(x0, L6, x) > 0 and np.abs(g).max() > 0
    assert np.abs(g - fd).max() <= 1e-9 * np.abs(g).max()
    if kind == "mixed":
        assert np.all(g.reshape(-1, 3)[2::3] == 0.0)              # a point with Lambda = 0 has no prior


def test_yardsticks_add_the_prior_to_cost_gradient_and_matrix():
    """DenseWithPointPrior and PointBlocksWithPrior against their parents: the differences are E, Lambda d and Lambda, and what the
    prior adds to the dense gradient is the central difference of what it adds to the dense cost."""
    name = "3-dense-63-points-anchor-0"
    p, anchors = pp.window(name), pp.anchors_of(name)
    x0, L6 = pp.prior(name, "mixed")
    L = pp.sym3(L6)
    plain, prog = lm.Dense(p, anchors), pp.DenseWithPointPrior(p, anchors, x0, L6)
    st = prog.start()
    a, b = plain.linearize(plain.start()), prog.linearize(st)
    nc = prog.n_cam
    E = pp.energy(x0, L6, p.xyz)
    assert np.isclose(b["cost"] - a["cost"], E, rtol=1e-9) and np.isclose(prog.prior_cost(st), E, rtol=1e-15)
    assert np.array_equal(a["gradient"][:nc], b["gradient"][:nc])
    # (a difference of two sums: the rounding of the photometric gradient is the floor)
    assert np.allclose(b["gradient"][nc:] - a["gradient"][nc:], np.einsum("nij,nj->ni", L, p.xyz - x0).ravel(), rtol=1e-9,
                       atol=1e-14 * np.abs(a["gradient"]).max())
    dH = b["H"] - a["H"]
    for i in range(p.n_points):
        s = slice(nc + 3 * i, nc + 3 * i + 3)
        assert np.allclose(dH[s, s], L[i], rtol=1e-9, atol=1e-14 * np.abs(a["H"]).max())
        dH[s, s] = 0.0
    assert np.all(dH == 0.0)
    assert np.array_equal(b["diagonal"], np.diag(b["H"]))
    # central differences of the yardstick's own cost.  The photometric part is sampled bilinearly and its analytic gradient uses the
    # gradient planes, so it is no derivative of the sampled cost to more than a percent; it is the SAME evaluation in both programs,
    # though, and leaves the difference of the two costs' central differences up to the rounding of a cost (eps x cost / h).  What is
    # left is the derivative of E, exact for a quadratic at any step.
    idx = np.arange(0, 3 * p.n_points, 7)
    cams, x = st
    h = 1e-3
    fd = _central_differences(lambda y: prog.cost((cams, y)), x, idx, h) - _central_differences(lambda y: plain.cost((cams, y)), x, idx, h)
    want = (b["gradient"] - a["gradient"])[nc:][idx]
    floor = 4 * np.finfo(np.float64).eps * a["cost"] / h
    print("prior part of the dense gradient against central differences: %.3e, rounding floor %.3e, largest entry %.3e" % (
        np.abs(fd - want).max(), floor, np.abs(want).max()))
    assert np.abs(want).max() > 100 * floor
    assert np.abs(fd - want).max() <= floor + 1e-9 * np.abs(want).max()
    # the cameras-constant yardstick holds the same blocks
    pb, pbp = lm.PointBlocks(p), pp.PointBlocksWithPrior(p, x0, L6)
    la, lb = pb.linearize(pb.start()), pbp.linearize(pbp.start())
    assert np.isclose(lb["cost"] - la["cost"], E, rtol=1e-9)
    assert np.allclose(lb["V"] - la["V"], L, rtol=1e-9, atol=1e-14 * np.abs(la["V"]).max())
    assert np.allclose(lb["gradient"], b["gradient"][nc:].reshape(-1, 3), rtol=1e-12, atol=1e-12 * np.abs(b["gradient"]).max())


# ---- 2. the gauge case, in the reference alone ---------------------------------------------------------------------------------------------
def test_depth_priors_close_the_gauge_of_a_window_with_one_constant_camera():
    """Three frames, one constant camera: the scale of the window is free, so the undamped reduced camera matrix is singular -- its
    unit-diagonal form fails Cholesky or has a pivot at rounding level.  Rank-1 depth priors, one per point, fix the scale: the same
    matrix then has every pivot >= marginal_cases.PIVOT_MIN and H + Lambda a condition number <= KAPPA_MAX."""
    p, anchors = pp.window(pp.GAUGE), pp.anchors_of(pp.GAUGE)
    assert len(anchors) == 1 and p.n_frames == 3
    x0, L6 = pp.prior(pp.GAUGE, "depth")
    assert all(np.linalg.matrix_rank(b) == 1 for b in pp.sym3(L6))
    plain = lm.Dense(p, anchors)
    H0, nc = plain.linearize(plain.start())["H"], plain.n_cam
    try:
        piv0 = cc.min_pivot(pp.reduced_unit_diagonal(H0, nc), np.float64)
    except np.linalg.LinAlgError:
        piv0 = 0.0
    prog = pp.DenseWithPointPrior(p, anchors, x0, L6)
    H1 = prog.linearize(prog.start())["H"]
    piv1, kappa = cc.min_pivot(pp.reduced_unit_diagonal(H1, nc), np.float64), cc.kappa(H1)
    print("gauge case: smallest pivot without the prior %.3e, with it %.3e; kappa(H + Lambda) %.3e (without: %.3e)" % (piv0, piv1, kappa, cc.kappa(H0)))
    assert piv0 <= 1e-9
    assert piv1 >= mc.PIVOT_MIN and kappa <= mc.KAPPA_MAX


# ---- 3. the new rows of the feature-conflict table ----------------------------------------------------------------------------------------
MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR, CULL, ADMIT, POINT_PRIOR = (1 << k for k in range(13))
ALL_OLD = (MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR, CULL, ADMIT)
SWEEP_MODES = "the precision-sweep sampler modes (pba_config.flags bits 1-2) "
# (feature present, feature switched on) -> sentence
NEW = {
    (MULTI, POINT_PRIOR): "multi-rank solves (pba_comm_*) are not built for the point prior",
    (POINT_PRIOR, MULTI): "multi-rank solves are not built for the point prior (pba_set_point_prior)",
    (SWEEP, POINT_PRIOR): SWEEP_MODES + "are not built for the point prior",
    (POINT_PRIOR, BATCH): "the point prior (pba_set_point_prior) solves alone",
    (PTS, POINT_PRIOR): "the point prior is not built for the points-constant mode (pba_set_points_constant): the prior is then a constant",
    (POINT_PRIOR, PTS): "the point prior (pba_set_point_prior) is not built for the points-constant mode: the prior is then a constant",
    (INVDEPTH, POINT_PRIOR): "the point prior is not built for the inverse-depth mode (pba_set_inverse_depth)",
    (POINT_PRIOR, INVDEPTH): "the point prior (pba_set_point_prior) is not built for the inverse-depth mode",
    (PRIOR, POINT_PRIOR): "the point prior is not built next to the camera prior (pba_set_camera_prior): it eliminates through the wide chain, "
                          "the camera prior is narrow-only",
    (POINT_PRIOR, PRIOR): "the camera prior is not built next to the point prior (pba_set_point_prior): it is narrow-only, the point prior "
                          "eliminates through the wide chain",
}
NEW_ONE_WAY = (SWEEP, BATCH)


@pytest.fixture(scope="module")
def lookup(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("point_prior_rules")), "mode_rules_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "mode_rules_probe.cpp")])

    def run(queries):
        r = subprocess.run([exe], input="".join("%x %x\n" % q for q in queries), capture_output=True, text=True, check=True, timeout=60)
        out = [line.split("\t") for line in r.stdout.splitlines()]
        assert len(out) == len(queries)
        return [(int(w, 16), None if s == "-" else s) for w, s in out]
    return run


def test_every_new_pair_in_both_orders(lookup):
    assert len(set(NEW.values())) == 10
    pairs = [(a, POINT_PRIOR) for a in ALL_OLD] + [(POINT_PRIOR, a) for a in ALL_OLD] + [(POINT_PRIOR, POINT_PRIOR)]
    for (present, on), (with_, why) in zip(pairs, lookup(pairs)):
        want = NEW.get((present, on))
        if want is None and (on in NEW_ONE_WAY or present in NEW_ONE_WAY):
            want = NEW.get((on, present))
        assert why == want, (hex(present), hex(on), why)
        assert with_ == (present if want else 0)
    # what combines with the point prior: wide windows, the cameras-constant mode, anchors, the covariance output, culling, re-observation
    for f in (WIDE, CAMS, ANCHORS, COV, CULL, ADMIT):
        assert (f, POINT_PRIOR) not in NEW and (POINT_PRIOR, f) not in NEW


def test_every_old_answer_stays_with_the_new_bit_present(lookup):
    """A pair of older features answers as before whether or not the point prior is present as well.  Present can be a state only:
    the covariance output, a batch, a cull and an admission are calls, and nothing is ever switched on next to one."""
    states = (MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, PRIOR)
    pairs = [(a, b) for a in states for b in ALL_OLD]
    plain = lookup(pairs)
    with_bit = lookup([(a | POINT_PRIOR, b) for a, b in pairs])
    for (a, b), (w0, s0), (w1, s1) in zip(pairs, plain, with_bit):
        if s0 is not None:
            assert (w1, s1) == (w0, s0), (hex(a), hex(b))         # the older row comes first
        else:
            want = NEW.get((POINT_PRIOR, b)) or (NEW.get((b, POINT_PRIOR)) if b in NEW_ONE_WAY else None)
            assert s1 == want and w1 == (POINT_PRIOR if want else 0), (hex(a), hex(b), s1)
    # ... and the table of tests/test_mode_rules_cpu.py as that file states it
    old_pairs = [(a, b) for a in OLD_FEATURES for b in OLD_FEATURES]
    for (present, on), (_, why) in zip(old_pairs, lookup([(a | POINT_PRIOR, b) for a, b in old_pairs])):
        want = OLD_EXPECTED.get((present, on))
        if want is None and (on in OLD_ONE_WAY or present in OLD_ONE_WAY):
            want = OLD_EXPECTED.get((on, present))
        if want is not None:
            assert why == want, (hex(present), hex(on), why)


def test_the_new_sentences_live_in_the_header_alone():
    with open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_engine.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_mode_rules.h")) as f:
        rules = f.read()
    for why in NEW.values():
        assert why not in src and why in rules, why
    assert re.search(r"kModePointPrior\s*=\s*4096\b", rules)


# ---- 4. declaration, binding, export -------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_bound_and_exported():
    from photobundle_amd import _lib
    header = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"int\s+pba_set_point_prior\s*\(\s*pba_engine\s*\*\s*e\s*,\s*int32_t\s+n_points\s*,\s*const\s+double\s*\*\s*x0\s*,"
                     r"\s*const\s+double\s*\*\s*Lambda6\s*\)\s*;", header)
    L = _lib.lib()
    assert "pba_set_point_prior" in _lib.SYMBOLS
    assert L.pba_set_point_prior.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T pba_set_point_prior\n" in nm
    assert L.pba_set_point_prior(None, 1, None, None) == -1      # PBA_ERR_INVALID
    from photobundle_amd.engine import Engine
    assert callable(Engine.set_point_prior)


# ---- 5. the host class: Options::depthPriorSigma without a device ----------------------------------------------------------------------------
def test_class_option_key_line_and_constructor_checks(tmp_path):
    import point_prior_class_probe
    probe = point_prior_class_probe.PointPriorClassProbe(tmp_path)
    assert probe.defaults_are_zero()
    assert probe.config_key("1.5") == 1.5 and probe.config_key("0") == 0.0
    assert "\ndepthPriorSigma = 0\n" in probe.print_options(0.0) and "\ndepthPriorSigma = 0.25\n" in probe.print_options(0.25)
    size, K = (96, 128), (160.0, 160.0, 64.0, 48.0)
    # std::invalid_argument from the constructor, before it touches a device
    rc, what = probe.create(size, K, 4, 1, sigma=1.0, baseline=0.0)
    assert rc == 1 and what.startswith("depthPriorSigma > 0 needs a stereo baseline"), what
    rc, what = probe.create(size, K, 4, 1, sigma=1.0, baseline=-0.5)
    assert rc == 1 and what.startswith("depthPriorSigma > 0 needs a stereo baseline"), what
    rc, what = probe.create(size, K, 4, 1, sigma=1.0, marginalize=True)
    assert rc == 1 and what.startswith("depthPriorSigma > 0 with marginalize"), what
    rc, what = probe.create(size, K, 4, 1, sigma=-1.0)
    assert rc == 1 and what.startswith("depthPriorSigma = -1"), what
    rc, what = probe.create(size, K, 4, 1, sigma=float("nan"))
    assert rc == 1 and what.startswith("depthPriorSigma = "), what
    # computeCovariance with ONE constant frame: refused as ever without the prior, legal with it
    rc, what = probe.create(size, K, 4, 1, sigma=0.0, compute_covariance=True, num_constant=1)
    assert rc == 1 and what.startswith("computeCovariance needs numConstantFrames >= 2 or camerasConstant"), what
    rc, what = probe.create(size, K, 4, 1, sigma=1.0, compute_covariance=True, num_constant=1)
    assert rc == 0 or (rc == 2 and "pba_create" in what), what      # (2: no device on this machine; the checks were passed)
    # a zero baseline is nobody's business while the prior is off
    rc, what = probe.create(size, K, 4, 1, sigma=0.0, baseline=0.0)
    assert rc == 0 or (rc == 2 and "pba_create" in what), what
    probe.release()
