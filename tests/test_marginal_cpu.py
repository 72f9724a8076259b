"""CPU: the cases of tests/marginal_cases.py qualify, the marginalisation identity holds in numpy, the prior-augmented yardstick gives
clear iterations, the feature table answers for the camera prior, and the host class parses and refuses what it should."""
import os
import subprocess

import numpy as np
import pytest

import lm_yardstick as lm
import marginal_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the cases qualify --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case_qualifies(name):
    ref = mc.case_reference(name)
    piv = min(ref["min_point_pivot"], ref["min_cam_pivot"])
    lam = np.linalg.eigvalsh(ref["Lambda"])
    print("%s: k %d, M %d points / %d blocks, kappa %.3e, smallest pivot %.3e, c %.6e of cost %.6e, eig(Lambda) %.3e .. %.3e" % (
        name, len(ref["slots"]), ref["n_points"], ref["n_blocks"], ref["kappa"], piv, ref["c"], ref["cost"], lam[0], lam[-1]))
    assert ref["kappa"] <= mc.KAPPA_MAX
    assert piv >= mc.PIVOT_MIN
    assert ref["c"] >= 0.0
    assert len(ref["slots"]) >= 1 and ref["n_points"] >= 1
    # E >= 0 at 100 random offsets of the size of an LM step and beyond
    rng = np.random.default_rng(7)
    prior = mc.as_prior(ref)
    for scale in np.logspace(-6, 0, 100):
        cams = np.array(mc.window(name).cams, np.float64)
        cams[prior["slots"]] = prior["x0"] + scale * rng.standard_normal(prior["x0"].shape)
        E = float(mc.prior_terms(prior, cams, mc.LD)[0])
        assert E >= 0.0, (scale, E)


def test_the_named_window_has_the_counts_of_the_issue():
    ref = mc.case_reference("5x60-causal-huber-anchor-0-drop-0")
    assert (ref["n_points"], ref["n_blocks"]) == (20, 98)
    assert sorted(len(mc.case_reference(n)["slots"]) for n in mc.TRACE_CASES if n.startswith("16-slots")) == [14, 14, 15]


# ---- 2. the identity in numpy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.TRACE_CASES))
def test_one_step_identity(name):
    """Window A with the dropped cameras eliminated from its undamped reduced system equals window B (A without the points of M, the
    dropped slots constant) with the prior set."""
    p, anchors, drop = mc.window(name), mc.anchors_of(name), mc.drop_of(name)
    S_a, r_a = mc.eliminate_columns(*mc.reduced_undamped(lm.Dense(p, anchors)), mc.dropped_columns(p, anchors, drop))
    q, anchors_b = mc.window_b(p, anchors, drop)
    prior = mc.as_prior(mc.case_reference(name))
    S_b, r_b = mc.reduced_undamped(mc.DenseWithPrior(q, anchors_b, prior))
    assert S_a.shape == S_b.shape == (6 * len(prior["slots"]),) * 2
    s = np.sqrt(np.diag(S_a))
    d_S = float((np.abs(S_a - S_b) / (s[:, None] * s[None, :])).max())
    d_r = float(np.abs(r_a - r_b).max() / np.abs(r_a).max())
    # both sides are float64 solves of systems whose condition the case's kappa measures: kappa x the float64 epsilon, times ten as in
    # every bar of these cases (the reference itself is extended precision)
    bar = 10 * mc.case_reference(name)["kappa"] * np.finfo(np.float64).eps
    print("%s: n %d, S %.3e in correlation units, rhs %.3e of the largest entry, bar %.3e" % (name, len(S_a), d_S, d_r, bar))
    assert d_S <= bar and d_r <= bar


# ---- 3. clear iterations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.TRACE_CASES))
def test_yardstick_gives_clear_iterations(name):
    res, n_cmp, _, _, _ = mc.yardstick(name)
    print("%s: %d clear iterations of %d, cost %.6e -> %.6e" % (name, n_cmp, len(res["iterations"]), res["initial_cost"], res["final_cost"]))
    assert n_cmp >= 4
    assert res["final_cost"] < res["initial_cost"]


# ---- 4. the feature table --------------------------------------------------------------------------------------------------------------
MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR = (1 << k for k in range(10))
SWEEP_MODES = "the precision-sweep sampler modes (pba_config.flags bits 1-2) "
# (feature present, feature switched on) -> the sentence
PRIOR_SENTENCES = {
    (MULTI, PRIOR): "multi-rank solves (pba_comm_*) are not built for the camera prior",
    (PRIOR, MULTI): "multi-rank solves are not built for the camera prior (pba_set_camera_prior)",
    (SWEEP, PRIOR): SWEEP_MODES + "are not built for the camera prior",
    (PRIOR, SWEEP): SWEEP_MODES + "are not built for the camera prior",
    (PRIOR, WIDE): "the camera prior (pba_set_camera_prior) is not built for wide windows",
    (WIDE, PRIOR): "the camera prior is not built for wide windows",
    (PTS, PRIOR): "the camera prior is not built for the points-constant mode (pba_set_points_constant)",
    (PRIOR, PTS): "the camera prior (pba_set_camera_prior) is not built for the points-constant mode",
    (CAMS, PRIOR): "the camera prior is not built for the cameras-constant mode (pba_set_cameras_constant)",
    (PRIOR, CAMS): "the camera prior (pba_set_camera_prior) is not built for the cameras-constant mode",
    (INVDEPTH, PRIOR): "the camera prior is not built for the inverse-depth mode (pba_set_inverse_depth)",
    (PRIOR, INVDEPTH): "the camera prior (pba_set_camera_prior) is not built for the inverse-depth mode",
    (PRIOR, COV): "the camera prior (pba_set_camera_prior) is set: a covariance that ignored it would be wrong",
    (COV, PRIOR): "the camera prior (pba_set_camera_prior) is set: a covariance that ignored it would be wrong",
    (PRIOR, BATCH): "the camera prior (pba_set_camera_prior) solves alone",
    (BATCH, PRIOR): "the camera prior (pba_set_camera_prior) solves alone",
}


@pytest.fixture(scope="module")
def lookup(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("mode_rules_prior")), "mode_rules_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "mode_rules_probe.cpp")])

    def run(queries):
        r = subprocess.run([exe], input="".join("%x %x\n" % q for q in queries), capture_output=True, text=True, check=True, timeout=60)
        out = [line.split("\t") for line in r.stdout.splitlines()]
        assert len(out) == len(queries)
        return [(int(w, 16), None if s == "-" else s) for w, s in out]
    return run


def test_every_pair_with_the_prior_bit_in_both_orders(lookup):
    others = (MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR)
    pairs = [(a, PRIOR) for a in others] + [(PRIOR, b) for b in others]
    for (present, on), (with_, why) in zip(pairs, lookup(pairs)):
        want = PRIOR_SENTENCES.get((present, on))
        assert why == want, (hex(present), hex(on), why)
        assert with_ == (present if want else 0)
    # anchors and the prior combine; the prior conflicts with eight features
    assert (ANCHORS, PRIOR) not in PRIOR_SENTENCES and len({frozenset(k) for k in PRIOR_SENTENCES}) == 8


def test_existing_answers_stay_with_the_prior_present(lookup):
    """The rows of the prior are appended: where an older conflict is present too, the older sentence still wins."""
    got = lookup([(MULTI | PRIOR, COV), (MULTI | PRIOR, BATCH), (MULTI | PRIOR, WIDE), (PRIOR, ANCHORS), (ANCHORS | PRIOR, MULTI)])
    assert got[0] == (MULTI, "multi-rank engines (pba_comm_*) are not built for the covariance output")
    assert got[1] == (MULTI, "multi-rank engines (pba_comm_*) solve alone")
    assert got[2] == (MULTI, "multi-rank solves (pba_comm_*) are not built for wide windows")
    assert got[3] == (0, None)
    assert got[4] == (ANCHORS, "multi-rank solves take at most one constant slot")


def test_the_prior_sentences_live_in_the_header_alone():
    with open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_engine.hip")) as f:
        src = f.read()
    for why in PRIOR_SENTENCES.values():
        assert why not in src, why


# ---- 5. the class option ---------------------------------------------------------------------------------------------------------------
def test_class_option_parses_prints_and_refuses(tmp_path):
    """Options::marginalize through the stand-alone probe program, with every device hidden: the key, its default, the printed line, and
    std::invalid_argument with camerasConstant and with computeCovariance before any device call.  The third case, addFrames, needs an
    instance and so a device: tests/test_gpu_marginal.py runs the same program there."""
    header = open(os.path.join(ROOT, "photobundle_amd", "host", "photobundle.h")).read()
    assert "bool marginalize = false;" in header and "double priorCost = 0.0;" in header
    r = mc.run_class_probe(tmp_path, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert "FAILED" not in r.stdout and sum(line.startswith("ok ") for line in lines) == 8
    for what in ("ok default 0", "ok key marginalize = 1", "ok key marginalize = 0", "ok operator<< prints the key",
                 "ok invalid_argument with camerasConstant", "ok invalid_argument with computeCovariance",
                 "ok marginalize alone passes the constructor's checks"):
        assert what in lines, what
    assert any(line.startswith("addFrames skipped: other: ") for line in lines)


def test_run_kitti_reads_the_key(tmp_path):
    """run_kitti on a one-frame sequence with every device hidden: the refusals come before any device call, the key alone reaches it."""
    import host_class_probe
    run = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    assert os.path.exists(run), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    host_class_probe.write_sequence(str(tmp_path), [np.zeros((32, 48), np.uint8)], [np.ones((32, 48), np.float32)], (50.0, 50.0, 24.0, 16.0), [np.eye(4)])

    def go(extra):
        cfg = os.path.join(str(tmp_path), "test.cfg")
        with open(cfg, "w") as f:
            f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nverbose = 0\nslidingWindowSize = 4\n%s" % (tmp_path, tmp_path, extra))
        return subprocess.run([run, "-c", cfg, "-o", os.path.join(str(tmp_path), "out.txt")], capture_output=True, text=True, timeout=120,
                              env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    r = go("marginalize = 1\ncamerasConstant = 1\n")
    assert r.returncode == 1 and "marginalize with camerasConstant" in r.stderr and "pba_create" not in r.stderr
    r = go("marginalize = 1\ncomputeCovariance = 1\nnumConstantFrames = 2\n")
    assert r.returncode == 1 and "marginalize with computeCovariance" in r.stderr and "pba_create" not in r.stderr
    r = go("marginalize = 1\n")
    assert r.returncode == 1 and "pba_create" in r.stderr and "marginalize with" not in r.stderr
