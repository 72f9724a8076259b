"""-m gpu: the semi-global matcher (include/pba_sgm.h) on the MI355X.  Device float and uint16 disparities against the fixtures made
by the reference's own code (tests/golden/sgm), byte for byte, full size included; every stage of pba_sgm_get_stage against the
numpy restatement (tests/sgm_ref.py) so that a failure names its stage; a seeded sweep of random shapes and parameter sets; the
fused depth, partial outputs and repeatability; the host SgmStereo; and run_kitti with StereoAlgorithm = SGM end to end."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sgm_ref as ref
import sgm_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
FIX = os.path.join(ROOT, "tests", "golden", "configs0")
BASELINE = 0.5372
CASES = sgm_util.load_cases()
# the semi-global keys the reference's config/kitti_stereo.cfg sets (the rest stay at their defaults)
REF_CFG = dict(number_of_disparities=128, sobel_cap_value=15, census_radius=1, window_radius=3)


def _matcher(rows, cols, p):
    from photobundle_amd.stereo import StereoSGM
    return StereoSGM(rows, cols, **sgm_util.snake_params(p))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_byte_for_byte(case):
    left, right = sgm_util.case_pair(case)
    assert sgm_util.sha256(left, right) == case["input_sha256"]
    p = sgm_util.params_of(case)
    with _matcher(case["rows"], case["cols"], p) as s:
        u, d, _ = s.compute_all(left, right, 1.0)
    whole, rows = sgm_util.case_expected(case)
    if whole is not None:
        bad = np.argwhere(u != whole)
        assert bad.size == 0, "%d of %d pixels differ from the reference, first %s: got %d want %d" % (
            len(bad), u.size, bad[0], u[tuple(bad[0])], whole[tuple(bad[0])])
        assert d.tobytes() == sgm_util.float_map(whole, p["disparityFactor"]).tobytes()
    else:
        index, stored = rows
        assert np.array_equal(u[index], stored)
    assert sgm_util.sha256(u) == case["disp_scaled_sha256"]
    assert sgm_util.sha256(d) == case["disparity_sha256"]


def _check_stages(left, right, p, bf=386.0):
    """Device against the restatement, stage by stage in pipeline order, then the outputs."""
    q = dict(p)
    want = ref.compute(left, right, q.pop("numberOfDisparities"), stages=True, **q)
    with _matcher(left.shape[0], left.shape[1], p) as s:
        u, d, z = s.compute_all(left, right, bf)
        for name in ref.STAGES:
            got = s.stage(name)
            assert got.dtype == want[name].dtype and got.shape == want[name].shape, name
            bad = np.argwhere(got != want[name])
            assert bad.size == 0, "stage %s: %d of %d elements differ, first %s: got %d want %d (%s)" % (
                name, len(bad), got.size, bad[0], got[tuple(bad[0])], want[name][tuple(bad[0])], p)
    assert np.array_equal(u, want["disp_scaled"]), p
    assert d.tobytes() == want["disparity"].tobytes()
    assert z.tobytes() == sgm_util.disparity_to_depth(want["disparity"], bf).tobytes()


@pytest.mark.parametrize("case", [c for c in CASES if c["file"]], ids=lambda c: c["name"])
def test_every_stage_equals_the_restatement(case):
    left, right = sgm_util.case_pair(case)
    _check_stages(left, right, sgm_util.params_of(case))


def _sweep_cases(n=28, seed=20261016):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nd = int(rng.choice([16, 32, 48, 64, 96, 128]))
        cols = int(rng.integers(nd, 401))
        wr = int(rng.integers(0, 10))
        rows = int(rng.integers(max(3, wr + 1), 201))
        if nd * rows * cols > 128 * 120 * 400:                  # keeps the restatement's time per case in seconds
            rows = max(3, wr + 1, (128 * 120 * 400) // (nd * cols))
        p1 = int(rng.choice([0, 5, 100, 400, 3000]))
        factor = float(rng.choice([1, 16, 100, 256, 512]))
        p = dict(numberOfDisparities=nd, sobelCapValue=int(rng.choice([15, 31, 64, 127])), censusRadius=int(rng.integers(1, 3)),
                 windowRadius=wr, smoothnessPenaltySmall=p1, smoothnessPenaltyLarge=int(p1 + rng.choice([1, 300, 1500, 9000, 29000])),
                 consistencyThreshold=int(rng.integers(0, 4)), disparityFactor=factor if nd * factor <= 65536 else 256.0,
                 censusWeightFactor=float(rng.choice([0.0, 1.0 / 6.0, 0.5, 1.0, 2.5])))
        out.append((rows, cols, 9000 + i, p))
    return out


SWEEP = _sweep_cases()


@pytest.mark.parametrize("rows,cols,seed,p", SWEEP, ids=["%dx%dx%d" % (r, c, p["numberOfDisparities"]) for r, c, _, p in SWEEP])
def test_seeded_sweep_equals_the_restatement(rows, cols, seed, p):
    assert len(SWEEP) >= 24
    if seed % 3 == 0:                                            # a third of the pairs are plain noise: worst case for the filters
        rng = np.random.RandomState(seed)
        left, right = (rng.randint(0, 256, (rows, cols)).astype(np.uint8) for _ in range(2))
    else:
        left, right, _ = sgm_util.make_pair(rows, cols, p["numberOfDisparities"], seed)
    _check_stages(left, right, p)


def test_outputs_one_at_a_time_two_handles_and_repeats():
    p = dict(sgm_util.DEFAULTS, numberOfDisparities=32)
    a = sgm_util.make_pair(60, 160, 32, 11)[:2]
    b = sgm_util.make_pair(60, 160, 32, 12)[:2]
    bf = 386.1726
    with _matcher(60, 160, p) as s, _matcher(60, 160, p) as t:
        u, d, z = s.compute_all(*a, bf)
        assert z.tobytes() == sgm_util.disparity_to_depth(d, bf).tobytes()
        assert (u != 0).mean() > 0.5
        for ask in ((True, False, False), (False, True, False), (False, False, True)):
            got = s.compute_all(*a, bf, *ask)
            for g, w, asked in zip(got, (u, d, z), ask):
                assert (g is None) if not asked else g.tobytes() == w.tobytes()
        d2, z2 = s.compute(*a, bf)
        assert d2.tobytes() == d.tobytes() and z2.tobytes() == z.tobytes()
        ub = s.compute_all(*b, bf)[0]
        assert not np.array_equal(ub, u)
        u3, d3, z3 = s.compute_all(*a, bf)                       # a different pair in between leaves nothing behind
        assert u3.tobytes() == u.tobytes() and d3.tobytes() == d.tobytes() and z3.tobytes() == z.tobytes()
        ut, dt, zt = t.compute_all(*a, bf)                       # a second handle
        assert ut.tobytes() == u.tobytes() and dt.tobytes() == d.tobytes() and zt.tobytes() == z.tobytes()
        assert t.compute_all(*b, bf)[0].tobytes() == ub.tobytes()
        k_ms, t_ms = s.timing()
        assert 0 < k_ms <= t_ms


def test_invalid_handle_use():
    from photobundle_amd.stereo import StereoError, StereoSGM
    with StereoSGM(32, 64, number_of_disparities=16) as s:
        with pytest.raises(StereoError, match="before pba_sgm_compute"):
            s.stage("sobel_left")
        with pytest.raises(StereoError, match="before pba_sgm_compute"):
            s.timing()
        with pytest.raises(ValueError):
            s.compute(np.zeros((32, 63), np.uint8), np.zeros((32, 64), np.uint8))


def test_host_sgm_stereo(tmp_path):
    from sgm_probe import SgmHostProbe
    probe = SgmHostProbe(tmp_path)
    left, right, _ = sgm_util.make_pair(48, 128, 32, 7101)
    probe.parse("StereoAlgorithm = SGM\nnumberOfDisparities = 32\n", tmp_path)
    want = ref.compute(left, right, 32)["disparity"]
    bf = float(np.float32(BASELINE * 718.856))
    assert probe.compute(left, right).tobytes() == want.tobytes()
    assert probe.depth(left, right, bf).tobytes() == sgm_util.disparity_to_depth(want, bf).tobytes()
    probe.release()


def _stereo_pair(T_wc, K, size, tex, baseline=BASELINE):
    from photobundle_amd import synthetic
    left, z = synthetic.render_frame(T_wc, K, size, tex)
    T_r = T_wc.copy()
    T_r[:3, 3] = T_wc[:3, 3] + T_wc[:3, 0] * baseline
    right, _ = synthetic.render_frame(T_r, K, size, tex)
    return left, right, z


def _write_pgm(path, im):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        f.write(im.tobytes())


def _sequence(tmp, tag, n_frames, seed):
    """Rendered stereo sequence the way tests/test_gpu_stereo.py builds its own: the reference's poor initial trajectory, ground
    truth = that trajectory with a small error removed; directories for DepthSource = stereo with both calibration formats and
    for DepthSource = files fed with StereoSGM.compute's depth."""
    from photobundle_amd import se3, synthetic
    from photobundle_amd.stereo import StereoSGM
    size, K = synthetic.KITTI_SIZE, synthetic.KITTI_K
    init_local = np.loadtxt(os.path.join(FIX, "data", "kitti_init_poor", "00.txt")).reshape(-1, 3, 4)[:n_frames]
    rng = np.random.default_rng(seed)
    T_gt = [np.eye(4)]
    for i in range(1, n_frames):
        Lp = np.eye(4)
        Lp[:3, :] = init_local[i]
        P = np.eye(4)
        P[:3, :3] = se3.angle_axis_to_matrix(np.deg2rad(rng.normal(0.0, 0.05, 3)))
        P[:3, 3] = rng.normal(0.0, 0.01, 3)
        T_gt.append(T_gt[-1] @ np.linalg.inv(np.linalg.inv(P) @ Lp))
    tex = synthetic.Texture()
    dirs = {n: os.path.join(tmp, tag + "_" + n) for n in ("stereo", "files", "kitti")}
    for d in dirs.values():
        os.makedirs(d)
    p1_03 = -K[0] * BASELINE
    base = -p1_03 / K[0]
    P0 = np.array([[K[0], 0, K[2], 0], [0, K[1], K[3], 0], [0, 0, 1, 0]])
    P1 = P0.copy()
    P1[0, 3] = p1_03
    with open(os.path.join(dirs["kitti"], "calib.txt"), "w") as f:
        for name, P in (("P0", P0), ("P1", P1), ("P2", P0), ("P3", P1)):
            f.write(name + ": " + " ".join("%r" % float(v) for v in P.reshape(-1)) + "\n")
    for n in ("stereo", "files"):
        with open(os.path.join(dirs[n], "calib.txt"), "w") as f:
            f.write("%r %r %r %r %r\n" % (K[0], K[1], K[2], K[3], base))
    bf = float(np.float32(base * K[0]))
    with StereoSGM(size[0], size[1], **REF_CFG) as s:
        for i, T in enumerate(T_gt):
            left, right, _ = _stereo_pair(T, K, size, tex)
            for d in dirs.values():
                _write_pgm(os.path.join(d, "image_%06d.pgm" % i), left)
            for n in ("stereo", "kitti"):
                _write_pgm(os.path.join(dirs[n], "right_%06d.pgm" % i), right)
            _, z = s.compute(left, right, bf)
            assert (z > 0).mean() > 0.5
            z.tofile(os.path.join(dirs["files"], "depth_%06d.bin" % i))
    T_init = [np.eye(4)]
    for i in range(1, n_frames):
        Lp = np.eye(4)
        Lp[:3, :] = init_local[i]
        T_init.append(T_init[-1] @ np.linalg.inv(Lp))
    return dirs, T_gt, T_init


def _config(tmp, name, data_dir, source):
    cfg_text = open(os.path.join(FIX, "config", "kitti_stereo.cfg")).read()
    cfg_text = re.sub(r"(?im)^\s*StereoAlgorithm\s*=.*$", "", cfg_text)
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write(cfg_text.replace("../data/", os.path.join(tmp, "data") + "/"))
        f.write("\nStereoAlgorithm = SGM\nDataDirectory = %s\nDepthSource = %s\nverbose = 0\n" % (data_dir, source))
    return cfg


def _errors(poses_text, T_gt, T_init):
    n = len(T_gt)
    refined = np.array([[float(v) for v in ln.split()] for ln in poses_text.strip().split("\n")]).reshape(-1, 3, 4)
    assert refined.shape[0] == n and np.isfinite(refined).all()
    e_ref = np.array([np.linalg.norm(refined[i][:, 3] - T_gt[i][:3, 3]) for i in range(n)])
    e_ini = np.array([np.linalg.norm(T_init[i][:3, 3] - T_gt[i][:3, 3]) for i in range(n)])
    return e_ref, e_ini


# First run on the MI355X: refined 0.009 .. 0.045 m against initial 0.023 .. 0.092 m (both grow along the sequence with the drift of the
# poor initial trajectory).  Later runs are held to twice the worst frame of that run, as tests/test_gpu_stereo.py does.
WORST_FRAME_FIRST_RUN = 0.0454


@pytest.mark.timeout(900)
def test_run_kitti_stereo_algorithm_sgm(tmp_path):
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    tmp = str(tmp_path)
    n_frames = 7
    shutil.copytree(os.path.join(FIX, "data"), os.path.join(tmp, "data"))
    dirs, T_gt, T_init = _sequence(tmp, "a", n_frames, 20261016)
    outs = {}
    for name, src in (("stereo", "stereo"), ("kitti", "stereo"), ("files", "files")):
        cfg = _config(tmp, name, dirs[name], src)
        out, res = os.path.join(tmp, name + "_poses.txt"), os.path.join(tmp, name + "_results.txt")
        r = subprocess.run([RUN, "-c", cfg, "-o", out, "-r", res, "-p"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = (open(out).read(), open(res).read())
    assert outs["stereo"] == outs["files"]
    assert outs["kitti"] == outs["files"]
    used = re.findall(r"^result frame (\d+)", outs["stereo"][1], flags=re.M)
    assert [int(u) for u in used] == list(range(4, n_frames))           # slidingWindowSize = 5
    e_ref, e_ini = _errors(outs["stereo"][0], T_gt, T_init)
    print("run_kitti StereoAlgorithm = SGM: translation error to ground truth per frame, refined %s m, initial %s m" % (
        np.array2string(e_ref, precision=4), np.array2string(e_ini, precision=4)))
    assert (e_ref[1:] < e_ini[1:]).all()
    assert e_ref.max() <= 2 * WORST_FRAME_FIRST_RUN


@pytest.mark.timeout(900)
def test_run_kitti_batch_of_two_sgm_sequences(tmp_path):
    """-b with two sequences, each DepthSource = stereo + StereoAlgorithm = SGM: the same pose and result files as each sequence's
    DepthSource = files run fed with StereoSGM.compute's depth."""
    assert os.path.exists(RUN)
    tmp = str(tmp_path)
    n_frames = 6
    shutil.copytree(os.path.join(FIX, "data"), os.path.join(tmp, "data"))
    args, singles, batch = [RUN, "-p"], [], []
    for tag, seed in (("a", 1), ("b", 2)):
        dirs, _, _ = _sequence(tmp, tag, n_frames, seed)
        cfg = _config(tmp, tag + "_files", dirs["files"], "files")
        out, res = os.path.join(tmp, tag + "_files_poses.txt"), os.path.join(tmp, tag + "_files_results.txt")
        r = subprocess.run([RUN, "-c", cfg, "-o", out, "-r", res, "-p"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        singles.append((open(out).read(), open(res).read()))
        out, res = os.path.join(tmp, tag + "_batch_poses.txt"), os.path.join(tmp, tag + "_batch_results.txt")
        args += ["-b", "%s:%s:%s" % (_config(tmp, tag + "_stereo", dirs["stereo"], "stereo"), out, res)]
        batch.append((out, res))
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for (out, res), want in zip(batch, singles):
        assert (open(out).read(), open(res).read()) == want
    assert singles[0] != singles[1]
