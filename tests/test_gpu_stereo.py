"""-m gpu: the stereo block matcher (include/pba_stereo.h) on the MI355X against the numpy restatement of the spec
(tests/stereo_bm_ref.py), bit for bit; its accuracy on a rendered stereo pair; the host StereoAlgorithm's fused depth against
run + disparityToDepth; and run_kitti with DepthSource = stereo end to end."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stereo_bm_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
FIX = os.path.join(ROOT, "tests", "golden", "configs0")
BASELINE = 0.5372
REF_CFG = dict(number_of_disparities=128, sad_window_size=9, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15)


def _stereo_pair(T_wc, K, size, tex, baseline=BASELINE):
    """Left view from T_wc and the right view from the camera offset by +baseline along its own x axis."""
    from photobundle_amd import synthetic
    left, z = synthetic.render_frame(T_wc, K, size, tex)
    T_r = T_wc.copy()
    T_r[:3, 3] = T_wc[:3, 3] + T_wc[:3, 0] * baseline
    right, _ = synthetic.render_frame(T_r, K, size, tex)
    return left, right, z


def _check(left, right, bf=386.0, **params):
    from photobundle_amd.stereo import StereoBM
    p = ref.default_params(**params)
    want = ref.bm(left, right, p)
    with StereoBM(left.shape[0], left.shape[1], **params) as s:
        d, z = s.compute(left, right, bf)
        pl, pr = s.prefiltered()
        assert np.array_equal(pl, ref.prefilter(left, p["pre_filter_cap"]))
        assert np.array_equal(pr, ref.prefilter(right, p["pre_filter_cap"]))
        bad = np.argwhere(d != want)
        assert bad.size == 0, "%d of %d pixels differ, first %s: got %d want %d (%s)" % (
            len(bad), d.size, bad[0], d[tuple(bad[0])], want[tuple(bad[0])], params)
        assert z.tobytes() == ref.depth_from_disp16(want, bf).tobytes()
        d2, z2 = s.compute(left, right, bf)
        assert d2.tobytes() == d.tobytes() and z2.tobytes() == z.tobytes()
        d3, none = s.compute(left, right, bf, depth=False)
        assert none is None and d3.tobytes() == d.tobytes()
    return d, want


@pytest.fixture(scope="module")
def kitti_pair():
    from photobundle_amd import synthetic
    T = np.eye(4)
    return _stereo_pair(T, synthetic.KITTI_K, synthetic.KITTI_SIZE, synthetic.Texture())


def test_kitti_pair_bit_exact_and_accurate(kitti_pair):
    from photobundle_amd import synthetic
    left, right, z_gt = kitti_pair
    bf = np.float32(BASELINE * synthetic.KITTI_K[0])
    d, _ = _check(left, right, bf=float(bf), **REF_CFG)
    assert np.isfinite(z_gt).all()
    valid = d != -16
    frac_filtered = 1.0 - valid.mean()
    gt = (BASELINE * synthetic.KITTI_K[0]) / z_gt.astype(np.float64)
    err = np.abs(d[valid] / 16.0 - gt[valid])
    ok = (err <= 1.0).mean()
    print("KITTI-size rendered pair: %.1f%% FILTERED; %.2f%% of the rest within 1 px of Bf/z (median error %.3f px)" % (
        100 * frac_filtered, 100 * ok, np.median(err)))
    assert ok >= 0.95
    assert frac_filtered < 0.6


@pytest.mark.parametrize("shape,params", [
    ((120, 300), dict(number_of_disparities=16, sad_window_size=5)),
    ((120, 300), dict(number_of_disparities=64, sad_window_size=9, min_disparity=-8)),
    ((96, 400), dict(number_of_disparities=256, sad_window_size=21, min_disparity=5, uniqueness_ratio=0, texture_threshold=0)),
    ((375, 1000), dict(number_of_disparities=128, sad_window_size=9, pre_filter_cap=63)),
    ((101, 300), dict(number_of_disparities=32, sad_window_size=21, uniqueness_ratio=3, texture_threshold=500)),
    ((101, 300), dict(number_of_disparities=16, sad_window_size=7, min_disparity=-20, uniqueness_ratio=0, texture_threshold=0)),
    ((160, 400), dict(number_of_disparities=16, sad_window_size=151, uniqueness_ratio=0)),   # LDS does not hold the tile: global path
])
def test_random_pairs_bit_exact(shape, params):
    rng = np.random.default_rng(sum(shape) + sum(params.values()))
    L = rng.integers(0, 256, shape).astype(np.uint8)
    shift = rng.integers(-40, 40, shape[0])
    R = np.stack([np.roll(L[y], -abs(int(shift[y])) % 24) for y in range(shape[0])])
    R = np.clip(R.astype(int) + rng.integers(-25, 26, shape), 0, 255).astype(np.uint8)
    d, want = _check(L, R, **params)
    assert (d != ref.filtered_value(ref.default_params(**params))).any()


def test_smooth_pairs_bit_exact():
    # low-texture content: many texture rejections, ties and flat cost curves
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:75, 0:260]
    L = (128 + 60 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.uint8)
    L[20:40, 100:140] = 90
    R = np.roll(L, -6, axis=1)
    R = np.clip(R.astype(int) + rng.integers(-2, 3, R.shape), 0, 255).astype(np.uint8)
    for params in (dict(number_of_disparities=32, sad_window_size=5), dict(number_of_disparities=48, sad_window_size=11, min_disparity=-3)):
        _check(L, R, **params)


@pytest.mark.parametrize("shape,params", [
    ((9, 9), dict(number_of_disparities=16, sad_window_size=9)),          # valid region empty: all FILTERED
    ((40, 20), dict(number_of_disparities=16, sad_window_size=5)),        # narrower than ndisp + window
    ((5, 64), dict(number_of_disparities=16, sad_window_size=5, texture_threshold=0, uniqueness_ratio=0)),   # one valid row
    ((7, 5), dict(number_of_disparities=16, sad_window_size=5, min_disparity=-16)),
    ((33, 90), dict(number_of_disparities=16, sad_window_size=5, min_disparity=-70, texture_threshold=0)),
])
def test_degenerate_sizes(shape, params):
    rng = np.random.default_rng(3)
    L = rng.integers(0, 256, shape).astype(np.uint8)
    R = rng.integers(0, 256, shape).astype(np.uint8)
    _check(L, R, **params)


def test_invalid_handle_use():
    from photobundle_amd.stereo import StereoBM, StereoError
    with StereoBM(32, 64, number_of_disparities=16, sad_window_size=5) as s:
        with pytest.raises(StereoError, match="before pba_stereo_compute"):
            s.prefiltered()
        with pytest.raises(ValueError):
            s.compute(np.zeros((32, 63), np.uint8), np.zeros((32, 64), np.uint8))


def test_host_fused_depth_equals_run_then_disparity_to_depth(tmp_path, kitti_pair):
    from photobundle_amd import synthetic
    from stereo_probe import HostProbe
    left, right, _ = kitti_pair
    probe = HostProbe(tmp_path)
    cfg = open(os.path.join(FIX, "config", "kitti_stereo.cfg")).read()
    _, inv = probe.parse(cfg, tmp_path)
    bf = float(np.float32(BASELINE * synthetic.KITTI_K[0]))
    dmap = probe.run(left, right)
    zmap = probe.depth(left, right, bf)
    want = ref.bm(left, right, ref.default_params(**REF_CFG))
    assert dmap.tobytes() == (want.astype(np.float32) * np.float32(0.0625)).tobytes()
    assert (dmap[want == -16] == inv).all()
    assert zmap.tobytes() == probe.disparity_to_depth(dmap, bf).tobytes()
    assert zmap.tobytes() == ref.depth_from_disp16(want, bf).tobytes()
    probe.release()


def _write_pgm(path, im):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        f.write(im.tobytes())


@pytest.mark.timeout(900)
def test_run_kitti_depth_source_stereo(tmp_path):
    from photobundle_amd import se3, synthetic
    from photobundle_amd.stereo import StereoBM
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    tmp = str(tmp_path)
    size, K = synthetic.KITTI_SIZE, synthetic.KITTI_K
    n_frames = 7
    init_local = np.loadtxt(os.path.join(FIX, "data", "kitti_init_poor", "00.txt")).reshape(-1, 3, 4)[:n_frames]
    rng = np.random.default_rng(20261016)
    T_gt = [np.eye(4)]
    for i in range(1, n_frames):                   # ground truth = initial local pose with a small error removed (test_gpu_configs0)
        Lp = np.eye(4)
        Lp[:3, :] = init_local[i]
        P = np.eye(4)
        P[:3, :3] = se3.angle_axis_to_matrix(np.deg2rad(rng.normal(0.0, 0.05, 3)))
        P[:3, 3] = rng.normal(0.0, 0.01, 3)
        T_gt.append(T_gt[-1] @ np.linalg.inv(np.linalg.inv(P) @ Lp))
    tex = synthetic.Texture()
    stereo_dir, files_dir, kitti_dir = (os.path.join(tmp, n) for n in ("stereo", "files", "kitti"))
    for d in (stereo_dir, files_dir, kitti_dir):
        os.makedirs(d)
    # KITTI's calib.txt: P0 = [K | 0], P1 = [K | -fx b]; baseline = -P1(0,3) / P1(0,0) in double, as the driver computes it
    p1_03 = -K[0] * BASELINE
    base = -p1_03 / K[0]
    P0 = np.array([[K[0], 0, K[2], 0], [0, K[1], K[3], 0], [0, 0, 1, 0]])
    P1 = P0.copy()
    P1[0, 3] = p1_03
    with open(os.path.join(kitti_dir, "calib.txt"), "w") as f:
        for name, P in (("P0", P0), ("P1", P1), ("P2", P0), ("P3", P1)):
            f.write(name + ": " + " ".join("%r" % float(v) for v in P.reshape(-1)) + "\n")
    for d in (stereo_dir, files_dir):
        with open(os.path.join(d, "calib.txt"), "w") as f:
            f.write("%r %r %r %r %r\n" % (K[0], K[1], K[2], K[3], base))
    bf = float(np.float32(base * K[0]))
    with StereoBM(size[0], size[1], **REF_CFG) as s:
        for i, T in enumerate(T_gt):
            left, right, _ = _stereo_pair(T, K, size, tex, baseline=BASELINE)
            for d in (stereo_dir, files_dir, kitti_dir):
                _write_pgm(os.path.join(d, "image_%06d.pgm" % i), left)
            for d in (stereo_dir, kitti_dir):
                _write_pgm(os.path.join(d, "right_%06d.pgm" % i), right)
            _, z = s.compute(left, right, bf, disparity=False)
            z.tofile(os.path.join(files_dir, "depth_%06d.bin" % i))
    cfg_text = open(os.path.join(FIX, "config", "kitti_stereo.cfg")).read()
    shutil.copytree(os.path.join(FIX, "data"), os.path.join(tmp, "data"))
    outs = {}
    for name, d, src in (("stereo", stereo_dir, "stereo"), ("kitti", kitti_dir, "stereo"), ("files", files_dir, "files")):
        cfg = os.path.join(tmp, name + ".cfg")
        with open(cfg, "w") as f:
            f.write(cfg_text.replace("../data/", os.path.join(tmp, "data") + "/"))
            f.write("\nDataDirectory = %s\nDepthSource = %s\nverbose = 0\n" % (d, src))
        out, res = os.path.join(tmp, name + "_poses.txt"), os.path.join(tmp, name + "_results.txt")
        r = subprocess.run([RUN, "-c", cfg, "-o", out, "-r", res, "-p"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = (open(out).read(), open(res).read())
    assert outs["stereo"] == outs["files"]
    assert outs["kitti"] == outs["files"]
    used = re.findall(r"^result frame (\d+)", outs["stereo"][1], flags=re.M)
    assert [int(u) for u in used] == list(range(4, n_frames))           # slidingWindowSize = 5
    refined = np.array([[float(v) for v in ln.split()] for ln in outs["stereo"][0].strip().split("\n")]).reshape(-1, 3, 4)
    assert refined.shape[0] == n_frames
    # initial world poses from the initial local poses (trajectory.cc: T_w_i = T_w_{i-1} inv(T_i))
    T_init = [np.eye(4)]
    for i in range(1, n_frames):
        Lp = np.eye(4)
        Lp[:3, :] = init_local[i]
        T_init.append(T_init[-1] @ np.linalg.inv(Lp))
    e_ref = np.array([np.linalg.norm(refined[i][:, 3] - T_gt[i][:3, 3]) for i in range(n_frames)])
    e_ini = np.array([np.linalg.norm(T_init[i][:3, 3] - T_gt[i][:3, 3]) for i in range(n_frames)])
    print("run_kitti DepthSource = stereo: translation error to ground truth per frame, refined %s m, initial %s m" % (
        np.array2string(e_ref, precision=4), np.array2string(e_ini, precision=4)))
    assert np.isfinite(refined).all()
    # bar from the first run on the MI355X: refined 0.002 .. 0.012 m against initial 0.02 .. 0.09 m (the drift of the poor initial
    # trajectory grows along the sequence).  Held to twice the observed worst frame, and every free frame must beat its initial pose.
    assert e_ref.max() <= 0.025
    assert (e_ref[1:] < e_ini[1:]).all()
