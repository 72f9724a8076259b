"""CPU checks of the stereo block matcher's spec and surfaces (DESIGN.md "Stereo block matching"): the two CPU restatements of
tests/stereo_bm_ref.py agree, hand-checked cases of the spec, disparityToDepth's edge values, the host StereoAlgorithm's config
keys and refusals, and the C-ABI of include/pba_stereo.h (symbols, parameter validation before any device call)."""
import os
import re

import numpy as np
import pytest

import stereo_bm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(rng, H, W, shift=4, noise=20):
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = np.clip(np.roll(L, -shift, axis=1).astype(int) + rng.integers(-noise, noise + 1, (H, W)), 0, 255).astype(np.uint8)
    return L, R


CASES = [(H, min_d, nd, w, u, t)
         for H, min_d, nd, w, u, t in [
             (13, 0, 16, 5, 15, 10), (14, 0, 16, 5, 0, 0), (15, -8, 16, 9, 15, 0), (16, -8, 32, 5, 0, 10),
             (13, 5, 16, 11, 15, 10), (14, 5, 32, 9, 0, 0), (17, 0, 32, 9, 15, 10), (12, -8, 16, 11, 15, 10000),
             (15, 5, 16, 5, 0, 10000), (18, 0, 16, 11, 0, 10)]]


@pytest.mark.parametrize("H,min_d,nd,w,uniq,tex", CASES)
def test_loop_and_numpy_restatements_agree(H, min_d, nd, w, uniq, tex):
    rng = np.random.default_rng(1000 + H * 7 + nd + w + uniq + (tex % 97) + min_d)
    W = nd + max(0, min_d) + w + 12
    L, R = _pair(rng, H, W)
    p = ref.default_params(number_of_disparities=nd, min_disparity=min_d, sad_window_size=w, uniqueness_ratio=uniq,
                           texture_threshold=tex)
    a = ref.bm_loop(L, R, p)
    b = ref.bm(L, R, p)
    assert a.dtype == b.dtype == np.int16
    assert np.array_equal(a, b)
    assert np.array_equal(ref.prefilter_loop(L, 31), ref.prefilter(L, 31))
    if tex >= 10000:
        assert (a == ref.filtered_value(p)).all()


def test_prefilter_borders():
    rng = np.random.default_rng(3)
    for H in (7, 8):
        I = rng.integers(0, 256, (H, 20)).astype(np.uint8)
        P = ref.prefilter(I, 31)
        assert (P[:, 0] == 31).all() and (P[:, -1] == 31).all()
        assert ((P[-1] == 31).all()) == (H % 2 == 1)           # the odd-H last row is cap (OpenCV filters rows in pairs)
        # reflect-101: row -1 is row 1, so a horizontal ramp's first row is the interior value
    ramp = np.tile(np.arange(20, dtype=np.uint8) * 3, (8, 1))
    P = ref.prefilter(ramp, 31)
    assert (P[:, 1:-1] == min(4 * 6, 31) + 31).all()         # (3+3)*(1+2+1) = 24 inside the cap
    P = ref.prefilter(ramp * 4, 7)
    assert (P[:, 1:-1] == 14).all()                          # clamped at cap, + cap


def test_constant_and_narrow_images_are_all_filtered():
    p = ref.default_params(number_of_disparities=16, sad_window_size=5, texture_threshold=10)
    c = np.full((12, 60), 77, np.uint8)
    assert (ref.bm(c, c, p) == ref.filtered_value(p)).all()     # texture 0 < 10
    assert (ref.bm_loop(c, c, p) == ref.filtered_value(p)).all()
    rng = np.random.default_rng(5)
    L, R = _pair(rng, 12, 15)                                   # narrower than ndisp + window: empty valid region
    out = ref.bm(L, R, p)
    assert (out == -16).all() and out.dtype == np.int16
    p2 = ref.default_params(number_of_disparities=16, sad_window_size=5, min_disparity=-3)
    assert (ref.bm(L, R, p2) == (-3 - 1) * 16).all()


def test_tie_goes_to_the_larger_disparity_and_edge_mirror():
    # a periodic texture of period 4 makes D and D + 4 equally good: the larger wins
    H, W = 9, 60
    base = np.array([0, 200, 40, 160], np.uint8)
    L = np.tile(np.tile(base, W // 4), (H, 1))
    R = L.copy()
    p = ref.default_params(number_of_disparities=16, sad_window_size=5, uniqueness_ratio=0, texture_threshold=0)
    out = ref.bm_loop(L, R, p)
    x0, x1, y0, y1 = ref.valid_region(H, W, p)
    inner = out[y0:y1, x0:x1 - 3]             # away from the constant (cap) last prefiltered column
    # cost 0 at D = 0, 4, 8, 12: D* = 12, the largest; the sub-pixel term moves the output by at most half a pixel
    assert (np.abs(inner.astype(int) - 12 * 16) <= 8).all(), np.unique(inner)
    assert np.array_equal(out, ref.bm(L, R, p))
    # D* = maxD: c_hi := c_lo, so frac = 0 and out = maxD * 16 exactly; same at minD with c_lo := c_hi
    rng = np.random.default_rng(9)
    L = rng.integers(0, 256, (9, 70)).astype(np.uint8)
    for shift, D in ((15, 15), (0, 0)):
        R = np.roll(L, -shift, axis=1)
        out = ref.bm_loop(L, R, p)
        x0, x1, y0, y1 = ref.valid_region(9, 70, p)
        inner = out[y0:y1, x0:min(x1, 70 - shift - 3)]
        assert (inner == D * 16).all(), (D, np.unique(inner))
        assert np.array_equal(out, ref.bm(L, R, p))


def test_subpixel_truncates_toward_zero_and_floors_the_shift():
    # C truncating division of a negative numerator and the arithmetic shift of a negative disparity
    p = ref.default_params(number_of_disparities=16, sad_window_size=5, min_disparity=-20, uniqueness_ratio=0, texture_threshold=0)
    rng = np.random.default_rng(11)
    L = rng.integers(0, 256, (11, 64)).astype(np.uint8)
    R = np.clip(np.roll(L, 9, axis=1).astype(int) + rng.integers(-30, 31, L.shape), 0, 255).astype(np.uint8)
    a, b = ref.bm_loop(L, R, p), ref.bm(L, R, p)
    assert np.array_equal(a, b)
    x0, x1, y0, y1 = ref.valid_region(11, 64, p)
    inner = a[y0:y1, x0:x1]
    assert (inner < 0).all() and len(np.unique(inner % 16)) > 1     # negative disparities with fractional parts


def test_disparity_to_depth_edges():
    bf = np.float32(386.1726)
    d = np.array([0.01, np.nextafter(np.float32(0.01), np.float32(1)), 0.0, -0.0, -3.5, -1.0, 0.0625, 12.25, 127.9375],
                 np.float32)
    z = ref.disparity_to_depth(d, bf)
    assert z[0] == np.float32(-0.1) and z[2] == z[3] == z[4] == z[5] == np.float32(-0.1)
    assert z[1] == bf * (np.float32(1) / d[1])
    assert z[6] == bf * np.float32(16.0) and z[7] == bf * (np.float32(1) / np.float32(12.25))
    # FILTERED of minD = 0 is -16 -> -1 px -> invalid; of minD = 3 it is 32 -> 2 px -> a (meaningless) positive depth, as specified
    assert ref.depth_from_disp16(np.array([-16], np.int16), bf)[0] == np.float32(-0.1)
    assert ref.depth_from_disp16(np.array([32], np.int16), bf)[0] == bf * np.float32(0.5)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from stereo_probe import HostProbe
    return HostProbe(tmp_path_factory.mktemp("stereo_probe"))


def test_host_disparity_to_depth_matches_the_spec(probe):
    rng = np.random.default_rng(13)
    d = (rng.integers(-300, 2048, (37, 41)).astype(np.float32) * np.float32(0.0625))
    d[0, :6] = [0.01, 0.0, -0.0, -1.0, -0.1, np.nextafter(np.float32(0.01), np.float32(1))]
    for bf in (386.1726, 0.5372 * 718.856, 1.0):
        z = probe.disparity_to_depth(d, bf)
        assert z.tobytes() == ref.disparity_to_depth(d, np.float32(bf)).tobytes()
    assert (z[0, :5] == np.float32(-0.1)).all() and z[0, 5] > 0


def test_host_stereo_algorithm_config(probe, tmp_path):
    # the reference cfg's keys: BlockMatching, 128 disparities, 9x9 window; the rest at the reference defaults
    cfg = open(os.path.join(ROOT, "tests", "golden", "configs0", "config", "kitti_stereo.cfg")).read()
    p, inv = probe.parse(cfg, tmp_path)
    assert p == dict(pre_filter_type=1, pre_filter_size=9, pre_filter_cap=31, sad_window_size=9, min_disparity=0,
                     number_of_disparities=128, texture_threshold=10, uniqueness_ratio=15, speckle_window_size=0, speckle_range=0,
                     try_smaller_windows=0, disp12_max_diff=-1)
    assert inv == -1.0
    p, inv = probe.parse("numberOfDisparities = 64\nminDisparity = -4\nstereoalgorithm = bm\npreFilterCap = 63\n", tmp_path)
    assert (p["number_of_disparities"], p["min_disparity"], p["pre_filter_cap"], p["sad_window_size"]) == (64, -4, 63, 15)
    assert inv == -5.0
    for text, msg in [("StereoAlgorithm = BlockMatching\n", "no key numberOfDisparities"),
                      ("StereoAlgorithm = SGBM\nnumberOfDisparities = 64\n", "not supported"),
                      ("StereoAlgorithm = SemiGlobalMatching\nnumberOfDisparities = 64\n", "not supported"),
                      ("StereoAlgorithm = RSGM\nnumberOfDisparities = 64\n", "not supported"),
                      ("StereoAlgorithm = Census\nnumberOfDisparities = 64\n", "Unknown stereo algorithm"),
                      ("numberOfDisparities = 64\nspeckleWindowSize = 100\n", "speckleWindowSize"),
                      ("numberOfDisparities = 64\ntrySmallerWindows = 1\n", "trySmallerWindows"),
                      ("numberOfDisparities = 64\ndisp12MaxDiff = 1\n", "disp12MaxDiff"),
                      ("numberOfDisparities = 64\npreFilterType = 0\n", "preFilterType"),
                      ("numberOfDisparities = 100\n", "multiple of 16"),
                      ("numberOfDisparities = 64\nSADWindowSize = 8\n", "SADWindowSize")]:
        with pytest.raises(RuntimeError, match=msg):
            probe.parse(text, tmp_path)


def test_library_exports_every_stereo_symbol():
    from photobundle_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pba_stereo.h")).read()
    declared = sorted(set(re.findall(r"\b(pba_stereo_[a-z0-9_]+)\s*\(", header)))
    assert declared
    for name in declared:
        assert hasattr(L, name), "libpba_hip.so does not export %s" % name
    assert sorted(_lib.STEREO_SYMBOLS) == declared


def test_default_params_are_the_reference_defaults():
    from photobundle_amd import stereo
    p = stereo.default_params()
    assert [getattr(p, f) for f in stereo.PARAM_FIELDS] == [1, 9, 31, 15, 0, 0, 10, 15, 0, 0, 0, -1]
    assert [getattr(p, f) for f in stereo.PARAM_FIELDS] == [ref.default_params()[f] for f in stereo.PARAM_FIELDS]


@pytest.mark.parametrize("kw,msg", [
    (dict(number_of_disparities=0), "numberOfDisparities"), (dict(number_of_disparities=24), "numberOfDisparities"),
    (dict(pre_filter_type=0), "NORMALIZED_RESPONSE"), (dict(pre_filter_cap=0), "preFilterCap"), (dict(pre_filter_cap=64), "preFilterCap"),
    (dict(sad_window_size=4), "SADWindowSize"), (dict(sad_window_size=257), "SADWindowSize"), (dict(sad_window_size=3), "SADWindowSize"),
    (dict(sad_window_size=41), "min\\(rows, cols\\)"), (dict(pre_filter_size=4), "preFilterSize"),
    (dict(texture_threshold=-1), "textureThreshold"), (dict(uniqueness_ratio=-1), "uniquenessRatio"),
    (dict(speckle_window_size=50), "speckleWindowSize"), (dict(try_smaller_windows=1), "trySmallerWindows"),
    (dict(disp12_max_diff=0), "disp12MaxDiff"), (dict(min_disparity=2040), "int16"), (dict(min_disparity=-2048), "int16")])
def test_invalid_params_are_refused_before_the_device(kw, msg):
    import ctypes as C
    from photobundle_amd import stereo
    params = dict(number_of_disparities=16)
    params.update(kw)
    with pytest.raises(stereo.StereoError, match=msg) as ei:
        stereo.StereoBM(40, 64, **params)
    assert ei.value.status == -1                       # PBA_ERR_INVALID
    L = stereo._stereo_lib()
    assert L.pba_stereo_validate_params(40, 64, C.byref(stereo.default_params(**params))) == -1
    assert re.search(msg, L.pba_stereo_last_error(None).decode())


def test_valid_params_pass_validation_and_no_cpu_fallback():
    import ctypes as C
    import torch
    from photobundle_amd import stereo
    L = stereo._stereo_lib()
    p = stereo.default_params(number_of_disparities=128, sad_window_size=9)
    assert L.pba_stereo_validate_params(376, 1241, C.byref(p)) == 0
    assert L.pba_stereo_validate_params(0, 0, C.byref(stereo.default_params(number_of_disparities=16, sad_window_size=255))) == 0
    if torch.cuda.is_available():
        return
    with pytest.raises(stereo.StereoError, match="no HIP device") as ei:
        stereo.StereoBM(376, 1241, number_of_disparities=128, sad_window_size=9)
    assert ei.value.status == -3                       # PBA_ERR_NO_DEVICE
