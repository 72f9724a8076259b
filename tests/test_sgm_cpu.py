"""The semi-global matcher without a GPU: the numpy restatement (tests/sgm_ref.py) against the fixtures made by the reference's own
code (tests/golden/sgm, tools/make_sgm_golden.py), bit for bit; the speckle filter's component rule against a literal stack-based
flood fill; hand-checked small cases; the exported symbols and every refusal of pba_sgm_validate_params, the Python class and the
host SgmStereo::Config::fromConfigFile."""
import os
import re

import numpy as np
import pytest

import sgm_ref as ref
import sgm_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sgm_util.load_cases()
LARGEST_FIXTURE = os.path.getsize(os.path.join(ROOT, "tests", "golden", "referee_traces.json"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    left, right = sgm_util.case_pair(case)
    assert left.shape == (case["rows"], case["cols"])
    assert sgm_util.sha256(left, right) == case["input_sha256"]          # before anything is compared
    p = sgm_util.params_of(case)
    out = ref.compute(left, right, p.pop("numberOfDisparities"), **p)
    whole, rows = sgm_util.case_expected(case)
    if whole is not None:
        assert sgm_util.sha256(whole) == case["disp_scaled_sha256"]
        bad = np.argwhere(out["disp_scaled"] != whole)
        assert bad.size == 0, "%d of %d pixels differ, first %s" % (len(bad), whole.size, bad[0])
        assert out["disparity"].tobytes() == sgm_util.float_map(whole, p["disparityFactor"]).tobytes()
    else:
        index, stored = rows
        assert np.array_equal(out["disp_scaled"][index], stored)
    assert sgm_util.sha256(out["disp_scaled"]) == case["disp_scaled_sha256"]
    assert sgm_util.sha256(out["disparity"]) == case["disparity_sha256"]
    if case["kind"] == "main":       # no main case passes on maps the filters never touched
        assert ((out["disp_left_raw"] != 0) & (out["disp_left_filtered"] == 0)).any(), "the speckle filter zeroes nothing"
        assert ((out["disp_left_filtered"] != 0) & (out["disp_scaled"] == 0)).any(), "the left-right check zeroes nothing"


def test_fixture_files_are_small_and_cover_the_issue():
    names = {c["name"] for c in CASES}
    shapes = {(c["rows"], c["cols"], c["ndisp"]) for c in CASES if c["kind"] == "main"}
    assert shapes == {(24, 64, 16), (48, 128, 32), (96, 256, 64), (376, 1241, 128)}
    assert (37, 131, 48) in {(c["rows"], c["cols"], c["ndisp"]) for c in CASES}
    assert any(c["cols"] == c["ndisp"] for c in CASES)
    assert any(c["rows"] == sgm_util.params_of(c)["windowRadius"] + 1 for c in CASES)
    for want in ("cap127", "census1", "window0", "window5", "window9", "weight1", "penalty_0_1", "penalty_3000_12000", "threshold0",
                 "threshold3", "factor16", "factor2048"):
        assert "param_" + want in names
    for f in os.listdir(sgm_util.GOLDEN_DIR):
        assert os.path.getsize(os.path.join(sgm_util.GOLDEN_DIR, f)) < LARGEST_FIXTURE, f


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "main"], ids=lambda c: c["name"])
def test_main_cases_are_not_empty(case):
    """The conditions on the main cases, on the committed data: 50-98 % non-zero, >= 90 % of those within 1 px of the planted
    disparity, and (on the restatement's stages) the speckle filter and the left-right check each zero at least one pixel."""
    assert 0.5 <= case["nonzero_share"] <= 0.98
    assert case["within_1px_share"] >= 0.9
    if case["file"] is None:
        index, stored = sgm_util.case_expected(case)[1]
        planted = sgm_util.planted_disparity(case["rows"], case["cols"], case["ndisp"])[index]
        nz = stored != 0
        assert 0.5 <= nz.mean() <= 0.98
        assert (np.abs(stored[nz] / 256.0 - planted[nz]) <= 1.0).mean() >= 0.9
        return
    left, right = sgm_util.case_pair(case)
    whole, _ = sgm_util.case_expected(case)
    planted = sgm_util.planted_disparity(case["rows"], case["cols"], case["ndisp"])
    nz = whole != 0
    assert abs(nz.mean() - case["nonzero_share"]) < 1e-4
    assert (np.abs(whole[nz] / 256.0 - planted[nz]) <= 1.0).mean() >= 0.9
    p = sgm_util.params_of(case)
    out = ref.compute(left, right, p.pop("numberOfDisparities"), **p)
    assert ((out["disp_left_raw"] != 0) & (out["disp_left_filtered"] == 0)).sum() >= 1
    assert ((out["disp_left_filtered"] != 0) & (out["disp_scaled"] == 0)).sum() >= 1


def _flood_fill_filter(image, max_size, max_diff, order):
    """The speckle filter as a literal region-growing loop with a stack that edits the image while it runs; `order` permutes the
    four neighbour checks."""
    img = image.copy()
    H, W = img.shape
    labels = np.zeros((H, W), np.int64)
    small = [False]
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)]
    steps = [steps[i] for i in order]
    for y in range(H):
        for x in range(W):
            if img[y, x] == 0:
                continue
            if labels[y, x] > 0:
                if small[labels[y, x]]:
                    img[y, x] = 0
                continue
            small.append(False)
            cur = len(small) - 1
            labels[y, x] = cur
            stack, count = [(y, x)], 0
            while stack:
                cy, cx = stack.pop()
                count += 1
                v = int(img[cy, cx])
                for dy, dx in steps:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and labels[ny, nx] == 0 and img[ny, nx] != 0 and abs(v - int(img[ny, nx])) <= max_diff:
                        labels[ny, nx] = cur
                        stack.append((ny, nx))
            if count <= max_size:
                small[cur] = True
                img[y, x] = 0
    return img


@pytest.mark.parametrize("seed", range(6))
def test_component_rule_equals_a_stack_flood_fill(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(5, 40)), int(rng.integers(5, 50))
    # plateaus with small steps, holes, and noise: chains whose ends differ by more than the threshold while neighbours do not
    base = (rng.integers(0, 6, (H, W)) * 3 + np.arange(W)[None, :] * int(rng.integers(0, 3))).astype(np.uint16)
    base[rng.random((H, W)) < 0.25] = 0
    base[rng.random((H, W)) < 0.1] += 40
    max_size, max_diff = int(rng.integers(1, 12)), int(rng.integers(1, 6))
    want = ref.speckle_filter(base, max_size, max_diff)
    assert (want != base).any() or max_size == 1
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)):
        assert np.array_equal(_flood_fill_filter(base, max_size, max_diff, order), want)


def test_constant_images():
    """No texture: Sobel = cap everywhere and all census bits set inside, so d = 0 costs nothing anywhere (larger d pays for the census
    codes of the border columns).  A path cost is min(...) - (previous minimum + P2) + cost, so with no cost each of the four paths
    leaves -P2 at d = 0; that is the minimum, the first minimum is d = 0, and the map is 0."""
    img = np.full((12, 40), 90, np.uint8)
    out = ref.compute(img, img, 16, stages=True)
    assert (out["sobel_left"] == 15).all()
    assert out["census_left"][5, 5] == (1 << 25) - 1
    assert out["census_left"][0, 0] == 0b0000000000001110011100111        # rows / columns outside the image give 0 bits
    assert (out["cost_left"][:, :, 0] == 0).all() and (out["sum_left"][:, :, 0] == -4 * 1600).all() and (out["sum_left"] >= -4 * 1600).all()
    assert (out["disp_scaled"] == 0).all() and (out["disparity"] == 0).all()


def test_pure_shift():
    rng = np.random.RandomState(5)
    tex = rng.randint(0, 256, (40, 150)).astype(np.uint8)
    shift = 7
    right, left = tex[:, shift:shift + 120].copy(), tex[:, :120].copy()      # left(x) = right(x - shift)
    out = ref.compute(left, right, 16)
    inner = out["disp_scaled"][4:-4, 40:-8]
    assert (np.abs(inner.astype(np.int32) - shift * 256) <= 32).mean() > 0.99    # the sub-pixel step moves it by < 1/8 px
    assert abs(out["disparity"][10, 60] - shift) <= 0.125


def test_cost_volume_borders_and_saturating_penalties():
    left, right, _ = sgm_util.make_pair(12, 48, 16, 3)
    out = ref.compute(left, right, 16, windowRadius=2, stages=True)
    C = out["cost_left"]
    assert (C[1:, 0, :] == 0).all() and (C[0, 0, :] != 0).any()               # column 0 of rows >= 1 is never written
    assert (C[-2:] == 0).all() and (C[-3, 1:] != 0).any()                     # nor are the bottom windowRadius rows
    assert (C[0, 3, 6:] == C[0, 3, 5]).all()                                  # d > x repeats d = x, for every x of the window (<= 5)
    # P2 close to the int16 limit: pathMin + P2 wraps when truncated to int16, and the path costs saturate
    big = ref.compute(left, right, 16, smoothnessPenaltySmall=3000, smoothnessPenaltyLarge=32767, censusWeightFactor=1.0,
                      sobelCapValue=127, stages=True)
    assert big["sum_left"].max() == 32767 or big["sum_left"].min() == -32768
    assert ref._wrap16(1 + 32767) == -32768 and ref._sat(np.int32(40000)) == 32767


def test_library_exports_every_sgm_symbol():
    from photobundle_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pba_sgm.h")).read()
    declared = sorted(set(re.findall(r"\b(pba_sgm_[a-z0-9_]+)\s*\(", header)))
    assert declared
    for name in declared:
        assert hasattr(L, name), "libpba_hip.so does not export %s" % name
    assert sorted(_lib.SGM_SYMBOLS) == declared
    assert not set(_lib.SGM_SYMBOLS) & set(_lib.STEREO_SYMBOLS)


def test_default_params_are_the_reference_defaults():
    from photobundle_amd import stereo
    p = stereo.sgm_default_params()
    got = {k: getattr(p, f) for k, f in sgm_util.FIELD_OF_KEY.items()}
    assert got == sgm_util.DEFAULTS
    assert set(stereo.SGM_STAGES) == set(ref.STAGES)


# (rows, cols, parameters, the key the message must name)
REFUSALS = [
    (40, 64, dict(number_of_disparities=0), "numberOfDisparities"), (40, 64, dict(number_of_disparities=-16), "numberOfDisparities"),
    (40, 64, dict(number_of_disparities=24), "numberOfDisparities"), (40, 64, dict(number_of_disparities=80), "numberOfDisparities"),
    (40, 64, dict(census_radius=0), "censusRadius"), (40, 64, dict(census_radius=3), "censusRadius"),
    (40, 64, dict(window_radius=-1), "windowRadius"), (40, 64, dict(window_radius=10), "windowRadius"),
    (2, 64, dict(window_radius=2), "windowRadius"), (1, 64, dict(window_radius=1), "windowRadius"),
    (40, 64, dict(smoothness_penalty_small=-1), "smoothnessPenaltySmall"),
    (40, 64, dict(smoothness_penalty_small=100, smoothness_penalty_large=100), "smoothnessPenaltyLarge"),
    (40, 64, dict(smoothness_penalty_small=100, smoothness_penalty_large=50), "smoothnessPenaltyLarge"),
    (40, 64, dict(smoothness_penalty_large=32768), "smoothnessPenaltyLarge"),
    (40, 64, dict(consistency_threshold=-1), "consistencyThreshold"),
    (40, 64, dict(disparity_factor=0.0), "disparityFactor"), (40, 64, dict(disparity_factor=0.5), "disparityFactor"),
    (40, 64, dict(disparity_factor=2.5), "disparityFactor"), (40, 64, dict(disparity_factor=-256.0), "disparityFactor"),
    (40, 64, dict(disparity_factor=4097.0), "disparityFactor"), (40, 64, dict(disparity_factor=float("nan")), "disparityFactor"),
    (40, 64, dict(census_weight_factor=-0.1), "censusWeightFactor"), (40, 64, dict(census_weight_factor=float("nan")), "censusWeightFactor"),
]


@pytest.mark.parametrize("rows,cols,kw,msg", REFUSALS)
def test_invalid_params_are_refused_before_the_device(rows, cols, kw, msg):
    import ctypes as C
    from photobundle_amd import stereo
    params = dict(number_of_disparities=16)
    params.update(kw)
    with pytest.raises(stereo.StereoError, match=msg) as ei:
        stereo.StereoSGM(rows, cols, **params)
    assert ei.value.status == -1                       # PBA_ERR_INVALID, also on a machine with no device
    with pytest.raises(stereo.StereoError, match=msg):
        stereo.sgm_validate_params(rows, cols, **params)
    L = stereo._sgm_lib()
    assert L.pba_sgm_validate_params(rows, cols, C.byref(stereo.sgm_default_params(**params))) == -1
    assert re.search(msg, L.pba_sgm_last_error(None).decode())


def test_valid_params_pass_validation_and_no_cpu_fallback():
    import torch
    from photobundle_amd import stereo
    stereo.sgm_validate_params(376, 1241)
    stereo.sgm_validate_params(0, 0, number_of_disparities=4096, disparity_factor=16)
    # what the reference ran clean with
    for kw in (dict(sobel_cap_value=127), dict(sobel_cap_value=-5), dict(census_radius=1), dict(window_radius=0), dict(window_radius=9),
               dict(census_weight_factor=1.0), dict(smoothness_penalty_small=0, smoothness_penalty_large=1),
               dict(smoothness_penalty_small=3000, smoothness_penalty_large=12000), dict(consistency_threshold=0),
               dict(disparity_factor=16), dict(disparity_factor=2048, number_of_disparities=32)):
        stereo.sgm_validate_params(30, 96, **dict(dict(number_of_disparities=32), **kw))
    stereo.sgm_validate_params(3, 64, number_of_disparities=64, window_radius=2)      # cols = D, rows = windowRadius + 1
    if torch.cuda.is_available():
        return
    with pytest.raises(stereo.StereoError, match="no HIP device") as ei:
        stereo.StereoSGM(376, 1241)
    assert ei.value.status == -3                       # PBA_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from sgm_probe import SgmHostProbe
    return SgmHostProbe(tmp_path_factory.mktemp("sgm_probe"))


def test_host_sgm_config(probe, tmp_path):
    cfg, selected = probe.parse("StereoAlgorithm = SGM\n", tmp_path)
    assert selected and cfg == sgm_util.DEFAULTS
    for alg, want in (("sgm", True), ("SemiGlobalMatching", True), ("SEMIGLOBALMATCHING", True), ("BlockMatching", False),
                      ("SGBM", False), ("RSGM", False)):
        assert probe.parse("StereoAlgorithm = %s\n" % alg, tmp_path)[1] is want
    assert probe.parse("numberOfDisparities = 64\n", tmp_path)[1] is False              # the key's default is BlockMatching
    text = ("StereoAlgorithm = SemiGlobalMatching\nnumberOfDisparities = 64\nsobelCapValue = 31\ncensusRadius = 1\nwindowRadius = 4\n"
            "smoothnessPenaltySmall = 50\nsmoothnessPenaltyLarge = 900\nconsistencyThreshold = 2\ndisparityFactor = 16\n"
            "censusWeightFactor = 0.25\n")
    cfg, selected = probe.parse(text, tmp_path)
    assert selected and cfg == dict(numberOfDisparities=64, sobelCapValue=31, censusRadius=1, windowRadius=4, smoothnessPenaltySmall=50,
                                    smoothnessPenaltyLarge=900, consistencyThreshold=2, disparityFactor=16.0, censusWeightFactor=0.25)
    for text, msg in [("numberOfDisparities = 100\n", "numberOfDisparities"), ("numberOfDisparities = 0\n", "numberOfDisparities"),
                      ("censusRadius = 3\n", "censusRadius"), ("windowRadius = 10\n", "windowRadius"), ("windowRadius = -1\n", "windowRadius"),
                      ("smoothnessPenaltySmall = -1\n", "smoothnessPenaltySmall"),
                      ("smoothnessPenaltySmall = 1600\n", "smoothnessPenaltyLarge"), ("smoothnessPenaltyLarge = 40000\n", "smoothnessPenaltyLarge"),
                      ("consistencyThreshold = -1\n", "consistencyThreshold"), ("disparityFactor = 0.5\n", "disparityFactor"),
                      ("disparityFactor = 1024\n", "disparityFactor"), ("censusWeightFactor = -1\n", "censusWeightFactor")]:
        with pytest.raises(RuntimeError, match=msg):
            probe.parse("StereoAlgorithm = SGM\n" + text, tmp_path)
    probe.release()
