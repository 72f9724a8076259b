"""Inputs and fixtures of the semi-global matcher's tests (numpy only).

make_pair(rows, cols, ndisp, seed) builds a stereo pair with a planted piecewise-constant disparity: a smoothed random
texture as the right image, the left image read from it at x - d.  Horizontal bands carry different disparities, and
one vertical strip (a tenth of the width) carries half the band's disparity so that occlusions (and with them the left-right check and small speckle
regions) occur.  After the random draw everything is integer arithmetic, so the bytes only depend on numpy's legacy
MT19937 stream and the sha256 of a pair can be asserted before anything is compared against it."""
import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sgm")

DEFAULTS = dict(numberOfDisparities=128, sobelCapValue=15, censusRadius=2, windowRadius=2, smoothnessPenaltySmall=100,
                smoothnessPenaltyLarge=1600, consistencyThreshold=1, disparityFactor=256.0, censusWeightFactor=1.0 / 6.0)

# snake_case field of pba_sgm_params for each key of the reference's config
FIELD_OF_KEY = dict(numberOfDisparities="number_of_disparities", sobelCapValue="sobel_cap_value", censusRadius="census_radius",
                    windowRadius="window_radius", smoothnessPenaltySmall="smoothness_penalty_small",
                    smoothnessPenaltyLarge="smoothness_penalty_large", consistencyThreshold="consistency_threshold",
                    disparityFactor="disparity_factor", censusWeightFactor="census_weight_factor")


def planted_disparity(rows, cols, ndisp):
    """int32 [rows, cols]: three bands at ndisp*{1/4, 1/2, 5/8} (at least 2), a strip of a tenth of the width at half of it."""
    band = np.array([max(2, ndisp // 4), max(2, ndisp // 2), max(2, (5 * ndisp) // 8)], np.int32)
    y = np.arange(rows)
    d_row = band[np.minimum((3 * y) // max(rows, 1), 2)]
    d = np.repeat(d_row[:, None], cols, axis=1)
    x = np.arange(cols)
    strip = (10 * x) // cols == 6
    d[:, strip] = d[:, strip] // 2
    return d.astype(np.int32)


def make_pair(rows, cols, ndisp, seed):
    """-> (left u8, right u8, planted disparity int32), each [rows, cols]."""
    rng = np.random.RandomState(int(seed))
    wide = cols + ndisp
    t = rng.randint(0, 256, size=(rows + 2, wide + 2)).astype(np.int64)
    # separable [1 2 1] / 4 twice (integer), then the contrast stretched back about the mean level
    h = t[:, :-2] + 2 * t[:, 1:-1] + t[:, 2:]
    v = h[:-2] + 2 * h[1:-1] + h[2:]                    # 16 x the smoothed value
    tex = np.clip((v - 16 * 128) * 3 // 16 + 128, 0, 255).astype(np.uint8)
    d = planted_disparity(rows, cols, ndisp)
    right = np.ascontiguousarray(tex[:, ndisp:ndisp + cols])
    xs = ndisp + np.arange(cols)[None, :] - d
    left = np.ascontiguousarray(np.take_along_axis(tex, xs, axis=1))
    return left, right, d


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def params_of(case):
    p = dict(DEFAULTS)
    p.update(case.get("params", {}))
    p["numberOfDisparities"] = case["ndisp"]
    return p


def snake_params(p):
    return {FIELD_OF_KEY[k]: v for k, v in p.items()}


def load_cases():
    with open(os.path.join(GOLDEN_DIR, "cases.json")) as f:
        return json.load(f)["cases"]


def case_pair(case):
    """Inputs of a golden case: from its .npz when it has one, else regenerated from the seed."""
    if case.get("file"):
        z = np.load(os.path.join(GOLDEN_DIR, case["file"]))
        return z["left"], z["right"]
    left, right, _ = make_pair(case["rows"], case["cols"], case["ndisp"], case["seed"])
    return left, right


def case_expected(case):
    """-> (uint16 map or None, dict row -> uint16 row) as committed for the case."""
    if case.get("file"):
        z = np.load(os.path.join(GOLDEN_DIR, case["file"]))
        return z["disp_scaled"], None
    z = np.load(os.path.join(GOLDEN_DIR, case["rows_file"]))
    return None, (z["row_index"], z["disp_rows"])


def float_map(disp_scaled, factor):
    """The reference's float output from its uint16 map: (float)(u16 / disparityFactor), the division in double."""
    return (disp_scaled.astype(np.float64) / float(factor)).astype(np.float32)


def disparity_to_depth(disparity, bf):
    d = np.asarray(disparity, np.float32)
    with np.errstate(divide="ignore"):
        z = np.float32(bf) * (np.float32(1.0) / d)
    return np.where(d > np.float32(0.01), z, np.float32(-0.1)).astype(np.float32)
