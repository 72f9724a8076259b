"""Timing of the stereo block matcher (include/pba_stereo.h) on one KITTI-size rendered pair at the reference cfg settings
(376 x 1241, 128 disparities, 9 x 9 window, cap 31, texture 10, uniqueness 15).

Writes profiles/stereo/timing.json:
  * device time per pair from the handle's events (pba_stereo_get_timing): prefilter + matcher kernels, and upload .. last
    copy-back, with the disparity only and with the fused depth copied back as well; after warm-up, median / min / max of repeats;
  * host wall time of pba_stereo_compute (includes the pinned staging memcpy of the pair and of the outputs);
  * the CPU numpy restatement's time (tests/stereo_bm_ref.py) -- context only, it is not the reference's OpenCV path.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/stereo_timing.py --profile`
(--profile: fewer repeats, no CPU timing, no JSON).  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.stereo import StereoBM  # noqa: E402

CFG = dict(number_of_disparities=128, sad_window_size=9, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15)
BASELINE = 0.5372


def _pair():
    T = np.eye(4)
    tex = synthetic.Texture()
    left, _ = synthetic.render_frame(T, synthetic.KITTI_K, synthetic.KITTI_SIZE, tex)
    T_r = T.copy()
    T_r[:3, 3] += T[:3, 0] * BASELINE
    right, _ = synthetic.render_frame(T_r, synthetic.KITTI_K, synthetic.KITTI_SIZE, tex)
    return left, right


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo", "timing.json"))
    a = ap.parse_args()
    if a.profile:
        a.warmup, a.repeats = 5, 50
    left, right = _pair()
    bf = float(np.float32(BASELINE * synthetic.KITTI_K[0]))
    rows, cols = left.shape
    res = dict(shape=[rows, cols], params=CFG, warmup=a.warmup, repeats=a.repeats)
    with StereoBM(rows, cols, **CFG) as s:
        for label, want_depth in (("disparity_only", False), ("disparity_and_depth", True)):
            for _ in range(a.warmup):
                s.compute(left, right, bf, depth=want_depth)
            kern, total, wall = [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                s.compute(left, right, bf, depth=want_depth)
                wall.append((time.perf_counter() - t0) * 1e3)
                k, t = s.timing()
                kern.append(k)
                total.append(t)
            res[label] = dict(kernels_ms=_stats(kern), device_total_ms=_stats(total), host_wall_ms=_stats(wall))
            print("%-20s kernels %.4f ms (min %.4f)  upload..copy-back %.4f ms  host wall %.4f ms (medians)" % (
                label, res[label]["kernels_ms"]["median"], res[label]["kernels_ms"]["min"],
                res[label]["device_total_ms"]["median"], res[label]["host_wall_ms"]["median"]))
        d, _ = s.compute(left, right, bf, depth=False)
    if a.profile:
        return
    import stereo_bm_ref as ref
    t0 = time.perf_counter()
    want = ref.bm(left, right, ref.default_params(**CFG))
    res["cpu_numpy_restatement_s"] = time.perf_counter() - t0
    res["cpu_numpy_restatement_note"] = "tests/stereo_bm_ref.py vectorised numpy, one process: context, not the reference (OpenCV)"
    res["device_equals_restatement"] = bool(np.array_equal(d, want))
    res["filtered_fraction"] = float((d == -16).mean())
    print("numpy restatement %.2f s; device output identical: %s" % (res["cpu_numpy_restatement_s"], res["device_equals_restatement"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
