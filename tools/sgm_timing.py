"""Timing of the semi-global matcher (include/pba_sgm.h) on the full-size golden pair (376 x 1241, 128 disparities, the
reference's default parameters; tests/golden/sgm/cases.json, inputs regenerated from the seed).

Writes profiles/sgm/timing.json:
  * device time per pair from the handle's events (pba_sgm_get_timing): first kernel .. last kernel, and upload .. last copy-back,
    with the depth only (what run_kitti asks for) and with all three outputs copied back; after warm-up, median / min / max;
  * host wall time of pba_sgm_compute (includes the pinned staging memcpy of the pair and of the outputs);
  * the wall time of the CPU numpy restatement (tests/sgm_ref.py) on this host -- context only, it is not the reference's SSE code.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/sgm_timing.py --profile`
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

import sgm_util  # noqa: E402
from photobundle_amd.stereo import StereoSGM  # noqa: E402

BF = 386.1726


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm", "timing.json"))
    a = ap.parse_args()
    if a.profile:
        a.warmup, a.repeats = 5, 50
    case = [c for c in sgm_util.load_cases() if c["name"] == "main_376x1241"][0]
    left, right = sgm_util.case_pair(case)
    rows, cols = left.shape
    res = dict(shape=[rows, cols], params=sgm_util.params_of(case), warmup=a.warmup, repeats=a.repeats)
    with StereoSGM(rows, cols) as s:
        for label, ask in (("depth_only", (False, False, True)), ("all_outputs", (True, True, True))):
            for _ in range(a.warmup):
                s.compute_all(left, right, BF, *ask)
            kern, total, wall = [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                s.compute_all(left, right, BF, *ask)
                wall.append((time.perf_counter() - t0) * 1e3)
                k, t = s.timing()
                kern.append(k)
                total.append(t)
            res[label] = dict(kernels_ms=_stats(kern), device_total_ms=_stats(total), host_wall_ms=_stats(wall))
            print("%-12s kernels %.4f ms (min %.4f)  upload..copy-back %.4f ms  host wall %.4f ms (medians)" % (
                label, res[label]["kernels_ms"]["median"], res[label]["kernels_ms"]["min"],
                res[label]["device_total_ms"]["median"], res[label]["host_wall_ms"]["median"]))
        u, d, _ = s.compute_all(left, right, BF)
    if a.profile:
        return
    res["device_equals_reference_fixture"] = bool(sgm_util.sha256(u) == case["disp_scaled_sha256"] and
                                                  sgm_util.sha256(d) == case["disparity_sha256"])
    import sgm_ref
    p = sgm_util.params_of(case)
    t0 = time.perf_counter()
    want = sgm_ref.compute(left, right, p.pop("numberOfDisparities"), **p)
    res["cpu_numpy_restatement_s"] = time.perf_counter() - t0
    res["cpu_numpy_restatement_note"] = "tests/sgm_ref.py vectorised numpy, one process: context, not the reference's SSE code"
    res["device_equals_restatement"] = bool(np.array_equal(u, want["disp_scaled"]))
    res["nonzero_share"] = float((u != 0).mean())
    print("numpy restatement %.2f s; device output identical to it: %s, to the reference's fixture: %s" % (
        res["cpu_numpy_restatement_s"], res["device_equals_restatement"], res["device_equals_reference_fixture"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
