"""Wall time of one applied pba_cull next to the host route to the same engine state and to one LM iteration of the same window, measured
in the same process -> profiles/cull/timing.json.

usage: python tools/cull_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE] [--kernels-only]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  kitti: the operating point of kitti_stereo.cfg
(5 frames, 5 000 points, 3 x 3, Huber 0.05).  One frame of each window carries an occluder as in tests/cull_cases.py (unrelated texture over
the same share of the frame).  The window is solved for N_IT iterations once; every repeat starts from that state, re-loaded and linearised
(a cull then finds its Jacobian pass done, as after a solve).  Per shape: one warm-up, then R repeats of
  device   Engine.cull(apply=True) at the class defaults: wall time of the call (it ends in a stream synchronise);
  host     the route the library offered before the call existed, to the same state: pba_get_obs_records, the rule in numpy
           (tests/cull_cases.reference_cull), pba_set_problem with the surviving lists (the full mode: no mode call to repeat) -- wall time of
           the three parts; the xyz of the survivors come from a pba_get_state that is NOT timed (a caller has them from its read-back);
  LM       pba_solve of that window with N_IT forced iterations (all tolerances 0) on the default driver: wall time per iteration.
Medians with the spread (min, max).  same_state: the two routes end in engines whose pba_linearize costs agree bit for bit.
--kernels-only: one warm-up and three applied culls per shape and nothing else, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/cull_timing.py --kernels-only --shapes configs1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cull_cases  # noqa: E402
from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20
RULE = cull_cases.DEFAULTS


def make(shape):
    if shape == "configs1":
        p = synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    else:
        p = synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI)
    # the occluder of tests/cull_cases.py, scaled to this frame: rows 1/3 .. 11/12, columns 1/16 .. 15/16 of the second-to-last frame
    rows, cols = KITTI["size"]
    r0, r1, c0, c1 = rows // 3, rows * 11 // 12, cols // 16, cols * 15 // 16
    images = p.images.copy()
    images[p.n_frames - 2, r0:r1, c0:c1] = cull_cases.occluder_patch((r1 - r0, c1 - c0), (r0, c0))
    p.images = images
    return p


def stats(v, scale):
    v = sorted(v)
    return dict(median=scale * v[len(v) // 2], min=scale * v[0], max=scale * v[-1], repeats=len(v))


def run(p, reps, kernels_only):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    dev, host, parts, lm = [], [], dict(get_obs_records=[], numpy_rule=[], set_problem=[]), []
    with Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber) as e:
        for s in range(p.n_frames):
            e.set_frame(s, p.images[s])
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(p.cams, p.fixed_slot)
        e.solve(opt, fetch_state=False)
        cams, xyz = e.get_state()

        def reload():
            e.set_problem(xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
            e.set_cameras(cams, p.fixed_slot)
            e.linearize()

        info = driver = None
        same = True
        for rep in range((3 if kernels_only else reps) + 1):      # (rep 0 warms everything up)
            reload()
            t0 = time.perf_counter()
            keep, pmap, info = e.cull(apply=True, **RULE)
            t1 = time.perf_counter()
            assert info["applied"] == 1
            if kernels_only:
                continue
            cost_dev = e.linearize()
            reload()
            x = e.get_state()[1]
            t2 = time.perf_counter()
            rec = e.obs_records()
            t3 = time.perf_counter()
            hkeep, hmap, _ = cull_cases.reference_cull(rec[:, 5], p.obs_point, **RULE)
            obs_point, obs_slot = cull_cases.surviving_lists(p.obs_point, p.obs_slot, hkeep, hmap)
            sx, sdesc = x[hmap >= 0], p.desc[hmap >= 0]
            t4 = time.perf_counter()
            e.set_problem(sx, sdesc, obs_point, obs_slot, p.weights)
            t5 = time.perf_counter()
            same = same and e.linearize().hex() == cost_dev.hex() and hkeep.tobytes() == keep.tobytes()
            reload()
            t6 = time.perf_counter()
            r = e.solve(opt, fetch_state=False)
            t7 = time.perf_counter()
            driver = e.solve_driver()
            if rep:
                dev.append(t1 - t0)
                host.append(t5 - t2)
                for k, v in zip(("get_obs_records", "numpy_rule", "set_problem"), (t3 - t2, t4 - t3, t5 - t4)):
                    parts[k].append(v)
                lm.append((t7 - t6) / max(1, r["num_iterations"] - 1))
    if kernels_only:
        return dict(culls=3, blocks_removed=info["n_blocks_before"] - info["n_blocks_after"])
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return dict(driver=driver, lm_iterations=N_IT, rule=RULE, blocks_removed=info["n_blocks_before"] - info["n_blocks_after"],
                points_removed=info["n_points_before"] - info["n_points_after"], threshold=info["threshold"], same_state=bool(same),
                device_cull_wall_us=stats(dev, 1e6), host_route_wall_us=stats(host, 1e6), host_route_parts_wall_us={k: stats(v, 1e6) for k, v in parts.items()},
                lm_wall_us_per_iteration=stats(lm, 1e6), host_over_device=med(host) / med(dev), device_cull_in_lm_iterations=med(dev) / med(lm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull", "timing.json"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        # rocprofv3 crashes in its exit handlers once a process has made a cooperative launch (pba_create's comment; its output files are
        # complete by then): the solve that only brings the window to its state runs on the three-kernel driver under the profiler
        os.environ["PBA_RESIDENT"] = "0"
    if a.reps < 5:
        ap.error("--reps: the median is taken over at least 5 repeats")
    out = {"reps": a.reps, "rows": []}
    for name in a.shapes.split(","):
        p = make(name)
        row = dict(shape=name, residual_blocks=int(p.n_obs), points=int(p.n_points), **run(p, a.reps, a.kernels_only))
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.kernels_only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
