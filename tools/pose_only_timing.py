"""Pose-only iteration against the full iteration on the same device (pba_set_points_constant)
-> profiles/pose_only/timing.json, and with --rocprof a `rocprofv3 --kernel-trace --stats` CSV of one pose-only run next to it.

usage: python tools/pose_only_timing.py [--reps R] [--shapes configs1,tracking] [--out FILE] [--rocprof DIR]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  tracking: ONE free camera x 4 096 points x 3 x 3 -- the
last frame of a 5-frame window against the window's points (the other cameras keep no residual block).  Every solve runs exactly
N_IT LM iterations (tolerances 0).  Per shape: the full problem on its default driver and on the host-stepped driver with event
profiling (kernel times), then the pose-only problem the same two ways (it has the host-stepped driver only)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 10


def make(shape):
    if shape == "configs1":
        return synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    p = synthetic.make_window(n_frames=5, n_points=4096, radius=1, huber=0.05, **KITTI)
    keep = p.obs_slot == p.n_frames - 1
    p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
    assert len(np.unique(p.obs_point)) == p.n_points
    return p


def run(p, pose, profile, reps):
    """Median wall time per iteration [us] and, with event profiling, the kernel times per launch [us]."""
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    walls, ctr, driver, n_it = [], None, None, None
    with Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber) as e:
        for rep in range(reps + 1):
            e.load(p)
            if pose:
                e.set_points_constant()
            if profile:
                e.reset_counters()
            t0 = time.perf_counter()
            r = e.solve(opt, fetch_state=False)
            t1 = time.perf_counter()
            n_it = r["num_iterations"] - 1
            driver = e.solve_driver()
            if rep:
                walls.append((t1 - t0) / max(1, n_it))
                if profile:
                    ctr = e.counters()
    walls.sort()
    row = dict(pose_only=bool(pose), event_profiling=bool(profile), driver=driver, iterations=n_it, wall_us_per_iteration=1e6 * walls[len(walls) // 2])
    if ctr:
        def per(ms, n):
            return 1e3 * ms / n if n else 0.0
        row.update(jacobian_pass_us=per(ctr["linearize_ms"], ctr["linearize_launches"]), cost_pass_us=per(ctr["cost_ms"], ctr["cost_launches"]),
                   system_us=per(ctr["schur_ms"], ctr["schur_launches"]), solve_us=per(ctr["solve_ms"], ctr["solve_launches"]),
                   launches=dict(jacobian=ctr["linearize_launches"], cost=ctr["cost_launches"], system=ctr["schur_launches"], solve=ctr["solve_launches"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,tracking")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_only", "timing.json"))
    ap.add_argument("--rocprof", default=None, help="directory for a rocprofv3 --kernel-trace --stats run of the pose-only solves (a fresh child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        for name in a.shapes.split(","):
            run(make(name), True, False, 2)
        return
    out = {"iterations": N_IT, "reps": a.reps, "rows": []}
    for name in a.shapes.split(","):
        p = make(name)
        for pose in (False, True):
            for profile in (False, True):
                row = dict(shape=name, residual_blocks=int(p.n_obs), **run(p, pose, profile, a.reps))
                out["rows"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "pose_only", "--",
                               sys.executable, os.path.abspath(__file__), "--child", "--shapes", a.shapes], timeout=540)


if __name__ == "__main__":
    main()
