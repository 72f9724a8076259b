"""Structure-only iteration against the full iteration on the same driver (pba_set_cameras_constant)
-> profiles/points_only/timing.json, and with --rocprof a `rocprofv3 --kernel-trace --stats` CSV of the mode's solves next to it.

usage: PBA_ASYNC=0 python tools/points_only_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE] [--rocprof DIR]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  kitti: the operating point of kitti_stereo.cfg
(5 frames, 5 000 points, 3 x 3).  Both solves run through pba_solve on the host-stepped driver (PBA_ASYNC=0, set by this tool when
absent), N_IT forced LM iterations (all tolerances 0), one warm-up solve each, then R alternations full / mode, each solve
synchronised by pba_solve itself.  Reported per shape and mode: the median of the R repeats and their spread (min, max), in
microseconds per iteration; the cameras of the mode's windows sit at the ground truth, the full solve runs the window as made."""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PBA_ASYNC", "0")

import numpy as np  # noqa: E402

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20


def make(shape):
    if shape == "configs1":
        return synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    return synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI)


def solve_once(e, p, mode, opt):
    cams = np.array(p.meta["cams_gt"], np.float64) if mode else p.cams
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(cams, p.fixed_slot)
    if mode:
        e.set_cameras_constant()
    t0 = time.perf_counter()
    r = e.solve(opt, fetch_state=False)
    t1 = time.perf_counter()
    return (t1 - t0) / max(1, r["num_iterations"] - 1), r["num_iterations"] - 1, e.solve_driver()


def run(p, reps):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    walls, info = {False: [], True: []}, {}
    with Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber) as e:
        e.load(p)
        for rep in range(reps + 1):      # (rep 0 warms both up)
            for mode in (False, True):
                w, n_it, driver = solve_once(e, p, mode, opt)
                info[mode] = (n_it, driver)
                if rep:
                    walls[mode].append(w)
    rows = []
    for mode in (False, True):
        w = sorted(walls[mode])
        rows.append(dict(cameras_constant=mode, driver=info[mode][1], iterations=info[mode][0], wall_us_per_iteration=1e6 * w[len(w) // 2],
                         min_us=1e6 * w[0], max_us=1e6 * w[-1], repeats=len(w)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_only", "timing.json"))
    ap.add_argument("--rocprof", default=None, help="directory for a rocprofv3 --kernel-trace --stats run of the mode's solves (a fresh child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5 and not a.child:
        ap.error("--reps: the median is taken over at least 5 alternations")
    if a.child:
        opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
        for name in a.shapes.split(","):
            p = make(name)
            with Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber) as e:
                e.load(p)
                for _ in range(2):
                    solve_once(e, p, True, opt)
        return
    out = {"iterations": N_IT, "reps": a.reps, "PBA_ASYNC": os.environ["PBA_ASYNC"], "rows": []}
    for name in a.shapes.split(","):
        p = make(name)
        for row in run(p, a.reps):
            row = dict(shape=name, residual_blocks=int(p.n_obs), points=int(p.n_points), **row)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        # the child runs in a session of its own: when the time limit strikes the whole process group goes, rocprofv3 AND the python below it
        child = subprocess.Popen(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "points_only", "--",
                                  sys.executable, os.path.abspath(__file__), "--child", "--shapes", a.shapes],
                                 start_new_session=True)
        try:
            rc = child.wait(timeout=540)
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)
            child.wait()
            raise
        if rc:
            raise subprocess.CalledProcessError(rc, "rocprofv3")


if __name__ == "__main__":
    main()
