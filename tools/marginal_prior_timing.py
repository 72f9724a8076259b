"""Wall time and per-kernel event time of one pba_marginalize next to one LM iteration of the same window, and the price of carrying the
prior (the host-stepped driver instead of the device-decided ones), measured in the same process
-> profiles/marginal_prior/timing.json.  Recorded, not gated.

usage: python tools/marginal_prior_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE] [--no-class]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  kitti: the operating point of kitti_stereo.cfg
(5 frames, 5 000 points, 3 x 3, Huber 0.05).  Slot 0 is constant and is the slot that is dropped.  Per shape: one warm-up, then R repeats of
  marginalize  pba_marginalize of the freshly loaded and linearised window: wall time of the call with the outputs copied to the host,
               profiling off; then once more with event profiling on (pba_set_profiling(e, 1)) for the event time of its kernels
               (-1: the kernel did not run -- k_prior runs only when a prior is set, and the second of two chained calls shows it);
  LM           pba_solve of that window with N_IT forced iterations (all tolerances 0): wall time per iteration on the default driver
               without a prior (what the window cost before this feature), on the host-stepped driver without a prior (PBA_ASYNC=0),
               and with the marginalised prior set (host-stepped, plus the prior's two launches per step).
class: run_kitti on a synthetic eight-frame 120 x 160 sequence (window 4, 3 x 3 patches, Huber 0.05) with marginalize = 0 and 1: the
"solve" and "read-back" phases optimize() reports per window (the marginalisation is in the read-back phase).
Medians with the spread (min, max)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20
KERNELS = ("k_marg_point", "k_elim_pair", "k_marg_grad", "k_prior", "k_marg_eliminate")
ANCHORS, DROP = (0,), (0,)


def make(shape):
    if shape == "configs1":
        return synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    return synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI)


def stats(v, scale):
    v = sorted(v)
    return dict(median=scale * v[len(v) // 2], min=scale * v[0], max=scale * v[-1], repeats=len(v))


def engine(p, async_on=True):
    old = os.environ.get("PBA_ASYNC")
    if not async_on:
        os.environ["PBA_ASYNC"] = "0"
    try:
        e = Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber)
    finally:
        os.environ.pop("PBA_ASYNC", None)
        if old is not None:
            os.environ["PBA_ASYNC"] = old
    for s in range(p.n_frames):
        e.set_frame(s, p.images[s])
    return e


def load(e, p):
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(p.cams, constant_slots=ANCHORS)


def run(p, reps):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    lm, lm_host, lm_prior, marg, kern, kern_chained = [], [], [], [], {k: [] for k in KERNELS}, {k: [] for k in KERNELS}
    drivers = {}
    with engine(p) as e, engine(p, async_on=False) as h:
        e._L.pba_internal_marginal_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        e._L.pba_internal_marginal_times.restype = None
        info = None
        for rep in range(reps + 1):      # (rep 0 warms everything up)
            load(e, p)
            e.linearize()                # (the call then finds its Jacobian pass done, as after a solve)
            t0 = time.perf_counter()
            info = e.marginalize(DROP)
            t1 = time.perf_counter()
            prior = {k: info[k] for k in ("slots", "x0", "Lambda", "eta", "c")}
            e.set_profiling(1)
            e.marginalize(DROP)
            ms = (C.c_double * 5)()
            e._L.pba_internal_marginal_times(e._h, ms)
            e.set_camera_prior(**prior)  # chained: the current prior is one more factor (k_prior)
            e.marginalize(DROP)
            ms2 = (C.c_double * 5)()
            e._L.pba_internal_marginal_times(e._h, ms2)
            e.set_profiling(0)
            load(e, p)
            t2 = time.perf_counter()
            r = e.solve(opt, fetch_state=False)
            t3 = time.perf_counter()
            drivers["default"] = e.solve_driver()
            load(e, p)
            e.set_camera_prior(**prior)
            t4 = time.perf_counter()
            rp = e.solve(opt, fetch_state=False)
            t5 = time.perf_counter()
            drivers["with_prior"] = e.solve_driver()
            load(h, p)
            t6 = time.perf_counter()
            rh = h.solve(opt, fetch_state=False)
            t7 = time.perf_counter()
            drivers["async_off"] = h.solve_driver()
            if rep:
                marg.append(t1 - t0)
                lm.append((t3 - t2) / max(1, r["num_iterations"] - 1))
                lm_prior.append((t5 - t4) / max(1, rp["num_iterations"] - 1))
                lm_host.append((t7 - t6) / max(1, rh["num_iterations"] - 1))
                for k, v, v2 in zip(KERNELS, ms, ms2):
                    kern[k].append(v)
                    kern_chained[k].append(v2)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return dict(free_cameras=p.n_frames - len(ANCHORS), anchors=list(ANCHORS), drop=list(DROP), kept_cameras=info["k"],
                marginalised_points=info["n_points"], marginalised_blocks=info["n_blocks"], min_point_pivot=info["min_point_pivot"],
                min_cam_pivot=info["min_cam_pivot"], drivers=drivers, lm_iterations=N_IT,
                marginalize_wall_us=stats(marg, 1e6), marginalize_kernel_event_us={k: stats(v, 1e3) for k, v in kern.items()},
                marginalize_chained_kernel_event_us={k: stats(v, 1e3) for k, v in kern_chained.items()},
                lm_wall_us_per_iteration=stats(lm, 1e6), lm_host_stepped_wall_us_per_iteration=stats(lm_host, 1e6),
                lm_with_prior_wall_us_per_iteration=stats(lm_prior, 1e6),
                marginalize_in_lm_iterations=med(marg) / med(lm), prior_iteration_over_default=med(lm_prior) / med(lm),
                prior_iteration_over_host_stepped=med(lm_prior) / med(lm_host))


def run_class(reps):
    """optimize() of the host class through run_kitti, marginalize = 0 and 1: its own phase report, per window."""
    import host_class_probe
    import numpy as np
    size, K, n = (120, 160), (200.0, 200.0, 80.0, 60.0), 8
    imgs, depths, _, local = host_class_probe.sequence(n, size, K)
    run_bin = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
    pat = re.compile(r"optimize phases ms: assemble ([\d.]+), set_problem ([\d.]+), set_cameras ([\d.]+), solve ([\d.]+), read-back ([\d.]+), evict ([\d.]+)")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        host_class_probe.write_sequence(d, imgs, [np.asarray(z, np.float32) for z in depths], K, local)
        for key in (0, 1):
            solve, back = [], []
            for rep in range(reps + 1):
                cfg = os.path.join(d, "t%d.cfg" % key)
                with open(cfg, "w") as f:
                    f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nmaxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\n"
                            "robustThreshold = 0.05\nverbose = 1\nmarginalize = %d\n" % (d, d, key))
                r = subprocess.run([run_bin, "-c", cfg, "-o", os.path.join(d, "o.txt")], capture_output=True, text=True, timeout=600, check=True)
                rows = [[float(v) for v in m.groups()] for m in pat.finditer(r.stderr)]
                if rep:      # (the first window of a process pays the runtime's set-up: windows 2.. of every run)
                    solve += [row[3] for row in rows[1:]]
                    back += [row[4] for row in rows[1:]]
            out["marginalize_%d" % key] = dict(windows=len(solve), solve_ms=stats(solve, 1.0), read_back_ms=stats(back, 1.0))
    out["solve_ratio"] = out["marginalize_1"]["solve_ms"]["median"] / out["marginalize_0"]["solve_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--no-class", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_prior", "timing.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: the median is taken over at least 5 repeats")
    out = {"reps": a.reps, "rows": []}
    for name in [s for s in a.shapes.split(",") if s]:
        p = make(name)
        row = dict(shape=name, residual_blocks=int(p.n_obs), points=int(p.n_points), **run(p, a.reps))
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_class:
        out["class"] = run_class(a.reps)
        print(json.dumps(out["class"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
