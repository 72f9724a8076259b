"""Wall time and per-kernel event time of one pba_covariance next to one LM iteration of the same window, measured in the same process
 -> profiles/covariance/timing.json.

usage: python tools/covariance_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241) with anchors {0, 7}.  kitti: the operating point of
kitti_stereo.cfg (5 frames, 5 000 points, 3 x 3, Huber 0.05) with anchors {0, 1}.  Per shape: one warm-up, then R repeats of
  covariance pba_covariance (cameras and points) of the freshly loaded and linearised window: wall time of the call with the outputs
             copied to the host, profiling off; then once more with event profiling on (pba_set_profiling(e, 1)) for the event time of
             its four kernels (-1: the kernel did not run);
  LM         pba_solve of that window with N_IT forced iterations (all tolerances 0) on the default driver: wall time per iteration.
Medians with the spread (min, max).  The covariance call runs once per solve, an LM iteration tens of times."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, EngineError, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20
KERNELS = ("k_cov_point", "k_elim_pair", "k_cov_invert", "k_cov_points")


def make(shape):
    if shape == "configs1":
        return synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI), (0, 7)
    return synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI), (0, 1)


def stats(v, scale):
    v = sorted(v)
    return dict(median=scale * v[len(v) // 2], min=scale * v[0], max=scale * v[-1], repeats=len(v))


def call(e):
    """(info fields, status text) of one pba_covariance; a singular window is timed like any other and reported as such."""
    try:
        return e.covariance(), "ok"
    except EngineError as err:
        if getattr(err, "status", 0) != -6:      # PBA_ERR_NUMERIC
            raise
        return err.info, str(err)


def run(p, slots, reps):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    lm, cov, kern = [], [], {k: [] for k in KERNELS}
    with Engine(KITTI["size"][0], KITTI["size"][1], p.K, p.radius, p.n_frames, huber=p.huber) as e:
        e._L.pba_internal_covariance_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        e._L.pba_internal_covariance_times.restype = None
        for s in range(p.n_frames):
            e.set_frame(s, p.images[s])
        info = driver = None
        for rep in range(reps + 1):      # (rep 0 warms everything up)
            e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
            e.set_cameras(p.cams, constant_slots=slots)
            e.linearize()                # (the covariance call then finds its Jacobian pass done, as after a solve)
            t2 = time.perf_counter()
            info, status = call(e)
            t3 = time.perf_counter()
            e.set_profiling(1)
            call(e)
            ms = (C.c_double * 4)()
            e._L.pba_internal_covariance_times(e._h, ms)
            e.set_profiling(0)
            t0 = time.perf_counter()
            r = e.solve(opt, fetch_state=False)
            t1 = time.perf_counter()
            driver = e.solve_driver()
            if rep:
                lm.append((t1 - t0) / max(1, r["num_iterations"] - 1))
                cov.append(t3 - t2)
                for k, v in zip(KERNELS, ms):
                    kern[k].append(v)
    return dict(free_cameras=p.n_frames - len(slots), anchors=list(slots), n_cam=info["n_cam"], driver=driver, lm_iterations=N_IT, covariance_status=status,
                min_cam_pivot=info["min_cam_pivot"], min_point_pivot=info["min_point_pivot"],
                lm_wall_us_per_iteration=stats(lm, 1e6), covariance_wall_us=stats(cov, 1e6),
                covariance_kernel_event_us={k: stats(v, 1e3) for k, v in kern.items()},
                covariance_in_lm_iterations=sorted(cov)[len(cov) // 2] / sorted(lm)[len(lm) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance", "timing.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: the median is taken over at least 5 repeats")
    out = {"reps": a.reps, "rows": []}
    for name in a.shapes.split(","):
        p, slots = make(name)
        row = dict(shape=name, residual_blocks=int(p.n_obs), points=int(p.n_points), **run(p, slots, a.reps))
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
