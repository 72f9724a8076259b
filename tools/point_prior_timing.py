"""Wall time per LM iteration of one window without a point prior (default driver; host-stepped driver, PBA_ASYNC=0) and with one (the wide
chain on the host-stepped driver), and the wall time of one pba_linearize cost read-back with and without the prior (the
difference is one k_point_prior_cost launch, its copy and its synchronisation), measured in the same process
-> profiles/point_prior/timing.json.  Recorded, not gated.

usage: python tools/point_prior_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  kitti: the operating point of kitti_stereo.cfg
(5 frames, 5 000 points, 3 x 3, Huber 0.05).  Slot 0 is constant.  The prior: rank-1 depth factors along the optical axis of each point's
first camera, sigma_z = z^2 / (0.54 fx) (one pixel of disparity at KITTI's baseline), x0 = the start.  Per shape: one warm-up, then R
repeats of pba_solve with N_IT forced iterations (all tolerances 0).  Medians with the spread (min, max).  Synthetic windows: the ratio on
real imagery is unmeasured."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from photobundle_amd import se3, synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20
BASELINE = 0.54


def make(shape):
    if shape == "configs1":
        return synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    return synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI)


def depth_prior(p):
    first = np.searchsorted(np.asarray(p.obs_point), np.arange(p.n_points))
    slot = np.asarray(p.obs_slot)[first]
    L6 = np.zeros((p.n_points, 6))
    for s in np.unique(slot):
        R, t = se3.angle_axis_to_matrix(p.cams[s][:3]), p.cams[s][3:6]
        m = slot == s
        z = (p.xyz[m] @ R.T + t)[:, 2]
        n = R.T @ np.array([0.0, 0.0, 1.0])
        w = (BASELINE * p.K[0] / (z * z)) ** 2
        L6[m] = w[:, None] * np.array([n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2]])[None, :]
    return np.ascontiguousarray(p.xyz, np.float64), L6


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


def load(e, p, prior=None):
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(p.cams, constant_slots=(0,))
    if prior is not None:
        e.set_point_prior(*prior)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def run(p, reps):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    prior = depth_prior(p)
    t = dict(default=[], host_stepped=[], with_prior=[], cost=[], cost_with_prior=[])
    drivers, its = {}, {}
    with engine(p) as e, engine(p, async_on=False) as h:
        for rep in range(reps + 1):      # (rep 0 warms everything up)
            row = {}
            for key, eng, pr in (("default", e, None), ("host_stepped", h, None), ("with_prior", e, prior)):
                load(eng, p, pr)
                dt, r = timed(lambda: eng.solve(opt, fetch_state=False))
                row[key] = dt / max(1, len(r["iterations"]) - 1)
                drivers[key], its[key] = eng.solve_driver(), len(r["iterations"]) - 1
            for key, pr in (("cost", None), ("cost_with_prior", prior)):
                load(e, p, pr)
                e.linearize()
                row[key] = min(timed(e.linearize)[0] for _ in range(5))       # (the Jacobian pass is done: the read-back alone)
            if rep:
                for k, v in row.items():
                    t[k].append(v)
    out = {k: stats(v, 1e3) for k, v in t.items()}
    out["unit"] = "ms (LM: per iteration)"
    out["drivers"], out["iterations"] = drivers, its
    out["ratio_with_prior_to_host_stepped"] = out["with_prior"]["median"] / out["host_stepped"]["median"]
    out["ratio_with_prior_to_default"] = out["with_prior"]["median"] / out["default"]["median"]
    out["prior_cost_launch_ms"] = out["cost_with_prior"]["median"] - out["cost"]["median"]
    out["window"] = dict(n_frames=p.n_frames, n_points=p.n_points, n_obs=p.n_obs, radius=p.radius, huber=p.huber)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_prior", "timing.json"))
    a = ap.parse_args()
    res = {}
    for shape in a.shapes.split(","):
        res[shape] = run(make(shape), a.reps)
        print(shape, json.dumps(res[shape]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
