"""Wall time of one applied pba_admit next to the host route to the same engine state and to one LM iteration of the same window, measured
in the same process -> profiles/admit/timing.json.

usage: python tools/admit_timing.py [--reps R] [--shapes configs1,kitti] [--out FILE] [--kernels-only]
configs1: bench.py configs[1] (8 frames, 50 000 points, 5 x 5 patches, 376 x 1241).  kitti: the operating point of kitti_stereo.cfg
(5 frames, 5 000 points, 3 x 3, Huber 0.05).  Both windows are dense and lose the blocks with (point + slot) % 3 == 0, as the window with
holes of tests/admit_cases.py does.  The window is solved for N_IT iterations once; every repeat starts from that state, re-loaded and
linearised (an admission then finds its Jacobian pass done, as after a solve).  Per shape: one warm-up, then R repeats of
  device   Engine.admit(apply=True) at the class defaults: wall time of the call (it ends in a stream synchronise);
  host     the six steps the library offered before the call existed, to the same state: pba_get_state, the candidates in numpy
           (tests/admit_cases.reference_candidates), pba_set_problem with the candidate list (the points that have one, and their
           descriptors), pba_linearize, pba_get_block_costs, the rule in numpy and pba_set_problem with the merged lists -- wall time of
           the parts; the costs of the problem's own blocks, which the rule needs, come from a pba_get_block_costs that is timed with them;
  LM       pba_solve of that window with N_IT forced iterations (all tolerances 0) on the default driver: wall time per iteration.
Medians with the spread (min, max).  same_state: the two routes end in engines whose pba_linearize costs agree bit for bit, with the same
candidates and the same verdict.
--kernels-only: one warm-up and three applied admissions per shape and nothing else, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/admit_timing.py --kernels-only --shapes configs1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import admit_cases  # noqa: E402
from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
N_IT = 20
RULE = admit_cases.DEFAULTS
MIN_DEPTH = 0.1


def make(shape):
    if shape == "configs1":
        p = synthetic.make_window(n_frames=8, n_points=50000, radius=2, **KITTI)
    else:
        p = synthetic.make_window(n_frames=5, n_points=5000, radius=1, huber=0.05, **KITTI)
    return admit_cases.with_holes(p)


def stats(v, scale):
    v = sorted(v)
    return dict(median=scale * v[len(v) // 2], min=scale * v[0], max=scale * v[-1], repeats=len(v))


PARTS = ("get_state", "numpy_candidates", "set_problem_candidates", "linearize", "get_block_costs", "numpy_rule_and_merge", "set_problem_merged")


def run(p, reps, kernels_only):
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    dev, host, parts, lm = [], [], {k: [] for k in PARTS}, []
    mask = (1 << p.n_frames) - 1
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
            cp, cs, cost, take, info = e.admit(min_depth=MIN_DEPTH, apply=True, **RULE)
            t1 = time.perf_counter()
            assert info["applied"] == 1
            if kernels_only:
                continue
            cost_dev = e.linearize()
            reload()
            t = [time.perf_counter()]
            hc, hx = e.get_state()
            t.append(time.perf_counter())
            hp, hs, _ = admit_cases.reference_candidates(p, hc, hx, mask, MIN_DEPTH, p.radius)
            has = np.zeros(p.n_points, bool)
            has[hp] = True
            renumber = np.cumsum(has) - 1
            t.append(time.perf_counter())
            c_own = e.block_costs()
            e.set_problem(hx[has], p.desc[has], renumber[hp].astype(np.int32), hs, p.weights)
            t.append(time.perf_counter())
            e.linearize()
            t.append(time.perf_counter())
            c_cand = e.block_costs()
            t.append(time.perf_counter())
            htake, _ = admit_cases.reference_admit(c_own, c_cand, **RULE)
            mp, ms = admit_cases.merged_lists(p.obs_point, p.obs_slot, hp, hs, htake)
            t.append(time.perf_counter())
            e.set_problem(hx, p.desc, mp, ms, p.weights)
            t.append(time.perf_counter())
            same = (same and e.linearize().hex() == cost_dev.hex() and hp.tobytes() == cp.tobytes() and hs.tobytes() == cs.tobytes() and
                    htake.tobytes() == take.tobytes())
            reload()
            t6 = time.perf_counter()
            r = e.solve(opt, fetch_state=False)
            t7 = time.perf_counter()
            driver = e.solve_driver()
            if rep:
                dev.append(t1 - t0)
                host.append(t[-1] - t[0])
                for k, a, b in zip(PARTS, t[:-1], t[1:]):
                    parts[k].append(b - a)
                lm.append((t7 - t6) / max(1, r["num_iterations"] - 1))
    if kernels_only:
        return dict(admissions=3, candidates=info["n_candidates"], admitted=info["n_admitted"])
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return dict(driver=driver, lm_iterations=N_IT, rule=RULE, min_depth=MIN_DEPTH, border=int(p.radius), candidates=info["n_candidates"],
                admitted=info["n_admitted"], threshold=info["threshold"], same_state=bool(same), device_admit_wall_us=stats(dev, 1e6),
                host_route_wall_us=stats(host, 1e6), host_route_parts_wall_us={k: stats(v, 1e6) for k, v in parts.items()},
                lm_wall_us_per_iteration=stats(lm, 1e6), host_over_device=med(host) / med(dev), device_admit_in_lm_iterations=med(dev) / med(lm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs1,kitti")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit", "timing.json"))
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
