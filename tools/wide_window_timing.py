"""Wide-window timing: microseconds per LM iteration of the host-stepped wide path, split into the three profiling shares
(elimination = k_wide_point + k_wide_pairs + k_wide_assemble | reduction + solve = k_solve_wide | sampling = the Jacobian / cost
passes), at 17, 24 and 32 frames x 50k points, 5x5 patches, causal visibility (synthetic.make_window).

usage: python tools/wide_window_timing.py [--frames 17 24 32] [--points 50000] [--iters 10] [--out FILE.json]
The shares come from the engine's HIP-event counters (pba_set_profiling 1); the wall time per iteration is measured in a separate
solve with profiling off.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/wide_window_timing.py` for per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_frames, n_points, radius, iters):
    from photobundle_amd import synthetic
    from photobundle_amd.engine import Engine, default_solver_options
    p = synthetic.make_window(n_frames=n_frames, n_points=n_points, radius=radius, visibility="causal")
    _, _, rows, cols = p.planes.shape
    opts = default_solver_options(max_num_iterations=iters, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    with Engine(rows, cols, p.K, p.radius, n_frames, huber=p.huber) as e:
        e.load(p)
        e.solve(opts)                                 # warm-up: code objects, co-observation lists, buffers
        e.load(p)
        t0 = time.perf_counter()
        res = e.solve(opts, fetch_state=False)
        wall = time.perf_counter() - t0
        driver = e.solve_driver()
        n_it = len(res["iterations"]) - 1
        e.load(p)
        e.set_profiling(1)
        e.reset_counters()
        e.solve(opts, fetch_state=False)
        c = e.counters()
        e.set_profiling(0)
    per = 1e3 / max(1, n_it)
    return dict(frames=n_frames, free_cameras=n_frames - 1, points=n_points, obs=int(p.n_obs), radius=radius, visibility="causal",
                driver=driver, iterations=n_it, us_per_iteration=1e6 * wall / max(1, n_it),
                profiled_us_per_iteration=dict(elimination=c["schur_ms"] * per, solve=c["solve_ms"] * per,
                                               sampling=(c["linearize_ms"] + c["cost_ms"]) * per),
                launches=dict(elimination=c["schur_launches"], solve=c["solve_launches"],
                              sampling=c["linearize_launches"] + c["cost_launches"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[17, 24, 32])
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for f in a.frames:
        r = measure(f, a.points, a.radius, a.iters)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
