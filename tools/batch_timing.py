"""Batched against back-to-back solo solves (pba_solve_batch) -> profiles/batch/timing.json.

usage: python tools/batch_timing.py [--reps R] [--shapes small,configs1]
Every window runs exactly 20 LM iterations (tolerances 0, max_num_iterations = 20).  small: the reference's operating point
(376 x 1241, 5 frames, 3 x 3 patches, 5 000 points = 25 k residual blocks) at n = 1, 2, 4, 8, 16; configs1: bench.py configs[1]
(8 frames, 50 k points, 5 x 5) at n = 1, 2, 4.  Solo = pba_solve on each engine in turn (the default driver)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from photobundle_amd import synthetic  # noqa: E402
from photobundle_amd.engine import Engine, default_solver_options, solve_batch  # noqa: E402

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
SHAPES = {"small": (dict(n_frames=5, n_points=5000, radius=1, **KITTI), (1, 2, 4, 8, 16)),
          "configs1": (dict(n_frames=8, n_points=50000, radius=2, **KITTI), (1, 2, 4))}
N_IT = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="small,configs1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "timing.json"))
    a = ap.parse_args()
    opt = default_solver_options(max_num_iterations=N_IT, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    out = {"iterations": N_IT, "reps": a.reps, "rows": []}
    for name in a.shapes.split(","):
        wkw, ns = SHAPES[name]
        probs = [synthetic.make_window(seed_offset=k, **wkw) for k in range(max(ns))]
        engines = [Engine(wkw["size"][0], wkw["size"][1], p.K, p.radius, p.n_frames, huber=p.huber).load(p) for p in probs]
        try:
            for n in ns:
                es, ps = engines[:n], probs[:n]
                solo, batch = [], []
                for rep in range(a.reps + 1):
                    for e, p in zip(es, ps):
                        e.load(p)
                    t0 = time.perf_counter()
                    for e in es:
                        r = e.solve(opt, fetch_state=False)
                        assert r["num_iterations"] == N_IT + 1, r["message"]
                    t1 = time.perf_counter()
                    driver = es[0].solve_driver()
                    for e, p in zip(es, ps):
                        e.load(p)
                    t2 = time.perf_counter()
                    res = solve_batch(es, opt, fetch_state=False)
                    t3 = time.perf_counter()
                    assert all(r["num_iterations"] == N_IT + 1 for r in res)
                    if rep:                       # the first round warms up
                        solo.append(t1 - t0)
                        batch.append(t3 - t2)
                solo.sort(); batch.sort()
                row = dict(shape=name, n=n, blocks_per_window=int(es[0].n_obs), solo_driver=driver,
                           solo_ms=1e3 * solo[len(solo) // 2], batch_ms=1e3 * batch[len(batch) // 2],
                           batch_us_per_iteration=1e6 * batch[len(batch) // 2] / N_IT)
                row["speedup"] = row["solo_ms"] / row["batch_ms"]
                out["rows"].append(row)
                print(json.dumps(row), flush=True)
        finally:
            for e in engines:
                e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
