"""Recorder of solve bits: the exact results of a fixed list of small solves with the library named by PBA_LIB (default: the built one).

    python tools/ab_bits.py                         prints one line per case
    python tools/ab_bits.py --out bits.json --commit <hash of the commit the library was built from>

Run it once per library and diff the outputs; the --out of one run is the form of a test fixture (a test calls record() on the built
library and compares field by field).  Per case: the driver that ran it, the iteration costs as hex floats, the
termination type, and the SHA-1 of the cameras, of the points and of the observation records.

The cases (all small, seconds each) aim at the code shared by the solo and the batched launches:
  rs_*   reduce + solve in its narrow form (4 frames x 300 points: 3 free cameras, four solve waves) and its eight-wave form (12 frames
         x 600 points: 11 free cameras), each three ways: the iteration limit hit (the fused final decision and flush run),
         max_num_iterations = 0, and a loose function tolerance that terminates early (the final pass only flushes)
  mc*    the multi-channel sampler: C = 3 (IntensityAndGradient) and C = 8 (BitPlanes), R = 1 and R = 2, unit and Gaussian weights, on
         a 120 x 160 image (border observations occur)
  batch  two windows through pba_solve_batch: single-channel, C = 3 and C = 8
Every case runs under every environment of ENVS (the default driver, PBA_RESIDENT=0, the host-stepped driver, PBA_FUSE=0; the batches
under the first two, which have the pipeline pba_solve_batch needs), one child process per environment, one after another (the
driver is chosen at pba_create)."""
import argparse
import copy
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENVS = {"default": {}, "pipelined": {"PBA_RESIDENT": "0"}, "host-stepped": {"PBA_ASYNC": "0"}, "unfused": {"PBA_FUSE": "0"}}
BATCH_ENVS = ("default", "pipelined")      # pba_solve_batch needs the asynchronous fused pipeline
DRIVER_VARS = ("PBA_RESIDENT", "PBA_ASYNC", "PBA_FUSE", "PBA_FUSE_FINAL")

SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
WINDOWS = {
    "narrow": dict(n_frames=4, n_points=300, radius=2, **SMALL),
    "wide8": dict(n_frames=12, n_points=600, radius=2, size=(188, 621), K=(359.4, 359.4, 303.6, 92.6)),
}
SOLVES = {"limit": dict(max_num_iterations=3), "zero": dict(max_num_iterations=0), "ftol": dict(function_tolerance=1e-2)}
DESCRIPTORS = {"mc3": "IntensityAndGradient", "mc8": "BitPlanes"}
MC_SOLVE = dict(max_num_iterations=4)


def case_names(env):
    names = ["rs_%s_%s" % (w, s) for w in WINDOWS for s in SOLVES]
    names += ["%s_r%d_%s" % (d, r, w) for d in DESCRIPTORS for r in (1, 2) for w in ("unit", "gauss")]
    if env in BATCH_ENVS:
        names += ["batch_%s/%d" % (b, k) for b in ("rs", "mc3", "mc8") for k in (0, 1)]
    return names


def _engine(p):
    from photobundle_amd.engine import Engine
    rows, cols = p.images.shape[1:]
    return Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, channels=p.channels or 1).load(p)


def _record(r, e):
    sha = lambda a: hashlib.sha1(a.tobytes()).hexdigest()
    return dict(driver=e.solve_driver(), costs=[i["cost"].hex() for i in r["iterations"]], termination_type=r["termination_type"],
                cams=sha(r["cams"]), xyz=sha(r["xyz"]), rec=sha(e.obs_records()))


def child(with_batches):
    """Every case in this process's environment: {case name: record}."""
    from photobundle_amd import imgproc, synthetic
    from photobundle_amd.engine import default_solver_options, solve_batch
    out = {}
    win = {w: synthetic.make_window(**kw) for w, kw in WINDOWS.items()}
    for w, p in win.items():
        for s, skw in SOLVES.items():
            with _engine(p) as e:
                out["rs_%s_%s" % (w, s)] = _record(e.solve(default_solver_options(**skw)), e)
    mc = {}
    for d, kind in DESCRIPTORS.items():
        for r in (1, 2):
            p = synthetic.make_window(n_frames=4, n_points=300, radius=r, channel_fn=synthetic.channel_fn(kind), **SMALL)
            for wname, gaussian in (("unit", False), ("gauss", True)):
                q = copy.copy(p)
                q.weights = imgproc.make_patch_weights(r, gaussian)
                mc[(d, r, wname)] = q
                with _engine(q) as e:
                    out["%s_r%d_%s" % (d, r, wname)] = _record(e.solve(default_solver_options(**MC_SOLVE)), e)
    batches = {"batch_rs": [(win["narrow"], SOLVES["limit"]), (win["wide8"], SOLVES["ftol"])],
               "batch_mc3": [(mc[("mc3", 2, "unit")], SOLVES["limit"]), (mc[("mc3", 2, "unit")], SOLVES["ftol"])],
               "batch_mc8": [(mc[("mc8", 2, "unit")], SOLVES["limit"]), (mc[("mc8", 2, "unit")], SOLVES["ftol"])]}
    for name, members in batches.items() if with_batches else ():
        engines = [_engine(p) for p, _ in members]
        try:
            res = solve_batch(engines, [default_solver_options(**skw) for _, skw in members])
            for k, (r, e) in enumerate(zip(res, engines)):
                out["%s/%d" % (name, k)] = _record(r, e)
        finally:
            for e in engines:
                e.close()
    return out


def record_env(name, cache_dir=None, lib=None):
    """{case: record} of one environment of ENVS, from a child process of its own.  lib: the library (None: the built one)."""
    env = {k: v for k, v in os.environ.items() if k not in DRIVER_VARS + ("PBA_LIB",)}
    env.update(ENVS[name])
    if lib:
        env["PBA_LIB"] = lib
    if cache_dir:
        env["PBA_WINDOW_CACHE"] = cache_dir
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "1" if name in BATCH_ENVS else "0"], capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise RuntimeError("ab_bits child %r failed (%d): %s" % (name, r.returncode, r.stderr[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])


def record(cache_dir=None, lib=None):
    """{environment: {case: record}}: one child process per environment, one after another."""
    return {name: record_env(name, cache_dir, lib) for name in ENVS}


def lines(cases):
    for env, recs in sorted(cases.items()):
        for name, c in sorted(recs.items()):
            yield "%-12s %-18s %-12s term %d  cams %s xyz %s rec %s  costs %s" % (
                env, name, c["driver"], c["termination_type"], c["cams"][:12], c["xyz"][:12], c["rec"][:12], " ".join(c["costs"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--child", choices=("0", "1"), help="run the cases (1: the batches too) in this process and print them as one JSON line")
    ap.add_argument("--out", help="write the result as JSON")
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (a field of --out)")
    ap.add_argument("--cache", default=None, help="directory for PBA_WINDOW_CACHE")
    a = ap.parse_args()
    if a.child:
        print("RESULT" + json.dumps(child(a.child == "1")))
        return
    cases = record(a.cache, os.environ.get("PBA_LIB"))
    for l in lines(cases):
        print(l)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(commit=a.commit, cases=cases), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
