"""-m gpu: pba_solve_batch -- independent windows solved together in batched launches (include/pba.h, pba_batch.h).

Every window of a batch must produce the bits of its own solo pba_solve on an identically loaded engine: summary, iteration log,
cameras and points.  The exceptions are the wall-clock fields and num_jacobian_passes, which counts the ENQUEUED Jacobian passes of
the pipelined driver (the passes queued behind a termination the host has not seen yet are no-ops on the device), so two solo runs
may already differ there.  Each driver of the solo side (the default one and PBA_RESIDENT=0) runs in a child process."""
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

KITTI = dict(size=(376, 1241), K=(718.856, 718.856, 607.1928, 185.2157))
SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
# (window keywords, solver keywords, flat camera): one kernel key (radius 2, one channel, unit weights), everything else differs
MAIN = [
    (dict(n_frames=3, n_points=40, radius=2, **SMALL), dict(gradient_tolerance=1e10), False),                 # one workgroup; stops at iteration 0
    (dict(n_frames=5, n_points=300, radius=2, **KITTI), dict(max_num_iterations=3), False),
    (dict(n_frames=5, n_points=1500, radius=2, size=(120, 200), K=(250.0, 250.0, 100.0, 60.0)),
     dict(min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=3), True),                                      # consecutive invalid steps
    (dict(n_frames=8, n_points=3000, radius=2, size=(188, 621), K=(359.4, 359.4, 303.6, 92.6), visibility="causal", huber=0.05),
     dict(function_tolerance=1e-2), False),                                                                      # function tolerance
    (dict(n_frames=12, n_points=2500, radius=2, size=(370, 1226), K=(707.0, 707.0, 601.9, 183.1), visibility="causal"),
     dict(max_num_iterations=50, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0), False),   # 50 iterations
    (dict(n_frames=16, n_points=4000, radius=2, visibility="causal", huber=0.1, **KITTI), dict(max_num_iterations=12), False),
    (dict(n_frames=8, n_points=50000, radius=2, **KITTI), dict(max_num_iterations=6), False),                    # configs[1]: > 1024 tiles
    (dict(n_frames=4, n_points=700, radius=2, size=(188, 621), K=(359.4, 359.4, 303.6, 92.6), huber=0.05), dict(), False),
]
# further kernel keys and modes, one batch each
MODES = {
    "gaussian": [(dict(n_frames=4, n_points=300, radius=1, gaussian=True, **SMALL), dict(max_num_iterations=10), False),
                 (dict(n_frames=6, n_points=900, radius=1, gaussian=True, huber=0.05, size=(120, 200), K=(250.0, 250.0, 100.0, 60.0)),
                  dict(), False)],
    "inverse_depth": [(dict(n_frames=4, n_points=200, radius=2, seed_offset=3, **SMALL), dict(max_num_iterations=8), False),
                      (dict(n_frames=5, n_points=400, radius=2, huber=0.05, seed_offset=4, **SMALL), dict(), False)],
    "IntensityAndGradient": [(dict(n_frames=4, n_points=80, radius=2, **SMALL), dict(max_num_iterations=8), False),
                             (dict(n_frames=5, n_points=150, radius=2, huber=0.5, seed_offset=2, **SMALL), dict(), False)],
    "BitPlanes": [(dict(n_frames=4, n_points=80, radius=2, **SMALL), dict(max_num_iterations=6), False),
                  (dict(n_frames=4, n_points=120, radius=2, huber=0.05, seed_offset=1, **SMALL), dict(), False)],
    "radius3": [(dict(n_frames=4, n_points=300, radius=3, **SMALL), dict(max_num_iterations=5), False),
                (dict(n_frames=6, n_points=600, radius=3, huber=0.05, gaussian=False, size=(188, 621), K=(359.4, 359.4, 303.6, 92.6)), dict(), False)],
}

CODE = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import test_gpu_batch as t
    print("RESULT" + json.dumps(t.child(json.loads(sys.argv[1]))))
""" % (ROOT, TESTS))


def _channel_fn(kind):
    from oracle import oracle

    def fn(img):
        ch = oracle.descriptor_channels(img, kind)
        return ch, oracle.channel_planes(ch)
    return fn


def _rays(p):
    """World ray of every point through the camera of its first observation: X = o + d / rho (tests/test_gpu_inverse_depth.py)."""
    from photobundle_amd import se3
    first = np.searchsorted(p.obs_point, np.arange(p.n_points))
    rays, rho = np.zeros((p.n_points, 6)), np.zeros(p.n_points)
    for i in range(p.n_points):
        T_cw = se3.params_to_pose(p.cams[p.obs_slot[first[i]]])
        R, t = T_cw[:3, :3], T_cw[:3, 3]
        Xc = R @ p.xyz[i] + t
        o = -R.T @ t
        rho[i] = 1.0 / Xc[2]
        rays[i, :3], rays[i, 3:] = o, R.T @ (Xc / Xc[2])
    return rays, rho


def window(wkw, flat, mode="main"):
    wkw = dict(wkw)
    wkw["size"], wkw["K"] = tuple(wkw["size"]), tuple(wkw["K"])
    if mode in ("IntensityAndGradient", "BitPlanes"):
        wkw["channel_fn"] = _channel_fn(mode)
    p = synthetic.make_window(**wkw)
    if flat:
        import test_oracle_solver_options as opts
        p, _ = opts.flat_camera(p)
    return p


def engine_for(p, mode="main"):
    rows, cols = p.images.shape[1:] if p.images is not None else p.channel_images.shape[2:]
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, channels=getattr(p, "channels", 1) or 1)
    e.load(p)
    if mode == "inverse_depth":
        e.set_inverse_depth(*_rays(p))
    return e


TIME_FIELDS = ("total_time_in_seconds", "iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds")


def fingerprint(r):
    """Everything a solve returns, as exact bits, minus the wall-clock fields and num_jacobian_passes (module docstring)."""
    def enc(v):
        return v.hex() if isinstance(v, float) else v
    out = {k: enc(v) for k, v in r.items() if k not in ("iterations", "cams", "xyz", "num_jacobian_passes") + TIME_FIELDS}
    out["log"] = [{k: enc(v) for k, v in it.items() if k not in TIME_FIELDS} for it in r["iterations"]]
    out["cams"] = hashlib.sha256(np.ascontiguousarray(r["cams"]).tobytes()).hexdigest()
    out["xyz"] = hashlib.sha256(np.ascontiguousarray(r["xyz"]).tobytes()).hexdigest()
    return out


def _opts(skw):
    return default_solver_options(**skw)


def child(what):
    """Runs in a child process: solo solves on fresh engines, the batched solves of the same windows, and the order / state checks."""
    out = {}
    groups = [("main", MAIN)] + [(m, MODES[m]) for m in what.get("modes", [])]
    for mode, cases in groups:
        probs = [window(w, f, mode) for w, _, f in cases]
        skws = [s for _, s, _ in cases]
        solo = []
        for p, skw in zip(probs, skws):
            with engine_for(p, mode) as e:
                r = e.solve(_opts(skw))
                solo.append(dict(fp=fingerprint(r), driver=e.solve_driver()))
        engines = [engine_for(p, mode) for p in probs]
        try:
            res = solve_batch(engines, [_opts(s) for s in skws])
            rec = dict(solo=solo, batch=[fingerprint(r) for r in res], drivers=[e.solve_driver() for e in engines],
                       passes=[(r["num_jacobian_passes"], r["num_iterations"]) for r in res])
            if mode == "main" and what.get("order"):
                for e, p in zip(engines, probs):        # reload: the same starting point
                    e.load(p)
                perm = [5, 2, 7, 0, 3, 6, 1, 4]
                res_p = solve_batch([engines[i] for i in perm], [_opts(skws[i]) for i in perm])
                rec["permuted"] = {str(i): fingerprint(r) for i, r in zip(perm, res_p)}
                for e, p in zip(engines, probs):
                    e.load(p)
                rec["again"] = [fingerprint(r) for r in solve_batch(engines, [_opts(s) for s in skws])]
                engines[3].load(probs[3])
                rec["single"] = fingerprint(solve_batch([engines[3]], _opts(skws[3]))[0])
                # state after a batch: reload and solve alone on an engine that took part in batches
                engines[1].load(probs[1])
                rec["after"] = fingerprint(engines[1].solve(_opts(skws[1])))
                rec["after_driver"] = engines[1].solve_driver()
        finally:
            for e in engines:
                e.close()
        out[mode] = rec
    return out


def _run(env_extra, what):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", CODE, json.dumps(what)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    cache = str(tmp_path_factory.mktemp("windows"))
    return {"default": _run({"PBA_WINDOW_CACHE": cache}, dict(modes=list(MODES), order=True)),
            "pipelined": _run({"PBA_WINDOW_CACHE": cache, "PBA_RESIDENT": "0"}, dict(modes=[])),
            # the final pass and the flush as separate launches on the lent stream (no decision + flush folded into the last workgroup)
            "unfused_final": _run({"PBA_WINDOW_CACHE": cache, "PBA_FUSE_FINAL": "0"}, dict(modes=[]))}


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "log":
            assert len(a[k]) == len(b[k]), (what, len(a[k]), len(b[k]))
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                assert x == y, (what, "iteration", i, x, y)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("driver", ["default", "pipelined", "unfused_final"])
def test_every_window_of_a_batch_equals_its_solo_solve(runs, driver):
    rec = runs[driver]["main"]
    assert rec["drivers"] == ["batched"] * len(MAIN)
    # num_jacobian_passes counts enqueued passes (module docstring): at least the first linearisation + one per logged step
    for (jac, n_it), b in zip(rec["passes"], rec["batch"]):
        assert jac >= n_it >= 1, (jac, n_it, b["message"])
    if driver == "pipelined":
        assert all(s["driver"] == "pipelined" for s in rec["solo"])
    for k, (s, b) in enumerate(zip(rec["solo"], rec["batch"])):
        _same(s["fp"], b, (driver, k, MAIN[k][:2]))
    msgs = [b["message"] for b in rec["batch"]]
    # the windows end the ways they are meant to
    assert msgs[0].startswith("Gradient tolerance") and len(rec["batch"][0]["log"]) == 1, msgs[0]
    assert msgs[1].startswith("Maximum number of iterations") and len(rec["batch"][1]["log"]) == 4, msgs[1]
    assert msgs[2].startswith("Number of consecutive invalid steps"), msgs[2]
    assert msgs[3].startswith("Function tolerance"), msgs[3]
    assert msgs[4].startswith("Maximum number of iterations") and len(rec["batch"][4]["log"]) == 51, msgs[4]


def test_order_repeat_and_a_batch_of_one_give_the_same_bits(runs):
    rec = runs["default"]["main"]
    for i, b in rec["permuted"].items():
        _same(rec["batch"][int(i)], b, ("permuted", i))
    for k, b in enumerate(rec["again"]):
        _same(rec["batch"][k], b, ("again", k))
    _same(rec["batch"][3], rec["single"], "single")


def test_a_solo_solve_after_batches_equals_one_on_a_fresh_engine(runs):
    rec = runs["default"]["main"]
    _same(rec["solo"][1]["fp"], rec["after"], "after")
    assert rec["after_driver"] in ("resident", "pipelined")


@pytest.mark.parametrize("mode", list(MODES))
def test_descriptors_weights_and_inverse_depth_in_a_batch(runs, mode):
    rec = runs["default"][mode]
    assert rec["drivers"] == ["batched"] * len(MODES[mode])
    for k, (s, b) in enumerate(zip(rec["solo"], rec["batch"])):
        _same(s["fp"], b, (mode, k))


# ---- refusals: nothing runs ------------------------------------------------------------------------------------------------------
def _small(radius=2, n_frames=4, n_points=120, seed=0, kind=None):
    kw = dict(n_frames=n_frames, n_points=n_points, radius=radius, seed_offset=seed, **SMALL)
    return window(kw, False, kind or "main")


def test_refusals_leave_every_engine_as_it_was():
    from photobundle_amd import _lib
    import ctypes as C
    pa, pb = _small(seed=0), _small(seed=1, n_points=150)
    pr1 = _small(radius=1, seed=2)
    pc = _small(seed=3, kind="IntensityAndGradient")
    pw = _small(n_frames=17, n_points=200, seed=4)        # 16 free cameras: a wide window
    engines = {"a": engine_for(pa), "b": engine_for(pb), "r1": engine_for(pr1), "c": engine_for(pc), "w": engine_for(pw)}
    fresh = Engine(SMALL["size"][0], SMALL["size"][1], SMALL["K"], 2, 4)          # no problem, no cameras
    multi = engine_for(_small(seed=5))
    multi.comm_init_callback(lambda a, op: None, 0, 1)
    try:
        ref = {}
        for k, e in engines.items():
            ref[k] = fingerprint(e.solve(_opts(dict(max_num_iterations=4))))
        reload = {"a": pa, "b": pb, "r1": pr1, "c": pc, "w": pw}
        for k, e in engines.items():
            e.load(reload[k])
        a, b = engines["a"], engines["b"]
        cases = [
            ([a, engines["r1"]], "patch radius"),
            ([a, engines["c"]], "channels"),
            ([a, engines["w"]], "wide window"),
            ([a, multi], "multi-rank"),
            ([a, b, a], "the same engine"),
        ]
        for lst, why in cases:
            with pytest.raises(EngineError, match=why):
                solve_batch(lst, _opts(dict(max_num_iterations=4)))
            msg = _lib.lib().pba_last_error(lst[-1]._h if why != "the same engine" else a._h).decode()
            assert why in msg and "engine" in msg, (why, msg)
        L = _lib.lib()
        h = (C.c_void_p * 2)(a._h, fresh._h)
        s = (_lib.SolverSummary * 2)()
        assert L.pba_solve_batch(h, 2, None, s, None, 0) == -4         # PBA_ERR_STATE, naming index 1
        assert "engine 1" in L.pba_last_error(a._h).decode() and "engine 1" in L.pba_last_error(fresh._h).decode()
        h65 = (C.c_void_p * 65)(*([a._h] * 65))
        s65 = (_lib.SolverSummary * 65)()
        assert L.pba_solve_batch(h65, 65, None, s65, None, 0) == -1
        with pytest.raises(EngineError):
            solve_batch([a] * 65)
        for k, e in engines.items():          # nothing ran: every engine solves from where it was
            _same(ref[k], fingerprint(e.solve(_opts(dict(max_num_iterations=4)))), ("after refusals", k))
            assert e.solve_driver() != "batched"
    finally:
        for e in list(engines.values()) + [fresh, multi]:
            e.close()


# ---- run_kitti -b: three sequences of different lengths, two kernel keys --------------------------------------------------------
RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")


def _sequence(tmp, n_frames, seed, descriptor):
    """A synthetic KITTI-style directory (tests/test_gpu_dropin_class.py) and its config."""
    import test_gpu_dropin_class as dropin
    os.makedirs(tmp)
    size, K = (120, 160), (200.0 + 10 * seed, 200.0 + 10 * seed, 80.0, 60.0)
    dropin._write_sequence(tmp, n_frames, size, K)
    cfg = os.path.join(tmp, "seq.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\n" % (tmp, tmp))
        f.write("maxNumPoints = 4096\nslidingWindowSize = 4\npatchRadius = 1\nminScore = 0.65\nrobustThreshold = 0.05\nverbose = 0\n")
        f.write("descriptorType = %s\n" % descriptor)
    return cfg


def test_run_kitti_batch_writes_what_three_solo_runs_write(tmp_path):
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    seqs = [(7, "Intensity"), (5, "IntensityAndGradient"), (6, "Intensity")]
    cfgs = [_sequence(str(tmp_path / ("s%d" % k)), n, k, d) for k, (n, d) in enumerate(seqs)]
    solo = []
    for k, cfg in enumerate(cfgs):
        out, dump = str(tmp_path / ("solo_%d.txt" % k)), str(tmp_path / ("solo_%d.res" % k))
        r = subprocess.run([RUN, "-c", cfg, "-o", out, "-r", dump, "-p"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        solo.append((out, dump))
    args = [RUN, "-p"]
    batch = []
    for k, cfg in enumerate(cfgs):
        out, dump = str(tmp_path / ("batch_%d.txt" % k)), str(tmp_path / ("batch_%d.res" % k))
        args += ["-b", "%s:%s:%s" % (cfg, out, dump)]
        batch.append((out, dump))
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, ((so, sd), (bo, bd)) in enumerate(zip(solo, batch)):
        assert open(so, "rb").read() == open(bo, "rb").read(), ("poses", k)
        a, b = open(sd, "rb").read(), open(bd, "rb").read()
        assert a == b, ("results", k)
        assert a.count(b"result frame") == seqs[k][0] - 3, (k, a.count(b"result frame"))
    # numLevels > 1 is refused with -b, before any solve
    pyr = str(tmp_path / "pyr.cfg")
    with open(pyr, "w") as f:
        f.write(open(cfgs[0]).read() + "numLevels = 2\n")
    r = subprocess.run([RUN, "-b", "%s:%s" % (pyr, tmp_path / "x.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "numLevels" in r.stderr, r.stderr
