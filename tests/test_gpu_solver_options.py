"""-m gpu: non-default solver options and every LM termination on every driver.

The cases of tests/test_oracle_solver_options.py (the oracle there is pinned to an independent dense loop at the same options) run
on the engine through three drivers, each in a process of its own because the driver is chosen at pba_create:
  resident      PBA_RESIDENT=1   the whole solve as one cooperative launch (pba_resident.h)
  pipelined     PBA_RESIDENT=0   the three-kernel asynchronous driver, decisions on the device (pba_lm_rules.h lm_decide)
  host-stepped  PBA_ASYNC=0      the host loop of pba_lm.cpp over the same lm_decide
Each run asserts the driver that actually ran it.  Every driver is compared with the oracle (the tolerances of
test_gpu_parity.py::_compare_traces), the resident driver with the pipelined one bit for bit, the host-stepped one with the
pipelined one at the tolerances of the multi_sync comparison in test_gpu_multirank.py."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle import oracle
from photobundle_amd import synthetic
import test_oracle_solver_options as opts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

BASE = dict(n_frames=5, n_points=1500, radius=2, size=(120, 200), K=(250.0, 250.0, 100.0, 60.0))
WINDOWS = {"plain": BASE, "huber": dict(BASE, huber=0.05)}
N_IT = 20
DRIVERS = {"resident": {"PBA_RESIDENT": "1"}, "pipelined": {"PBA_RESIDENT": "0"}, "host-stepped": {"PBA_ASYNC": "0"}}
HUBER_CASES = ("A_no_jacobi", "D_min_decrease", "F_grad_mid")


def _window(name, flat=None):
    p = synthetic.make_window(**WINDOWS[name])
    if flat == "camera":
        return opts.flat_camera(p)
    if flat == "point":
        return opts.flat_point(p)
    return p, None


def _jobs():
    """[(job id, window name, flat, solver keywords, termination message prefix)]"""
    jobs = []
    for name in WINDOWS:
        p, _ = _window(name)
        ref = oracle.solve(p, oracle.default_options(max_num_iterations=N_IT, **opts.TOLERANCES_OFF))
        for cid, kw, kind in opts.option_cases(p, ref, N_IT):
            if name == "plain" or cid in HUBER_CASES:
                jobs.append(("%s/%s" % (name, cid), name, None, kw, kind))
    for flat in ("camera", "point"):
        for cid, kw, kind, _ in opts.invalid_cases():
            jobs.append(("flat_%s/%s" % (flat, cid), "plain", flat, kw, kind))
    return jobs


CODE = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    from photobundle_amd.engine import Engine, default_solver_options
    import test_gpu_solver_options as t
    jobs = json.loads(sys.argv[1])
    out = {}
    engines = {}
    try:
        for jid, name, flat, kw, kind in jobs:
            p, _ = t._window(name, flat)
            key = (name, flat)
            if key not in engines:
                rows, cols = t.WINDOWS[name]["size"]
                engines[key] = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber)   # flag bit 0 off: the resident driver may run
            e = engines[key]
            e.load(p)
            r = e.solve(default_solver_options(**kw))
            its = [{k: (v.hex() if isinstance(v, float) else v) for k, v in i.items()} for i in r["iterations"]]
            out[jid] = dict(driver=e.solve_driver(), its=its, message=r["message"], cams=r["cams"].tobytes().hex(), xyz=r["xyz"].tobytes().hex(),
                            **{k: (r[k].hex() if isinstance(r[k], float) else r[k]) for k in ("initial_cost", "final_cost", "termination_type",
                               "num_successful_steps", "num_unsuccessful_steps", "num_iterations")})
    finally:
        for e in engines.values():
            e.close()
    print("RESULT" + json.dumps(out))
""" % (ROOT, TESTS))


def _run(driver, jobs):
    env = dict(os.environ)
    for k in ("PBA_RESIDENT", "PBA_ASYNC"):
        env.pop(k, None)
    env.update(DRIVERS[driver])
    r = subprocess.run([sys.executable, "-c", CODE, json.dumps(jobs)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    for res in out.values():
        res["iterations"] = [{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in i.items()} for i in res["its"]]
        for k in ("initial_cost", "final_cost"):
            res[k] = float.fromhex(res[k])
        res["cams_a"] = np.frombuffer(bytes.fromhex(res["cams"]), np.float64).reshape(-1, 6)
        res["xyz_a"] = np.frombuffer(bytes.fromhex(res["xyz"]), np.float64).reshape(-1, 3)
    return out


@pytest.fixture(scope="module")
def runs():
    jobs = _jobs()
    refs = {}
    for jid, name, flat, kw, kind in jobs:
        p, idx = _window(name, flat)
        refs[jid] = (p, idx, oracle.solve(p, oracle.default_options(**kw)), kw, kind)
    return refs, {d: _run(d, jobs) for d in DRIVERS}


JOB_IDS = (["plain/" + c for c in opts.OPTION_IDS] + ["huber/" + c for c in HUBER_CASES] +
           ["flat_%s/%s" % (f, c[0]) for f in ("camera", "point") for c in opts.invalid_cases()])
_NUM = re.compile(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|inf|nan)")


def _check_message(a, b, jid):
    ha, _, ta = a.partition(":")
    hb, _, tb = b.partition(":")
    assert ha == hb, (jid, a, b)
    na, nb = [float(x) for x in _NUM.findall(ta)], [float(x) for x in _NUM.findall(tb)]
    assert len(na) == len(nb) and np.allclose(na, nb, rtol=1e-6, atol=0), (jid, a, b)


def _against_oracle(p, ref, res, jid):
    ri, gi = ref["iterations"], res["iterations"]
    assert len(ri) == len(gi), (jid, ref["message"], res["message"])
    for a, b in zip(ri, gi):
        assert a["iteration"] == b["iteration"]
        assert (a["step_is_successful"], a["step_is_valid"]) == (b["step_is_successful"], b["step_is_valid"]), (jid, a["iteration"])
        assert np.isclose(a["cost"], b["cost"], rtol=1e-9), (jid, a["iteration"])
        assert np.isclose(a["trust_region_radius"], b["trust_region_radius"], rtol=1e-6), (jid, a["iteration"])
        assert np.isclose(a["gradient_max_norm"], b["gradient_max_norm"], rtol=1e-6), (jid, a["iteration"])
        assert np.isclose(a["gradient_norm"], b["gradient_norm"], rtol=1e-6), (jid, a["iteration"])
        if a["iteration"] > 0 and a["step_is_valid"]:
            assert np.isclose(a["step_norm"], b["step_norm"], rtol=1e-5), (jid, a["iteration"])
    for k in ("termination_type", "num_successful_steps", "num_unsuccessful_steps"):
        assert res[k] == ref[k], (jid, k, res[k], ref[k])
    _check_message(ref["message"], res["message"], jid)
    assert np.isclose(res["initial_cost"], ref["initial_cost"], rtol=1e-12)
    assert np.isclose(res["final_cost"], ref["final_cost"], rtol=1e-9)
    assert np.abs(res["cams_a"] - ref["cams"]).max() <= 1e-5, jid
    assert np.array_equal(res["cams_a"][p.fixed_slot], p.cams[p.fixed_slot])


@pytest.mark.parametrize("jid", JOB_IDS)
def test_case_on_every_driver(runs, jid):
    refs, out = runs
    p, idx, ref, kw, kind = refs[jid]
    cid = jid.split("/")[1]
    if not jid.startswith("flat"):
        opts.check_case_shape(cid, ref, kind, kw["max_num_iterations"])
    elif kind is not None:
        assert ref["message"].startswith(kind), ref["message"]
    long_limit = kw.get("max_num_iterations", 500) >= 1022         # beyond the device log: the host-stepped driver, whatever the setting
    for d in DRIVERS:
        res = out[d][jid]
        assert res["driver"] == ("host-stepped" if long_limit else d), (jid, d, res["driver"])
        _against_oracle(p, ref, res, jid)
        if jid.startswith("flat"):
            its = res["iterations"]
            if kind is not None:
                n_invalid = [c for c in opts.invalid_cases() if c[0] == cid][0][3]
                assert len(its) == 1 + n_invalid and all(i["step_is_valid"] == 0 for i in its[1:]), (jid, d)
                assert [i["trust_region_radius"] for i in its] == [i["trust_region_radius"] for i in ref["iterations"]], (jid, d)
                assert res["termination_type"] == (2 if kind == opts.INVALID else 0)
                assert res["final_cost"] == res["initial_cost"], (jid, d)
                assert np.array_equal(res["cams_a"], p.cams) and np.array_equal(res["xyz_a"], p.xyz), (jid, d)
            else:
                moved = res["cams_a"][idx] if "camera" in jid else res["xyz_a"][idx]
                assert np.array_equal(moved, p.cams[idx] if "camera" in jid else p.xyz[idx]), (jid, d)
    # resident against pipelined: the same device functions on the same tiles, reduced in the same order -> bit-identical
    a, b = out["resident"][jid], out["pipelined"][jid]
    untimed = lambda its: [{k: v for k, v in i.items() if not k.endswith("_in_seconds")} for i in its]
    assert untimed(a["its"]) == untimed(b["its"]), jid
    for f in ("message", "cams", "xyz", "final_cost", "initial_cost"):
        assert a[f] == b[f], (jid, f)
    # host-stepped against pipelined (test_gpu_multirank.py multi_sync)
    h = out["host-stepped"][jid]
    assert len(h["iterations"]) == len(b["iterations"])
    assert np.allclose([i["cost"] for i in h["iterations"]], [i["cost"] for i in b["iterations"]], rtol=1e-11), jid
    assert np.abs(h["cams_a"] - b["cams_a"]).max() <= 1e-9, jid


def test_a_long_iteration_limit_gives_the_device_trace(runs):
    """max_num_iterations = 2000 routes to the host-stepped driver; ending early on a tolerance it must give the trace of the same
    solve at the 500 limit on the device drivers."""
    _, out = runs
    for d in ("resident", "pipelined"):
        a, b = out[d]["plain/I_long_limit"], out[d]["plain/F_grad_mid"]
        assert a["driver"] == "host-stepped" and b["driver"] == d
        assert [i["step_is_successful"] for i in a["iterations"]] == [i["step_is_successful"] for i in b["iterations"]]
        assert np.allclose([i["cost"] for i in a["iterations"]], [i["cost"] for i in b["iterations"]], rtol=1e-11)
        assert np.abs(a["cams_a"] - b["cams_a"]).max() <= 1e-9
        _check_message(a["message"], b["message"], d)


# ---- multi-rank: two ranks on one device over the gloo harness of test_gpu_multirank.py ------------------------------------------------
def _worker_rank(rank, world, port, out_dir, jobs):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["PBA_WAIT_TIMEOUT_S"] = "30"          # a stuck exchange becomes PBA_ERR_COMM, not a hang
    import torch
    import torch.distributed as dist
    from photobundle_amd.engine import default_solver_options
    from gpu_util import make_engine
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(a, op):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)

    out = {}
    for jid, name, flat, kw in jobs:
        p, idx = _window(name, flat)
        sh = p.shard(rank, world)
        e = make_engine(sh, keep_reduced_system=False)
        e.comm_init_callback(allreduce, rank, world)
        transport = e.comm_enable_peer_exchange()
        res = e.solve(default_solver_options(**kw))
        out[jid] = dict(transport=transport, driver=e.solve_driver(), message=res["message"], termination_type=res["termination_type"],
                        costs=[i["cost"] for i in res["iterations"]], ok=[(i["step_is_valid"], i["step_is_successful"]) for i in res["iterations"]],
                        cams=res["cams"].tolist(), xyz=res["xyz"].tolist(), point_range=list(map(int, sh.meta["point_range"])))
        dist.barrier()       # nobody frees its mailbox while a peer may still read it
        e.close()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_match_the_single_rank_pipelined_trace(runs, tmp_path):
    """A flat point on ONE rank's shard (its Schur elimination failure must reach both ranks' decisions) and the deferred gradient check
    mid-solve (against the multi-rank over-enqueue of pba_lm.cpp): both ranks give the single-rank pipelined trace."""
    import torch.multiprocessing as mp
    refs, out = runs
    jobs = [("flat_point/H_invalid_3", "plain", "point", refs["flat_point/H_invalid_3"][3]),
            ("plain/F_grad_mid", "plain", None, refs["plain/F_grad_mid"][3])]
    world = 2
    port = 29500 + ((os.getpid() + 131) % 2000)
    mp.spawn(_worker_rank, args=(world, port, str(tmp_path), jobs), nprocs=world, join=True)
    r = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in range(world)]
    for jid, name, flat, kw in jobs:
        single = out["pipelined"][jid]
        a, b = r[0][jid], r[1][jid]
        assert a["transport"] == b["transport"]
        expected = "pipelined" if a["transport"] == "callback+peer" else "host-stepped"
        assert a["driver"] == b["driver"] == expected, (jid, a["transport"], a["driver"], b["driver"])
        if flat == "point":
            j = refs[jid][1]
            inside = [lo <= j < hi for lo, hi in (a["point_range"], b["point_range"])]
            assert sum(inside) == 1, (j, a["point_range"], b["point_range"])
        assert a["costs"] == b["costs"] and a["ok"] == b["ok"] and a["message"] == b["message"] and a["cams"] == b["cams"]
        assert [tuple(x) for x in a["ok"]] == [(i["step_is_valid"], i["step_is_successful"]) for i in single["iterations"]], jid
        assert np.allclose(a["costs"], [i["cost"] for i in single["iterations"]], rtol=1e-9), jid
        assert a["termination_type"] == single["termination_type"]
        _check_message(single["message"], a["message"], jid)
        assert np.abs(np.array(a["cams"]) - single["cams_a"]).max() <= 1e-8, jid
        assert np.abs(np.concatenate([a["xyz"], b["xyz"]]) - single["xyz_a"]).max() <= 1e-6, jid
