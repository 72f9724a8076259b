"""-m gpu: every mode pba_mode_rules.h leaves permitted next to a multi-rank transport, and the whole LM log of a multi-rank solve.

The cases are those of tests/multirank_cases.py (tests/test_multirank_cases_cpu.py shows that they hold the edges they name): patch
radius 1 and 3, Gaussian weights, Huber loss, 3- and 8-channel descriptors, inverse depths, a constant slot other than 0 and none at
all, three ranks, a rank without a block of a free camera, ranks with less than one tile, and six solver-option cases that end on a
scalar summed over the ranks (parameter tolerance: step and x norm; function tolerance: candidate cost; minimum radius) or change
the scaling and damping every rank must agree on.  Two or three processes share the one device, each with a point shard, over the
gloo callback transport with the device-side peer exchange (the harness of tests/test_gpu_solver_options.py::_worker_rank): one
mp.spawn per world size, every worker runs all jobs of its world.

The reference is never the engine: oracle.solve on the FULL window, and for the inverse-depth cases the numpy yardstick
(lm_yardstick.Dense with Ceres' rule for a candidate that cannot be evaluated, multirank_cases.RayProgram) cut at its clear iterations.
Tolerances are the single-rank ones (test_gpu_parity.py::_compare_traces, test_gpu_anchors.py::_check_trace): decisions equal,
cost 1e-9, radius 1e-6, both gradient norms 1e-6, step norm 1e-5, model cost change 1e-7, initial cost 1e-12, final cost 1e-9, cameras
1e-5 absolute; the reduced system of the first step at 1e-9 of its largest entry (test_gpu_inverse_depth.py).  relative_decrease has
no bar of its own there; it is a quotient of logged quantities, rd = (c_prev - c_new) / m, so the bars above bound it:
|rd' - rd| <= 1e-9 (|c_prev| + |c_new|) / |m| + 1e-7 |rd|, and that is what is asserted.  The only engine-to-engine comparisons are
bit identities: the replicas of one solve, and PBA_FORCE_MULTI=1 at world 1 against the engine without a transport.

Largest differences to the reference on one MI355X (relative, cameras absolute; printed by every run as MAXDIFF; every case ran on the
pipelined driver over callback+peer):
  case                       cost     gradient_norm  step_norm  model_cost_change  cameras   first step's S / rhs
  r1-gauss-huber-causal-w3   1.9e-15  6.5e-13        3.2e-11    4.3e-12            1.5e-11   4.4e-13 / 5.3e-14
  r3-dense-w2                1.8e-15  7.4e-12        4.1e-12    5.8e-13            6.0e-13   5.1e-14 / 7.9e-14
  r2-causal-70-w3            7.9e-16  7.2e-14        2.8e-12    1.0e-13            2.7e-12   7.5e-14 / 1.4e-13
  ig-w2                      5.2e-16  6.8e-14        1.1e-11    1.4e-13            2.9e-13   5.0e-14 / 8.0e-14
  bitplanes-w2               4.4e-16  2.1e-13        3.1e-11    4.4e-13            5.5e-13   6.9e-14 / 5.5e-14
  inverse-depth-w2           0.0      2.2e-13        2.5e-08    8.0e-09            5.1e-11   7.0e-12 / 3.6e-11   (rho 1.7e-11)
  inverse-depth-clean-w2     2.5e-11  1.3e-09        5.2e-09    1.0e-10            4.6e-09   1.4e-11 / 4.0e-11   (rho 2.8e-10)
  slot2-constant-w2          9.1e-16  8.7e-15        1.9e-12    5.2e-14            2.6e-13   5.8e-14 / 9.0e-14
  no-constant-w2             7.2e-16  1.6e-12        4.4e-12    7.6e-14            6.0e-12   5.0e-14 / 9.2e-14
  plain/G_parameter          3.1e-15  3.5e-12        7.0e-11    4.7e-13            2.2e-12
  plain/G_function           3.1e-15  1.9e-12        9.0e-13    7.2e-14            2.3e-12
  plain/E_min_radius         3.1e-15  3.4e-15        1.1e-13    1.6e-14            2.0e-14
  plain/A_no_jacobi          4.8e-10  9.4e-08        7.6e-11    5.9e-13            6.2e-12   (20 iterations without Jacobi scaling; radius 7.0e-9)
  plain/B_min_diag           5.1e-15  3.1e-12        9.3e-11    4.8e-13            4.6e-12
  huber/G_parameter          2.6e-15  5.6e-13        2.2e-11    7.1e-13            6.9e-14
Every case sits inside the single-rank bars, so none needed the twin-based bar (20 x the distance of the oracle's one-ulp twin)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import multirank_cases as mc
import test_gpu_solver_options as gso

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

LOG_FIELDS = ("iteration", "step_is_valid", "step_is_nonmonotonic", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "eta", "step_size", "linear_solver_iterations",
              "model_cost_change", "candidate_cost")      # every field of the log but the wall-clock ones
SUMMARY_FIELDS = ("initial_cost", "final_cost", "fixed_cost", "num_successful_steps", "num_unsuccessful_steps", "num_iterations",
                  "num_residuals", "num_residual_blocks", "termination_type", "message")


def _record(e, res):
    S, rhs = e.reduced_system()
    return dict(log=[{k: it[k] for k in LOG_FIELDS} for it in res["iterations"]], summary={k: res[k] for k in SUMMARY_FIELDS},
                cams=res["cams"].tolist(), xyz=res["xyz"].tolist(), S=S.tolist(), rhs=rhs.tolist(), driver=e.solve_driver())


def _worker(rank, world, port, out_dir, jobs):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["PBA_WAIT_TIMEOUT_S"] = "30"          # a desynchronised rank becomes PBA_ERR_COMM, not a hang
    import torch
    import torch.distributed as dist
    from photobundle_amd.engine import default_solver_options
    from gpu_util import make_engine
    import multirank_cases as cases
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(a, op):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)

    out = {}
    for name, kw, with_first in jobs:
        sh, rays, rho = cases.shard(name, rank)
        e = make_engine(sh, keep_reduced_system=True)
        if rays is not None:
            e.set_inverse_depth(rays, rho)
        e.comm_init_callback(allreduce, rank, world)
        out[name] = dict(transport=e.comm_enable_peer_exchange(), point_range=[int(v) for v in sh.meta["point_range"]])
        if with_first:      # a one-iteration solve: the reduced system it leaves is the first step's
            out[name]["first"] = _record(e, e.solve(default_solver_options(max_num_iterations=1)))
            e.load(sh)
            if rays is not None:
                e.set_inverse_depth(rays, rho)
        out[name]["full"] = _record(e, e.solve(default_solver_options(**kw)))
        dist.barrier()       # nobody frees its mailbox while a peer may still read it
        e.close()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


def _spawn(world, out_dir, offset):
    import torch.multiprocessing as mp
    jobs = [(name, mc.reference(name)["solver"], name in mc.MODE_CASES) for name in mc.names_of_world(world)]
    port = 29500 + ((os.getpid() + offset) % 2000)
    mp.spawn(_worker, args=(world, port, str(out_dir), jobs), nprocs=world, join=True)
    return [json.load(open(os.path.join(str(out_dir), "rank%d.json" % k))) for k in range(world)]


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    return _spawn(2, tmp_path_factory.mktemp("world2"), 211)


@pytest.fixture(scope="module")
def world3(tmp_path_factory):
    return _spawn(3, tmp_path_factory.mktemp("world3"), 223)


def _ranks(request, name):
    return [r[name] for r in request.getfixturevalue("world%d" % mc.world_of(name))]


# ---- 1. replicas ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", mc.NAMES)
def test_replicas_agree_to_the_bit(request, name):
    ranks = _ranks(request, name)
    p, _, _ = mc.window(name)
    assert len(ranks) == mc.world_of(name)
    assert len({r["transport"] for r in ranks}) == 1
    # the driver that ran: the pipelined one needs the device-side exchange, the host-staged transport is stepped by the host
    expected = "pipelined" if ranks[0]["transport"] == "callback+peer" else "host-stepped"
    print("%s: transport %s, driver %s" % (name, ranks[0]["transport"], ranks[0]["full"]["driver"]))
    for tag in ("first", "full") if name in mc.MODE_CASES else ("full",):
        a = ranks[0][tag]
        for b in ranks:
            assert b[tag]["driver"] == expected, (name, tag, ranks[0]["transport"], b[tag]["driver"])
            assert b[tag]["log"] == a["log"], (name, tag)
            assert b[tag]["summary"] == a["summary"], (name, tag)
            assert b[tag]["cams"] == a["cams"] and b[tag]["S"] == a["S"] and b[tag]["rhs"] == a["rhs"], (name, tag)
        assert np.array(a["S"]).shape == (6 * (p.n_frames - len(mc.constant_slots(p))),) * 2
    # the shards' points are the window's, in rank order
    assert [r["point_range"] for r in ranks] == [list(mc.shard(name, k)[0].meta["point_range"]) for k in range(len(ranks))]
    assert sum(len(r["full"]["xyz"]) for r in ranks) == p.n_points


# ---- 2. the log against the reference ----------------------------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(a) if a != 0.0 else abs(b)


def _check_log(name, ref, res):
    """The whole log and the summary against the reference (ref: a result in the oracle's shape).  Returns the largest differences."""
    ri, gi = ref["iterations"], res["log"]
    assert len(ri) == len(gi), (name, ref["message"], res["summary"]["message"])
    worst = dict(cost=0.0, gradient_norm=0.0, gradient_max_norm=0.0, step_norm=0.0, model_cost_change=0.0, trust_region_radius=0.0,
                 relative_decrease=0.0)
    for a, b in zip(ri, gi):
        i = a["iteration"]
        print(name, i, "ok %d %d" % (a["step_is_successful"], b["step_is_successful"]), "cost %.12e %.12e" % (a["cost"], b["cost"]),
              "|g| %.9e %.9e" % (a["gradient_norm"], b["gradient_norm"]), "step %.9e %.9e" % (a["step_norm"], b["step_norm"]),
              "mcc %.9e %.9e" % (a["model_cost_change"], b["model_cost_change"]), "rd %.6e %.6e" % (a["relative_decrease"], b["relative_decrease"]),
              "radius %.6e %.6e" % (a["trust_region_radius"], b["trust_region_radius"]))
        assert b["iteration"] == i
        assert (a["step_is_valid"], a["step_is_successful"]) == (b["step_is_valid"], b["step_is_successful"]), (name, i)
        for k, tol in (("cost", 1e-9), ("trust_region_radius", 1e-6), ("gradient_max_norm", 1e-6), ("gradient_norm", 1e-6)):
            assert np.isclose(a[k], b[k], rtol=tol, atol=0.0), (name, i, k, a[k], b[k])
            worst[k] = max(worst[k], _rel(a[k], b[k]))
        if i > 0 and a["step_is_valid"]:
            for k, tol in (("step_norm", 1e-5), ("model_cost_change", 1e-7)):
                assert np.isclose(a[k], b[k], rtol=tol, atol=0.0), (name, i, k, a[k], b[k])
                worst[k] = max(worst[k], _rel(a[k], b[k]))
            if a["cost"] == mc.EVAL_FAILED:
                # a candidate that could not be evaluated: the cost Ceres gives it, to the bit
                assert b["cost"] == mc.EVAL_FAILED and b["cost_change"] == a["cost_change"], (name, i)
            else:
                # (module docstring) a quotient of logged quantities: bounded by the bars of its parts
                c_new = a["cost"]                       # (a rejected step logs the candidate's cost)
                c_prev = c_new + a["cost_change"]
                bar = 1e-9 * (abs(c_prev) + abs(c_new)) / abs(a["model_cost_change"]) + 1e-7 * abs(a["relative_decrease"])
                d = abs(a["relative_decrease"] - b["relative_decrease"])
                assert d <= 1.01 * bar, (name, i, a["relative_decrease"], b["relative_decrease"], bar)
                assert np.isclose(b["cost_change"], a["cost_change"], rtol=0.0, atol=1e-9 * (abs(c_prev) + abs(c_new))), (name, i)
                worst["relative_decrease"] = max(worst["relative_decrease"], d / bar)
    return worst


@pytest.mark.parametrize("name", mc.NAMES)
def test_log_matches_the_reference(request, name):
    ranks = _ranks(request, name)
    p, rays, _ = mc.window(name)
    case = mc.reference(name)
    ref, res = case["res"], ranks[0]["full"]
    worst = _check_log(name, ref, res)
    s = res["summary"]
    assert s["termination_type"] == ref["termination_type"] and s["num_successful_steps"] == ref["num_successful_steps"], (name, s["message"])
    assert np.isclose(s["initial_cost"], ref["initial_cost"], rtol=1e-12, atol=0.0)
    assert np.isclose(s["final_cost"], ref["final_cost"], rtol=1e-9, atol=0.0)
    assert s["fixed_cost"] == 0.0
    assert s["num_residuals"] == mc.num_residuals(p) and s["num_residual_blocks"] == p.n_obs       # of the FULL window, on every rank
    cams = np.array(res["cams"])
    worst["cameras"] = float(np.abs(cams - ref["cams"]).max())
    assert worst["cameras"] <= 1e-5, (name, worst)
    for c in mc.constant_slots(p):
        assert cams[c].tobytes() == np.ascontiguousarray(p.cams[c], np.float64).tobytes(), name
    pts = np.concatenate([np.array(r["full"]["xyz"]) for r in ranks])
    assert pts.shape == (p.n_points, 3)
    if rays is not None:
        # inverse depths: (rho, 0, 0), rho > 0 on every rank, and the yardstick's state
        assert (pts[:, 0] > 0.0).all() and not pts[:, 1:].any()
        worst["rho"] = float(np.abs(pts[:, :1] - ref["points"]).max())
        assert worst["rho"] <= 1e-5, (name, worst)
    if name in mc.OPTION_CASES:
        gso._check_message(ref["message"], s["message"], name)
        assert s["message"].startswith(case["kind"]), (name, s["message"])
        if case["cid"] in ("G_parameter", "G_function"):
            # the terminating test reads a sum over the ranks: the solve stops at the oracle's iteration
            assert s["num_iterations"] == len(ref["iterations"]) and len(res["log"]) == len(ref["iterations"])
    else:
        assert s["message"].startswith("Maximum number of iterations"), (name, s["message"])
    print("MAXDIFF %-26s " % name + "  ".join("%s %.1e" % (k, worst[k]) for k in ("cost", "gradient_norm", "step_norm", "model_cost_change", "cameras")) +
          "  (gradient_max_norm %.1e, radius %.1e, relative_decrease %.2f of its bar%s)" % (
              worst["gradient_max_norm"], worst["trust_region_radius"], worst["relative_decrease"], ", rho %.1e" % worst["rho"] if "rho" in worst else ""))


# ---- 3. the reduced system every rank holds after the exchange ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.MODE_CASES))
def test_reduced_system_of_the_first_step(request, name):
    """The system left by a one-iteration solve is the first step's: the Schur complement of the FULL window although every rank
    eliminated its own points only (and a rank that misses a camera has no scale or damping of that column before the exchange)."""
    ranks = _ranks(request, name)
    S_ref, rhs_ref = mc.first_system(name)
    S, rhs = np.array(ranks[0]["first"]["S"]), np.array(ranks[0]["first"]["rhs"])
    assert S.shape == S_ref.shape and rhs.shape == rhs_ref.shape
    d_S, d_rhs = np.abs(S - S_ref).max() / np.abs(S_ref).max(), np.abs(rhs - rhs_ref).max() / np.abs(rhs_ref).max()
    print("%s: n %d, S %.3e, rhs %.3e of the largest entry" % (name, S.shape[0], d_S, d_rhs))
    assert d_S <= 1e-9 and d_rhs <= 1e-9
    assert len(ranks[0]["first"]["log"]) == 2


# ---- 4. the multi-rank code path at world 1 ----------------------------------------------------------------------------------------------
CODE = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    from photobundle_amd.engine import default_solver_options
    from gpu_util import make_engine
    import multirank_cases as cases
    out = {}
    for name, kw in json.loads(sys.argv[1]):
        p, rays, rho = cases.window(name)
        e = make_engine(p)
        if rays is not None:
            e.set_inverse_depth(rays, rho)
        transport = "none"
        if os.environ.get("PBA_FORCE_MULTI") == "1":
            e.comm_init_callback(lambda a, op: None, 0, 1)      # world 1: every all-reduce is the identity
            transport = e.comm_enable_peer_exchange()
        r = e.solve(default_solver_options(**kw))
        out[name] = dict(transport=transport, driver=e.solve_driver(), message=r["message"], cams=r["cams"].tolist(), xyz=r["xyz"].tolist(),
                         log=[{k: it[k] for k in %r} for it in r["iterations"]])
        e.close()
    print("RESULT" + json.dumps(out))
""" % (ROOT, TESTS, LOG_FIELDS))


@pytest.mark.timeout(600)
def test_forced_multirank_path_gives_the_single_rank_bits():
    """PBA_FORCE_MULTI=1 at world 1 over the callback transport (no RCCL needed) runs the multi-rank code of both drivers -- packed
    reduced system, one scalar exchange, decisions after it -- on every mode case.  Asynchronously (its own mailbox is the only peer) it
    gives the bits of the engine without a transport; with PBA_ASYNC=0 the host-stepped driver is at the bars
    tests/test_gpu_multirank.py::test_rccl_collectives_on_the_device_stream holds it to: costs 1e-11, cameras 1e-9."""
    jobs = [(name, mc.reference(name)["solver"]) for name in mc.MODE_CASES]
    outs = {}
    for tag, env in (("plain", {}), ("multi_async", {"PBA_FORCE_MULTI": "1"}), ("multi_sync", {"PBA_FORCE_MULTI": "1", "PBA_ASYNC": "0"})):
        full = {k: v for k, v in os.environ.items() if k not in ("PBA_FORCE_MULTI", "PBA_ASYNC", "PBA_RESIDENT")}
        r = subprocess.run([sys.executable, "-c", CODE, json.dumps(jobs)], env=dict(full, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    for name, _ in jobs:
        plain, a, s = outs["plain"][name], outs["multi_async"][name], outs["multi_sync"][name]
        assert plain["transport"] == "none" and plain["driver"] in ("pipelined", "resident"), (name, plain["driver"])      # (the same bits)
        assert s["driver"] == "host-stepped", (name, s["driver"])
        costs = lambda o: [i["cost"] for i in o["log"]]
        if a["transport"] == "callback+peer":
            assert a["driver"] == "pipelined", (name, a["driver"])
            assert a["log"] == plain["log"] and a["cams"] == plain["cams"] and a["xyz"] == plain["xyz"] and a["message"] == plain["message"], name
        else:      # no device-side exchange on this machine: the host steps the host-staged transport
            assert a["driver"] == "host-stepped", (name, a["transport"], a["driver"])
            assert a["log"] == s["log"] and a["cams"] == s["cams"], name
        assert len(s["log"]) == len(plain["log"]), name
        assert [(i["step_is_valid"], i["step_is_successful"]) for i in s["log"]] == [(i["step_is_valid"], i["step_is_successful"]) for i in plain["log"]]
        assert np.allclose(costs(s), costs(plain), rtol=1e-11, atol=0.0), name
        assert np.abs(np.array(s["cams"]) - np.array(plain["cams"])).max() <= 1e-9, name
