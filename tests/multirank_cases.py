"""The multi-rank cases shared by tests/test_multirank_cases_cpu.py (the cases are what they claim to be) and
tests/test_gpu_multirank_modes.py (the engine on them): every mode pba_mode_rules.h leaves permitted next to a multi-rank transport,
at the smallest shapes that still hold the edge, and the solver-option cases that end a solve on a summed scalar.

A case is (make_window keywords, world, mode, solver keywords).  mode is a dict: channels (the descriptor type of a multi-channel
window), inverse_depth (rays and rho from synthetic.inverse_depth_rays, sharded by the same [lo, hi) as the points), fixed_slot (the
constant slot, -1 for none), misses_free_slot (some rank has no block of a free camera) and sub_tile (every rank has fewer than one
128-observation tile).  The option cases take window and keywords from tests/test_gpu_solver_options.py and
tests/test_oracle_solver_options.py and are resolved on the oracle's default trace like there.

The reference of a case is never the engine: oracle.solve on the FULL window, or for inverse depths the numpy yardstick
(lm_yardstick.Dense) cut at its clear iterations."""
import functools
import sys

import numpy as np

from oracle import oracle
from photobundle_amd import synthetic

import lm_yardstick as lm
import test_gpu_solver_options as gso
import test_oracle_solver_options as opts

SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
TILE = 128          # observations of one tile of the point-walking kernels
EVAL_FAILED = sys.float_info.max      # the cost Ceres gives a candidate that cannot be evaluated (DBL_MAX in the engine's log)

MODE_CASES = {
    # shards (points, blocks) = (59, 349), (77, 356), (104, 354); rank 2 sees slots {2, 3, 4, 5} only: no block of the constant slot 0 and
    # none of the free slot 1.  Rejected steps and radius halving are part of the trace.
    "r1-gauss-huber-causal-w3": (dict(n_frames=6, n_points=240, radius=1, visibility="causal", huber=0.05, gaussian=True), 3,
                                 dict(misses_free_slot=True, rejects=True), dict(max_num_iterations=8)),
    "r3-dense-w2": (dict(n_frames=3, n_points=130, radius=3), 2, dict(), dict(max_num_iterations=6)),
    # shards of 18, 22 and 30 points: less than one tile on every rank; rank 2 misses slot 0
    "r2-causal-70-w3": (dict(n_frames=5, n_points=70, radius=2, visibility="causal"), 3, dict(sub_tile=True), dict(max_num_iterations=6)),
    "ig-w2": (dict(n_frames=4, n_points=90, radius=2), 2, dict(channels="IntensityAndGradient"), dict(max_num_iterations=6)),
    "bitplanes-w2": (dict(n_frames=4, n_points=90, radius=2), 2, dict(channels="BitPlanes"), dict(max_num_iterations=6)),
    # seven of its eight steps lead through a camera centre (a candidate rho <= 0) for points 119 .. 131, all of rank 1: an evaluation
    # failure that rank 0 learns of through the exchange alone (kEvalFailCand); one step is accepted
    "inverse-depth-w2": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, seed_offset=3), 2,
                         dict(inverse_depth=True, eval_failure_on_one_rank=True), dict(max_num_iterations=8)),
    # the same shape on a window whose candidates all stay in front of their cameras: six accepted steps
    "inverse-depth-clean-w2": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, seed_offset=4), 2, dict(inverse_depth=True),
                               dict(max_num_iterations=8)),
    "slot2-constant-w2": (dict(n_frames=4, n_points=150, radius=2, visibility="causal"), 2, dict(fixed_slot=2), dict(max_num_iterations=6)),
    # (the options of tests/test_gpu_edge_cases.py::test_no_constant_camera)
    "no-constant-w2": (dict(n_frames=4, n_points=150, radius=2, visibility="causal"), 2, dict(fixed_slot=-1), dict(max_num_iterations=6)),
}
# (window of tests/test_gpu_solver_options.py, case of test_oracle_solver_options.option_cases), all on two ranks
OPTION_CASES = {"plain/G_parameter": 2, "plain/G_function": 2, "plain/E_min_radius": 2, "plain/A_no_jacobi": 2, "plain/B_min_diag": 2,
                "huber/G_parameter": 2}
NAMES = list(MODE_CASES) + list(OPTION_CASES)
WORLDS = (2, 3)


def world_of(name):
    return MODE_CASES[name][1] if name in MODE_CASES else OPTION_CASES[name]


def mode_of(name):
    return MODE_CASES[name][2] if name in MODE_CASES else {}


def names_of_world(world):
    return [n for n in NAMES if world_of(n) == world]


@functools.lru_cache(maxsize=None)
def _option_window(window_name):
    return gso._window(window_name)[0]


@functools.lru_cache(maxsize=None)
def window(name):
    """(full window, rays or None, rho or None) of a case."""
    if name in OPTION_CASES:
        return _option_window(name.split("/")[0]), None, None
    kw, _, mode, _ = MODE_CASES[name]
    fn = synthetic.channel_fn(mode["channels"]) if "channels" in mode else None
    p = synthetic.make_window(channel_fn=fn, **kw, **SMALL)
    if "fixed_slot" in mode:
        p.fixed_slot = mode["fixed_slot"]
    if mode.get("inverse_depth"):
        rays, rho = synthetic.inverse_depth_rays(p)
        return p, rays, rho
    return p, None, None


def shard(name, rank):
    """(rank's shard, its rays or None, its rho or None)."""
    p, rays, rho = window(name)
    sh = p.shard(rank, world_of(name))
    lo, hi = sh.meta["point_range"]
    return sh, (None if rays is None else rays[lo:hi]), (None if rho is None else rho[lo:hi])


def constant_slots(p):
    return (p.fixed_slot,) if p.fixed_slot >= 0 else ()


@functools.lru_cache(maxsize=None)
def _option_cases(window_name):
    p = _option_window(window_name)
    ref = oracle.solve(p, oracle.default_options(max_num_iterations=gso.N_IT, **opts.TOLERANCES_OFF))
    return {cid: (kw, kind) for cid, kw, kind in opts.option_cases(p, ref, gso.N_IT)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(solver (the keywords the engine runs), kind (termination message prefix, or None), cid, res (a result in the oracle's
    shape: iterations, cams, points (xyz, or rho [n, 1]), initial_cost, final_cost, termination_type, num_successful_steps, message),
    n_clear (lm_yardstick.compared_iterations of the uncut reference)).  The inverse-depth case is cut at its clear iterations."""
    p, rays, rho = window(name)
    if name in OPTION_CASES:
        wname, cid = name.split("/")
        kw, kind = _option_cases(wname)[cid]
        kw = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in kw.items()}      # plain numbers: the keywords travel to the ranks
        res = oracle.solve(p, oracle.default_options(**kw))
        return dict(solver=kw, kind=kind, cid=cid, res=dict(res, points=res["xyz"]), n_clear=lm.compared_iterations(res))
    kw = MODE_CASES[name][3]
    if rays is None:
        res = oracle.solve(p, oracle.default_options(**kw))
        return dict(solver=kw, kind=None, cid=None, res=dict(res, points=res["xyz"]), n_clear=lm.compared_iterations(res))
    prog = RayProgram(p, constant_slots(p), rays, rho)
    full = prog.solve(**kw)
    n = lm.compared_iterations(full)
    its = full["iterations"][:n]
    cams, x = full["states"][n - 1]
    res = dict(iterations=its, cams=cams, points=x, initial_cost=full["initial_cost"], termination_type=1,
               final_cost=min(i["cost"] for i in its if i["step_is_successful"]), num_successful_steps=sum(i["step_is_successful"] for i in its),
               message="Maximum number of iterations reached.", failed=prog.failed,
               min_state=min(float(s[1].min()) for s in full["states"][:n]))
    return dict(solver=dict(max_num_iterations=n - 1), kind=None, cid=None, res=res, n_clear=n)


class RayProgram(lm.Dense):
    """lm_yardstick.Dense with Ceres' rule for a candidate that cannot be evaluated (TrustRegionMinimizer: its cost is the largest double,
    so the step is valid and rejected): a candidate with an inverse depth <= 0 would mirror its point behind the ray origin, and the
    engine flags it as an evaluation failure (include/pba.h: rho > 0).  `failed` lists the offending points of every such candidate."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.failed = []

    def cost(self, state):
        bad = np.nonzero(~(state[1][:, 0] > 0.0))[0]
        if len(bad):
            self.failed.append(bad)
            return EVAL_FAILED
        return super().cost(state)


def first_system(name):
    """(S, rhs): the scaled and damped reduced camera system of the first LM step (radius 1e4, default clamps), by explicit Schur
    elimination of the point columns of the yardstick's dense matrix."""
    p, rays, rho = window(name)
    st = lm.Dense(p, constant_slots(p), rays, rho).first_step(radius=1e4)
    return st["S"], st["rhs"]


def num_residuals(p):
    return p.n_obs * p.channels * p.patch_len
