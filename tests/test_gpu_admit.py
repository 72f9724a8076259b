"""-m gpu: pba_admit (include/pba.h "re-observation") against the rule restated in numpy (tests/admit_cases.py).

1. the candidates equal the yardstick's, in order;
2. their costs equal the CPU yardstick's block costs of the window whose observation list is the candidate list;
3. the verdict (take bytes, every info field) equals the rule bit for bit, at every capacity;
4. an applied admission leaves the engine a fresh one reaches through pba_set_problem with the merged lists, in every mode;
5. a verdict alone, or one that takes nothing, leaves the engine untouched; 6. two fresh engines give the same bytes; 7. the refusals;
8. on a window that lost a whole frame behind an occluder, what the rule takes; 9. the class and run_kitti.
Images are 120 x 160 as in the other small GPU tests."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import admit_cases as ac
import cull_cases as cc
import host_class_probe
from photobundle_amd import synthetic
from photobundle_amd.engine import Engine, EngineError, default_solver_options, solve_batch

pytestmark = pytest.mark.gpu

SMALL = dict(radius=1, size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
PBA_ERR_INVALID, PBA_ERR_STATE, PBA_ERR_NUMERIC = -1, -4, -6
TIMES = ("total_time_in_seconds", "iteration_time_in_seconds", "step_solver_time_in_seconds", "cumulative_time_in_seconds")
MARGIN_PX, MARGIN_DEPTH = 1e-6, 1e-9      # the margin condition: no tested projection / depth closer than this to a bound


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _strip(res):
    """A solve result without its wall-clock fields, floats as hex (NaN compares equal to itself)."""
    def val(v):
        if isinstance(v, float):
            return v.hex()
        if isinstance(v, np.ndarray):
            return v.tobytes()
        if isinstance(v, list):
            return [_strip(x) for x in v]
        return v
    return {k: val(v) for k, v in res.items() if k not in TIMES}


def _engine(p, slots=(0,), keep=False, **kw):
    rows, cols = p.planes.shape[-2:]
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=keep, channels=p.channels, **kw)
    for s in range(p.n_frames):
        if p.channels > 1:
            e.set_frame_channels(s, p.channel_images[s])
        else:
            e.set_frame(s, p.images[s])
    e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    e.set_cameras(p.cams, constant_slots=slots)
    return e


@pytest.fixture(scope="module")
def windows():
    base = synthetic.make_window(**ac.BASE)
    return dict(base=base, holes=ac.with_holes(base),
                causal=synthetic.make_window(n_frames=5, n_points=300, visibility="causal", **SMALL),
                wide=ac.with_holes(synthetic.make_window(n_frames=17, n_points=100, **SMALL)))


# ---- 1. the candidates -------------------------------------------------------------------------------------------------------------------
GEOMETRY = {
    "every-slot": ("holes", dict(slot_mask=0b1111, min_depth=0.1, border=1)),
    "two-slots": ("holes", dict(slot_mask=0b0110, min_depth=0.1, border=1)),
    "border-0": ("holes", dict(slot_mask=0b1111, min_depth=0.1, border=0)),
    "large-min-depth": ("holes", dict(slot_mask=0b1111, min_depth=38.02, border=1)),
    # a causal window loses its blocks where a point leaves the margin: with border 0 its candidates sit at the image edge
    "border-0-at-the-edge": ("causal", dict(slot_mask=0b11111, min_depth=0.1, border=0)),
    "border-5": ("causal", dict(slot_mask=0b11111, min_depth=0.1, border=5)),
}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_candidates_equal_the_yardstick(windows, name):
    which, kw = GEOMETRY[name]
    p = windows[which]
    want_point, want_slot, margins = ac.reference_candidates(p, p.cams, p.xyz, **kw)
    print("%s: %d candidates, margins %.3g px, %.3g depth" % (name, len(want_point), margins["px"], margins["depth"]))
    assert margins["px"] > MARGIN_PX and margins["depth"] > MARGIN_DEPTH and len(want_point) > 20
    if name == "large-min-depth":
        assert len(want_point) < len(ac.reference_candidates(p, p.cams, p.xyz, 0b1111, 0.1, 1)[0])
    if name == "border-0-at-the-edge":
        fewer = ac.reference_candidates(p, p.cams, p.xyz, kw["slot_mask"], 0.1, p.radius)[0]
        assert len(want_point) > len(fewer)      # some patches cross the image edge
    with _engine(p) as e:
        cp, cs, cost, take, info = e.admit(apply=False, **kw)
        assert cp.tobytes() == want_point.tobytes() and cs.tobytes() == want_slot.tobytes()
        assert info["n_candidates"] == info["n_written"] == len(want_point) and info["n_points"] == p.n_points
        assert info["n_blocks_before"] == p.n_obs and info["applied"] == 0
        assert np.isfinite(cost).all() and (cost >= 0).all()


# ---- 2. the costs ------------------------------------------------------------------------------------------------------------------------
COSTS = {
    "radius-1-unit-weights": dict(radius=1),
    "radius-2-gaussian-huber": dict(radius=2, gaussian=True, huber=0.05),
    "three-channels": dict(radius=1, channel_fn="IntensityAndGradient"),
}


@pytest.mark.parametrize("name", list(COSTS))
def test_candidate_costs_equal_the_yardstick(name):
    kw = dict(COSTS[name])
    if "channel_fn" in kw:
        kw["channel_fn"] = synthetic.channel_fn(kw["channel_fn"])
    p = ac.with_holes(synthetic.make_window(**dict(ac.BASE, **kw)))
    border = 0 if name == "radius-1-unit-weights" else p.radius
    want_point, want_slot, margins = ac.reference_candidates(p, p.cams, p.xyz, 0b1111, 0.1, border)
    assert margins["px"] > MARGIN_PX and margins["depth"] > MARGIN_DEPTH
    want = cc.yardstick_block_costs(ac.candidate_window(p, p.cams, p.xyz, want_point, want_slot), p.cams, p.xyz)
    with _engine(p) as e:
        cp, cs, cost, _, _ = e.admit(border=border, apply=False)
        own = e.block_costs()
    assert cp.tobytes() == want_point.tobytes() and cs.tobytes() == want_slot.tobytes()
    err = np.abs(cost - want) / np.maximum(np.abs(want), 1e-300)      # (a candidate in its point's own frame costs exactly 0 at the initial state)
    print("%s: %d candidates, largest relative difference %.3g (existing blocks: %.3g)" % (
        name, len(cost), err.max(), (np.abs(own - cc.yardstick_block_costs(p, p.cams, p.xyz)) / np.maximum(np.abs(own), 1e-300)).max()))
    np.testing.assert_allclose(cost, want, rtol=1e-12, atol=0.0)


def test_candidate_costs_are_the_block_costs_of_the_candidate_list(windows):
    """The number pba_get_block_costs reports for a block: an engine whose observation list IS the candidate list gives the same bytes."""
    p = windows["holes"]
    with _engine(p) as e:
        cp, cs, cost, _, _ = e.admit(apply=False)
    keep = np.isin(np.arange(p.n_points), cp)      # (pba_set_problem wants every point observed: the points without a candidate leave)
    remap = np.cumsum(keep) - 1
    q = dataclasses.replace(p, xyz=p.xyz[keep], desc=p.desc[keep], obs_point=remap[cp].astype(np.int32), obs_slot=cs)
    with _engine(q) as f:
        assert f.block_costs().tobytes() == cost.tobytes()


# ---- 3. the verdict ----------------------------------------------------------------------------------------------------------------------
def _assert_verdict(got, want, what):
    take, info = got
    wtake, winfo = want
    assert take.tobytes() == wtake.tobytes(), "%s: take bytes differ in %d places" % (what, int((take != wtake).sum()))
    for f, w in winfo.items():
        g = info[f]
        assert (_bits(g) == _bits(w)) if isinstance(w, float) else g == w, "%s: %s = %r, the rule gives %r" % (what, f, g, w)


def test_verdict_equals_the_rule_at_every_capacity(windows):
    p = windows["holes"]
    with _engine(p) as e:
        e.solve(default_solver_options(max_num_iterations=3))
        c = e.block_costs()
        cp, cs, cost, _, _ = e.admit(apply=False)
        n = len(cp)
        tie = float(np.sort(cost)[n // 3])
        rules = [dict(quantile=q, factor=f) for q in (0.0, 0.5, 0.9, 1.0) for f in (0.0, 0.5, 1.0, 3.0)]
        rules += [dict(min_cost=tie, factor=0.0), dict(min_cost=tie, factor=1.0, quantile=0.0), dict(min_cost=1e300, factor=0.0)]
        admitted = set()
        for rule in rules:
            gp, gs, gc, take, info = e.admit(apply=False, **rule)
            assert gp.tobytes() == cp.tobytes() and gs.tobytes() == cs.tobytes() and gc.tobytes() == cost.tobytes()
            assert info["applied"] == 0 and info["n_written"] == n and e.n_obs == p.n_obs
            _assert_verdict((take, info), ac.reference_admit(c, cost, **rule), repr(rule))
            admitted.add(info["n_admitted"])
        print("%d rules over %d candidates: between %d and %d admitted" % (len(rules), n, min(admitted), max(admitted)))
        assert len(admitted) > 5 and 0 in admitted and n in admitted      # the sweep is no row of equal verdicts
        wtake, winfo = ac.reference_admit(c, cost, **ac.DEFAULTS)
        assert 0 < winfo["n_admitted"] < n
        # a capacity below the number of candidates: a prefix, and the full counts
        for cap in (1, n // 2, n - 1, n, n + 7):
            gp, gs, gc, take, info = e.admit(apply=False, capacity=cap, **ac.DEFAULTS)
            m = min(cap, n)
            assert info["n_written"] == m == len(gp) and gp.tobytes() == cp[:m].tobytes() and gs.tobytes() == cs[:m].tobytes()
            assert gc.tobytes() == cost[:m].tobytes() and take.tobytes() == wtake[:m].tobytes()
            assert {f: info[f] for f in winfo} == winfo
        # capacity 0 with null pointers: a count
        gp, _, _, _, info = e.admit(apply=False, capacity=0, **ac.DEFAULTS)
        assert len(gp) == 0 and info["n_written"] == 0 and {f: info[f] for f in winfo} == winfo
        assert e.block_costs().tobytes() == c.tobytes()


# ---- 4. an applied admission is pba_set_problem with the merged lists -----------------------------------------------------------------------
def _prior(p, slots=(1, 2)):
    rng = np.random.default_rng(5)
    k = len(slots)
    A = rng.standard_normal((6 * k, 6 * k))
    return dict(slots=list(slots), x0=p.cams[list(slots)] + 1e-3 * rng.standard_normal((k, 6)), Lambda=A @ A.T * 50.0 + 10.0 * np.eye(6 * k),
                eta=rng.standard_normal(6 * k), c=0.5)


MODES = {
    "full": dict(),
    "two-anchors": dict(slots=(0, 3)),
    "inverse-depth": dict(inverse_depth=True),
    "points-constant": dict(points_const=True),
    "cameras-constant": dict(cams_const=True),
    "prior": dict(prior=True),
    "wide": dict(window="wide"),
    "batch": dict(batch=True),
}


def _set_modes(e, mode, rays=None, rho=None):
    if mode.get("inverse_depth"):
        e.set_inverse_depth(rays, rho)
    if mode.get("points_const"):
        e.set_points_constant()
    if mode.get("cams_const"):
        e.set_cameras_constant()


def _measure(e, partner=None):
    """linearize cost, records, a full solve (next to an untouched engine in one batch when asked)."""
    cost = e.linearize()
    rec = e.obs_records()
    o = default_solver_options(max_num_iterations=6)
    res = solve_batch([e, partner], o)[0] if partner is not None else e.solve(o)
    return cost.hex(), rec.tobytes(), _strip(res)


@pytest.mark.parametrize("name", list(MODES))
def test_applied_admission_equals_set_problem_with_the_merged_lists(windows, name):
    mode = MODES[name]
    p = windows[mode.get("window", "holes")]
    slots = mode.get("slots", (0,))
    rays, rho = synthetic.inverse_depth_rays(p) if mode.get("inverse_depth") else (None, None)
    prior = _prior(p) if mode.get("prior") else None
    with _engine(p, slots) as E:
        _set_modes(E, mode, rays, rho)
        if prior:
            E.set_camera_prior(**prior)
        E.solve(default_solver_options(max_num_iterations=3))
        cams, x = E.get_state()
        # the candidates are the yardstick's at this state too
        want_point, want_slot, margins = ac.reference_candidates(p, cams, ac.world_points(x, rays), (1 << p.n_frames) - 1, 0.1, p.radius)
        assert margins["px"] > MARGIN_PX and margins["depth"] > MARGIN_DEPTH
        c = E.block_costs()
        cp, cs, cost, take, info = E.admit(**ac.DEFAULTS)
        assert cp.tobytes() == want_point.tobytes() and cs.tobytes() == want_slot.tobytes()
        _assert_verdict((take, info), ac.reference_admit(c, cost, **ac.DEFAULTS), name)
        print("%s: %d candidates, %d admitted, %d -> %d blocks" % (name, info["n_candidates"], info["n_admitted"], p.n_obs, info["n_blocks_after"]))
        assert info["applied"] == 1 and E.n_obs == info["n_blocks_after"] == p.n_obs + info["n_admitted"] and info["n_admitted"] > 20
        assert E.counters()["n_obs"] == E.n_obs and E.counters()["n_points"] == p.n_points and p.n_obs > 3 * 128
        with pytest.raises(EngineError, match="pba_step before pba_linearize"):      # the linearisation is dropped
            E.step(1e4, init_scale=True)
        cams2, x2 = E.get_state()
        assert cams2.tobytes() == cams.tobytes() and x2.tobytes() == x.tobytes()      # the parameters, byte for byte
        if prior:      # the prior survives: the cost is the merged problem's WITH the prior
            with _engine(p, slots) as f:
                mp, ms = ac.merged_lists(p.obs_point, p.obs_slot, cp, cs, take)
                f.set_problem(x, p.desc, mp, ms, p.weights)
                f.set_cameras(cams, constant_slots=slots)
                without = f.linearize()
                f.set_camera_prior(**prior)
                assert E.linearize().hex() == f.linearize().hex() != without.hex()
        mp, ms = ac.merged_lists(p.obs_point, p.obs_slot, cp, cs, take)
        # a point whose blocks now straddle what was a boundary between two tiles of 128 observations
        first = np.searchsorted(mp, np.arange(p.n_points))
        last = np.searchsorted(mp, np.arange(p.n_points), side="right") - 1
        assert ((first // 128) != (last // 128)).any()
        rows, cols = p.planes.shape[-2:]
        with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber) as F:
            for s in range(p.n_frames):
                F.set_frame(s, p.images[s])
            F.set_problem(x, p.desc, mp, ms, p.weights)
            _set_modes(F, mode, rays, x[:, 0].copy())
            for e in (E, F):      # (accepted and set cameras differ in the last bit of dR: tests/test_gpu_state_rules.py)
                e.set_cameras(cams, constant_slots=slots)
                if prior:
                    e.set_camera_prior(**prior)
            if mode.get("batch"):
                with _engine(p) as pa, _engine(p) as pb:
                    want, got = _measure(F, pa), _measure(E, pb)
            else:
                want, got = _measure(F), _measure(E)
        for what, g, w in zip(("linearize cost", "records", "solve"), got, want):
            assert g == w, "%s: %s differs from the fresh engine's" % (name, what)


def test_solve_right_after_an_applied_admission(windows):
    """Without the cameras being set again: the solve starts from the state the admission left, and a free camera that gains its first
    blocks becomes a live column."""
    p = ac.without_frame(windows["base"], 2)
    o = default_solver_options(max_num_iterations=4)
    with _engine(p) as e:
        e.solve(o)
        cams = e.get_state()[0]
        cp, cs, _, take, info = e.admit(slot_mask=0b0100, min_cost=1e300, factor=0.0)
        # (camera 2 had no block and stayed at its initial pose: a few points project outside under it)
        assert info["applied"] == 1 and info["n_admitted"] == info["n_candidates"] == len(cs) > 0.9 * p.n_points and (cs == 2).all() and take.all()
        res = e.solve(o)
        assert res["num_residual_blocks"] == p.n_obs + info["n_admitted"]
        assert res["cams"][2].tobytes() != cams[2].tobytes() and res["cams"][0].tobytes() == cams[0].tobytes()
        # the pairs that were admitted are blocks now: they are no candidates any more
        again = e.admit(apply=False)
        assert again[4]["n_candidates"] <= p.n_points - info["n_admitted"] and not (set(zip(again[0], again[1])) & set(zip(cp, cs)))


# ---- 5. untouched ------------------------------------------------------------------------------------------------------------------------
def test_a_verdict_alone_and_a_verdict_that_takes_nothing_change_nothing(windows):
    p = windows["holes"]
    o3, o5 = default_solver_options(max_num_iterations=3), default_solver_options(max_num_iterations=5)
    for kw in (dict(apply=False), dict(apply=True, factor=0.0, min_cost=0.0)):
        with _engine(p) as e, _engine(p) as twin:
            for x in (e, twin):
                x.solve(o3)
                x.reset_counters()
                x.linearize()
            before = e.counters()
            _, _, _, take, info = e.admit(**kw)
            assert info["applied"] == 0 and e.n_obs == p.n_obs and info["n_candidates"] > 0
            if kw["apply"]:
                assert info["n_admitted"] == 0 and not take.any() and info["threshold"] == 0.0
            else:
                assert info["n_admitted"] > 0
            after = e.counters()
            for f in ("linearize_launches", "cost_launches", "schur_launches", "solve_launches", "n_obs", "n_points"):
                assert after[f] == before[f], f
            assert e.step(1e4, init_scale=True) == twin.step(1e4, init_scale=True)      # (the linearisation is still valid)
            assert _strip(e.solve(o5)) == _strip(twin.solve(o5))
    # without a valid linearisation the call runs one, counted as pba_covariance counts it
    with _engine(p) as e:
        e.reset_counters()
        e.admit(apply=False)
        e.linearize()                       # (a no-op on a linearised point: it collects the event timers)
        assert e.counters()["linearize_launches"] == 1
        e.admit(apply=False)
        e.linearize()
        assert e.counters()["linearize_launches"] == 1


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_fresh_engines_give_the_same_bytes(windows):
    p = windows["holes"]
    out = []
    for _ in range(2):
        with _engine(p) as e:
            cp, cs, cost, take, info = e.admit(**ac.DEFAULTS)       # (no linearisation yet: the call runs it)
            out.append((cp.tobytes(), cs.tobytes(), cost.tobytes(), take.tobytes(), info, e.linearize().hex(), e.obs_records().tobytes()))
    assert out[0] == out[1] and out[0][4]["applied"] == 1


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(windows):
    p = windows["holes"]
    o = default_solver_options(max_num_iterations=4)
    with _engine(p) as plain:
        want = _strip(plain.solve(o))

    def refused(e, match, status=PBA_ERR_INVALID, **kw):
        with pytest.raises(EngineError, match=match) as ei:
            e.admit(**kw)
        assert ei.value.status == status
        return ei.value

    with _engine(p) as e:
        for kw, match in ((dict(min_depth=0.0), "min_depth"), (dict(min_depth=-1.0), "min_depth"), (dict(min_depth=float("nan")), "min_depth"),
                          (dict(min_depth=float("inf")), "min_depth"), (dict(border=-1), "border"),
                          (dict(min_cost=-1.0), "min_cost"), (dict(min_cost=float("nan")), "min_cost"), (dict(min_cost=float("inf")), "min_cost"),
                          (dict(factor=-0.5), "factor"), (dict(factor=float("inf")), "factor"), (dict(quantile=1.5), "quantile"),
                          (dict(quantile=-0.1), "quantile"), (dict(quantile=float("nan")), "quantile"), (dict(capacity=-1), "capacity"),
                          (dict(slot_mask=0), "slot_mask is empty"), (dict(slot_mask=0b10000), "at or above n_frames"),
                          (dict(slot_mask=0b10011), "at or above n_frames")):
            refused(e, match, **kw)
        # factor * quantile_cost overflows
        err = refused(e, "not finite", status=PBA_ERR_NUMERIC, factor=1e308, quantile=1.0)
        assert err.info["n_blocks_before"] == p.n_obs and err.info["applied"] == 0 and np.isinf(err.info["threshold"]) and err.info["n_candidates"] > 0
        assert e.n_obs == p.n_obs
        assert _strip(e.solve(o)) == want
    # a slot without a frame: five slots, cameras for five, frames (and blocks) in four
    rows, cols = p.planes.shape[-2:]
    with Engine(rows, cols, p.K, p.radius, 5, huber=p.huber) as e:
        for s in range(4):
            e.set_frame(s, p.images[s])
        e.set_problem(p.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
        e.set_cameras(np.concatenate([p.cams, p.cams[-1:]]), constant_slots=(0,))
        refused(e, "slot 4 of slot_mask holds no frame", slot_mask=0b11111)
        assert e.admit(slot_mask=0b01111, apply=False)[4]["n_candidates"] > 0
    with _engine(p, precision="fp32") as e:
        refused(e, "precision-sweep")
    with _engine(p) as e, _engine(p) as twin:
        for x in (e, twin):
            x.comm_init_callback(lambda v, op: None, 0, 2)
        refused(e, "multi-rank")
        assert _strip(e.solve(o)) == _strip(twin.solve(o))
    with Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber) as e:
        e.n_frames = p.n_frames
        refused(e, "call order violated", status=PBA_ERR_STATE)


# ---- 8. it finds what was lost and leaves what is wrong --------------------------------------------------------------------------------------
def test_after_an_occluder_took_a_whole_frame():
    """cull_cases.occluded_window with every block of OCCLUDER_FRAME removed, solved, then pba_admit with the class defaults.

    On the CPU yardstick (solve with the oracle's defaults, the rule over the yardstick's block costs): 1199 candidates, 168 taken; of
    the 328 candidates inside the rectangle 0 % are taken, of the 871 outside it 19.3 %.  Inside the occluded FRAME nothing is taken on
    either side of the rectangle's edge (0 of 591): the frame has no block left, so the solve never refines its camera, its patches land
    beside their place under the initial pose and cost far more than the median of the converged blocks.  What is taken lies in the other
    frames.  The defaults are not tuned to change that."""
    clean, dirty, inside = cc.occluded_window(synthetic.make_window, dataclasses.replace)
    p = ac.without_frame(dirty, cc.OCCLUDER_FRAME)
    B, min_depth = max(1, max(2, p.radius)), 0.01      # the class defaults: addFrame's border, Options::minValidDepth
    with _engine(p) as e:
        e.solve()
        cams, x = e.get_state()
        want_point, want_slot, margins = ac.reference_candidates(p, cams, x, (1 << p.n_frames) - 1, min_depth, B)
        assert margins["px"] > MARGIN_PX and margins["depth"] > MARGIN_DEPTH
        c = e.block_costs()
        cp, cs, cost, take, info = e.admit(min_depth=min_depth, border=B, apply=False, **ac.DEFAULTS)
    assert cp.tobytes() == want_point.tobytes() and cs.tobytes() == want_slot.tobytes()
    _assert_verdict((take, info), ac.reference_admit(c, cost, **ac.DEFAULTS), "occluder")
    in_rect = {(int(a), int(b)) for a, b, i in zip(dirty.obs_point, dirty.obs_slot, inside) if i}
    is_in = np.array([(int(a), int(b)) in in_rect for a, b in zip(cp, cs)])
    frame = cs == cc.OCCLUDER_FRAME
    print("occluder: %d candidates, %d taken; inside the rectangle %d taken of %d, outside %d of %d (outside, in the occluded frame: %d of %d)"
          % (len(cp), int(take.sum()), int(take[is_in].sum()), int(is_in.sum()), int(take[~is_in].sum()), int((~is_in).sum()),
             int(take[frame & ~is_in].sum()), int((frame & ~is_in).sum())))
    assert is_in.sum() > 100 and (~is_in).sum() > 100
    assert take[~is_in].mean() > take[is_in].mean()


# ---- 9. the class ------------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")
SEQ = dict(n_frames=6, window=4, occluded_frame=2)


@pytest.fixture(scope="module")
def occluder_sequence():
    """The sequence of tests/test_gpu_cull.py: six photo-consistent 120 x 160 frames with exact depth and perturbed initial poses, the
    rectangle of cull_cases over frame 2."""
    size, K = SMALL["size"], SMALL["K"]
    imgs, depths, T_gt, _ = host_class_probe.sequence(SEQ["n_frames"], size, K)
    local, _ = synthetic.perturb_local_poses(T_gt, rot_deg=0.03, trans=0.005)
    r0, r1, c0, c1 = cc.OCCLUDER_RECT
    imgs = [im.copy() for im in imgs]
    imgs[SEQ["occluded_frame"]][r0:r1, c0:c1] = cc.occluder_patch((r1 - r0, c1 - c0), (r0, c0))
    return imgs, depths, T_gt, local


def test_the_class_admits_and_keeps_its_visibility_lists_in_order(tmp_path, occluder_sequence):
    import admit_class_probe
    imgs, depths, _, local = occluder_sequence
    probe = admit_class_probe.AdmitClassProbe(tmp_path)
    try:
        assert probe.defaults() == ((0.0, 1.0, 0.5, 0.0), 0)
        with pytest.raises(RuntimeError, match="reobservePasses = -1 is negative"):
            probe.create(SMALL["size"], SMALL["K"], window=SEQ["window"], radius=1, passes=-1)
        ran = {}
        for passes in (0, 1):
            probe.create(SMALL["size"], SMALL["K"], window=SEQ["window"], radius=1, min_score=0.65, passes=passes)
            ran[passes] = []
            for im, z, T in zip(imgs[:5], depths[:5], local[:5]):
                r = probe.add(im, z, T)
                if r is not None:
                    r["lists"] = probe.visibility()      # as they stand after this call: what admittedBlocks indexes
                ran[passes].append(r)
            if passes == 0:
                assert all(r is None or (r["admitted_blocks"] == 0 and len(r["admitted"]) == 0) for r in ran[0])
        assert [r is not None for r in ran[1]] == [False, False, False, True, True]
        first, second = ran[1][3], ran[1][4]
        print("admitted blocks per window: %d, %d (residuals %d, %d; without the pass %d, %d)" % (
            first["admitted_blocks"], second["admitted_blocks"], first["residuals"], second["residuals"], ran[0][3]["residuals"], ran[0][4]["residuals"]))
        assert first["admitted_blocks"] > 0 and first["initial_cost"] == ran[0][3]["initial_cost"]
        assert first["residuals"] > ran[0][3]["residuals"]      # the last solve carried the admitted blocks
        assert len(first["admitted"]) + len(second["admitted"]) > 0
        for r, lo, hi in ((first, 0, 3), (second, 1, 4)):
            assert len(r["admitted"]) <= r["admitted_blocks"]      # (the points of the window's oldest frame have left)
            for pos, frame in r["admitted"]:
                f = r["lists"][pos]
                assert lo <= frame <= hi and frame in f, (pos, frame, f)
            assert all((np.diff(f) > 0).all() for f in r["lists"])      # every list ascending, no frame twice
        with pytest.raises(RuntimeError, match="addFrames: Options::reobservePasses solves alone"):
            probe.add_frames(imgs[5], depths[5], local[5])
    finally:
        probe.release()


def _run_kitti(tmp, seq, extra):
    imgs, depths, _, local = seq
    os.makedirs(tmp)
    host_class_probe.write_sequence(tmp, imgs, depths, SMALL["K"], local)
    cfg = os.path.join(tmp, "test.cfg")
    with open(cfg, "w") as f:
        f.write("DataDirectory = %s\nTrajectory = %s/init.txt\nmaxNumPoints = 4096\nslidingWindowSize = %d\npatchRadius = 1\nminScore = 0.65\n"
                "robustThreshold = 0.05\nverbose = 0\n%s" % (tmp, tmp, SEQ["window"], extra))
    r = subprocess.run([RUN, "-c", cfg, "-o", os.path.join(tmp, "refined.txt"), "-r", os.path.join(tmp, "results.txt"), "-p"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(tmp, "refined.txt")).read(), open(os.path.join(tmp, "results.txt")).read(), r.stdout


def test_run_kitti_with_the_config_key(tmp_path, occluder_sequence):
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    # reobservePasses = 0 is the class without the keys, byte for byte
    absent = _run_kitti(str(tmp_path / "absent"), occluder_sequence, "")
    zero = _run_kitti(str(tmp_path / "zero"), occluder_sequence, "reobservePasses = 0\nreobserveFactor = 2\nreobserveQuantile = 0.9\n")
    assert absent == zero and "admitted" not in absent[1]
    one = _run_kitti(str(tmp_path / "one"), occluder_sequence, "reobservePasses = 1\n")
    admitted = [int(m.group(1)) for m in re.finditer(r"^admitted blocks (\d+)$", one[1], re.M)]
    print("admitted blocks per window: %s" % (admitted,))
    assert len(admitted) == SEQ["n_frames"] - SEQ["window"] + 1 and admitted[0] > 0
    assert len(one[0].splitlines()) == len(absent[0].splitlines()) == SEQ["n_frames"] and one[0] != absent[0]
    # ... and together with the outlier passes: the cull comes second and judges the admitted blocks too
    both = _run_kitti(str(tmp_path / "both"), occluder_sequence, "reobservePasses = 1\noutlierPasses = 1\n")
    assert len(re.findall(r"^admitted blocks \d+$", both[1], re.M)) == len(re.findall(r"^culled blocks \d+ points \d+$", both[1], re.M)) == len(admitted)
