"""The cases of tests/multirank_cases.py are what they claim to be, and what every exchanged scalar of a multi-rank step SHOULD be.

No engine code runs here.  Per case: the shards tile the point range and none is empty; the cases that name an edge (a rank without
a block of a free camera, less than one 128-observation tile on every rank) have it; the oracle's linearisation of the shards sums
(or maximises) to the full window's for everything pba_lm_rules.h reduces across ranks -- cost, camera gradient and U (the packed
all-reduce), sum |g_p|^2 (kGnorm2Pts), max |g_p| (kGmaxPts), sum xyz^2 or sum rho^2 (kX2Pts) -- at 1e-12 relative, the bar of
tests/test_multirank_cpu.py; and the reference trace has the shape the GPU test relies on.  The last group is about the inputs: a
case that fails one gets another seed or size in multirank_cases.py, the condition stays."""
import numpy as np
import pytest

from oracle import oracle

import lm_yardstick as lm
import multirank_cases as mc
import test_oracle_solver_options as opts


@pytest.mark.parametrize("name", mc.NAMES)
def test_shards_tile_the_points_and_hold_the_named_edge(name):
    p, rays, rho = mc.window(name)
    world, mode = mc.world_of(name), mc.mode_of(name)
    assert world in mc.WORLDS
    shards = [mc.shard(name, r) for r in range(world)]
    ranges = [sh.meta["point_range"] for sh, _, _ in shards]
    assert ranges[0][0] == 0 and ranges[-1][1] == p.n_points
    assert all(a[1] == b[0] for a, b in zip(ranges[:-1], ranges[1:]))
    assert all(sh.n_points > 0 and sh.n_obs > 0 for sh, _, _ in shards)
    assert sum(sh.n_points for sh, _, _ in shards) == p.n_points and sum(sh.n_obs for sh, _, _ in shards) == p.n_obs
    assert np.array_equal(np.concatenate([sh.xyz for sh, _, _ in shards]), p.xyz)
    for sh, r, q in shards:
        assert sh.fixed_slot == p.fixed_slot and np.array_equal(sh.cams, p.cams)
        assert (r is None) == (rays is None)
        if rays is not None:
            lo, hi = sh.meta["point_range"]
            assert np.array_equal(r, rays[lo:hi]) and np.array_equal(q, rho[lo:hi]) and (q > 0).all()
            assert np.abs(r[:, :3] + r[:, 3:] / q[:, None] - sh.xyz).max() <= 1e-9
    free = set(range(p.n_frames)) - set(mc.constant_slots(p))
    if mode.get("misses_free_slot"):
        assert any(free - set(sh.obs_slot.tolist()) for sh, _, _ in shards)
    if mode.get("sub_tile"):
        assert all(sh.n_obs < mc.TILE for sh, _, _ in shards)
    if "fixed_slot" in mode:
        assert p.fixed_slot == mode["fixed_slot"] and len(free) == p.n_frames - (1 if p.fixed_slot >= 0 else 0)
    if "channels" in mode:
        assert p.channels == {"IntensityAndGradient": 3, "BitPlanes": 8}[mode["channels"]]
        assert p.desc.shape[1] == p.channels * p.patch_len
    assert mc.num_residuals(p) == p.n_obs * p.channels * (2 * p.radius + 1) ** 2


def test_the_stated_shards_of_the_three_rank_cases():
    """The figures the cases were chosen for."""
    sh = [mc.shard("r1-gauss-huber-causal-w3", r)[0] for r in range(3)]
    assert [(s.n_points, s.n_obs) for s in sh] == [(59, 349), (77, 356), (104, 354)]
    assert sorted(set(sh[2].obs_slot.tolist())) == [2, 3, 4, 5]          # no block of the constant slot 0, none of the free slot 1
    sh = [mc.shard("r2-causal-70-w3", r)[0] for r in range(3)]
    assert [s.n_points for s in sh] == [18, 22, 30] and 0 not in set(sh[2].obs_slot.tolist())
    sh = [mc.shard("r3-dense-w2", r)[0] for r in range(2)]
    assert [(s.n_points, s.n_obs) for s in sh] == [(65, 195), (65, 195)]


def _point_gradient(lin, rays, rho):
    """The gradient of the point parameters: world points, or inverse depths through dX / drho = -d / rho^2."""
    g = lin["grad_pts"]
    if rays is None:
        return g
    return np.einsum("ni,ni->n", -rays[:, 3:] / (rho * rho)[:, None], g)[:, None]


@pytest.mark.parametrize("name", mc.NAMES)
def test_per_rank_quantities_reduce_to_the_full_window(name):
    p, rays, rho = mc.window(name)
    world = mc.world_of(name)
    full = oracle.linearize(p)
    g_full = _point_gradient(full, rays, rho)
    parts = []
    for r in range(world):
        sh, rays_r, rho_r = mc.shard(name, r)
        lin = oracle.linearize(sh)
        g = _point_gradient(lin, rays_r, rho_r)
        x = sh.xyz if rays_r is None else rho_r
        parts.append(dict(cost=lin["cost"], grad_cams=lin["grad_cams"], U=lin["U"], g2=float((g * g).sum()), gmax=float(np.abs(g).max()),
                          x2=float((x * x).sum()), V=lin["V"]))

    def close(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.abs(a - b).max() <= 1e-12 * np.abs(b).max()

    assert close(sum(q["cost"] for q in parts), full["cost"])
    assert close(sum(q["grad_cams"] for q in parts), full["grad_cams"])
    assert close(sum(q["U"] for q in parts), full["U"])
    assert close(sum(q["g2"] for q in parts), (g_full * g_full).sum())
    assert max(q["gmax"] for q in parts) == np.abs(g_full).max()
    x_full = p.xyz if rays is None else rho
    assert close(sum(q["x2"] for q in parts), (x_full * x_full).sum())
    assert np.array_equal(np.concatenate([q["V"] for q in parts]), full["V"])      # point blocks never leave their rank
    # a rank that misses a camera contributes exact zeros to its column: the column exists only after the exchange
    for r, q in enumerate(parts):
        missing = sorted(set(range(p.n_frames)) - set(mc.shard(name, r)[0].obs_slot.tolist()))
        assert not q["U"][missing].any() and not q["grad_cams"][missing].any()


@pytest.mark.parametrize("name", mc.NAMES)
def test_reference_trace_has_the_shape_the_gpu_test_relies_on(name):
    ref = mc.reference(name)
    res, its = ref["res"], ref["res"]["iterations"]
    if name in mc.OPTION_CASES:
        opts.check_case_shape(ref["cid"], res, ref["kind"], ref["solver"]["max_num_iterations"])
        return
    # fixed length: it ends on the iteration limit with at least four clear iterations
    assert res["message"].startswith(opts.MAX_IT) and len(its) == ref["solver"]["max_num_iterations"] + 1
    assert ref["n_clear"] >= 4 and len(its) >= 4
    if mc.mode_of(name).get("rejects"):
        assert any(i["step_is_valid"] and not i["step_is_successful"] for i in its[1:])
        radii = [i["trust_region_radius"] for i in its]
        assert any(b < a for a, b in zip(radii[:-1], radii[1:]))
    if mc.mode_of(name).get("inverse_depth"):
        # every accepted state stays in front of the cameras; a candidate that does not is an evaluation failure (multirank_cases.RayProgram)
        assert res["min_state"] > 0.0 and res["points"].shape == (mc.window(name)[0].n_points, 1)
        failed_entries = [i for i in its if i["cost"] == mc.EVAL_FAILED]
        assert len(failed_entries) == len(res["failed"]) and all(i["step_is_valid"] and not i["step_is_successful"] for i in failed_entries)
        if mc.mode_of(name).get("eval_failure_on_one_rank"):
            ranges = [mc.shard(name, r)[0].meta["point_range"] for r in range(mc.world_of(name))]
            owners = [{k for k, (lo, hi) in enumerate(ranges) for j in bad if lo <= j < hi} for bad in res["failed"]]
            assert owners and all(len(o) == 1 for o in owners), owners
            assert sum(i["step_is_successful"] for i in its[1:]) >= 1
        else:
            assert not res["failed"] and sum(i["step_is_successful"] for i in its[1:]) >= 4


def test_every_permitted_mode_has_a_case():
    """The modes pba_mode_rules.h does not refuse next to a multi-rank transport, and the worlds and constant slots never run before."""
    modes = [mc.mode_of(n) for n in mc.MODE_CASES]
    kws = [mc.MODE_CASES[n][0] for n in mc.MODE_CASES]
    assert any(m.get("inverse_depth") for m in modes)
    assert {m["channels"] for m in modes if "channels" in m} == {"IntensityAndGradient", "BitPlanes"}
    assert any(k.get("huber", 0.0) > 0.0 for k in kws) and any(k.get("gaussian") for k in kws)
    assert {k["radius"] for k in kws} >= {1, 2, 3}
    assert {m["fixed_slot"] for m in modes if "fixed_slot" in m} == {2, -1}
    assert {mc.world_of(n) for n in mc.NAMES} == {2, 3}          # 3: not a power of two
    ends = {mc.reference(n)["kind"] for n in mc.OPTION_CASES}
    assert ends >= {opts.PARAM, opts.FUNC, opts.MIN_RADIUS, opts.MAX_IT}
