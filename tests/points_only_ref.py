"""Yardstick of the structure-only mode (pba_set_cameras_constant): a numpy Levenberg-Marquardt over the POINT columns only, written from
Ceres' documented rules for the reduced program (TrustRegionMinimizer + LevenbergMarquardtStrategy), the twin of pose_only_ref.py:

  program        parameter blocks = the points (every one has a residual block); every camera is constant, every residual block depends
                 on a point, so none leaves the program: fixed_cost = 0, the counts are those of the whole problem
  scaling        1 / (1 + sqrt(diag J^T J)) per point column, fixed at iteration 0
  damping        clip(diag of the scaled J^T J, min_lm_diagonal, max_lm_diagonal) / radius
  step           exact solve of the block-diagonal normal equations (one 3 x 3 block per point; 1 x 1 with inverse depths), model cost
                 change -m^T (r + m / 2); a block that is not positive definite fails the whole step
  decision       relative decrease > min_relative_decrease; radius / max(1/3, 1 - (2 rho - 1)^3) on success, / 2, / 4, ... on failure
  termination    gradient tolerance after a successful step; parameter and function tolerance on the candidate (the solve ends without
                 logging that iteration); iteration limit; minimum radius

Evaluations come from the unchanged oracle (oracle.linearize's V, grad_pts, block_sqnorm).  With inverse depths the parameter of point i
is rho_i on the fixed world ray (o_i, d_i), X_i = o_i + d_i / rho_i, and the oracle's world-point blocks go through the chain rule
dX / drho = -d / rho^2.  Shares no code with the engine."""
import numpy as np

from oracle import oracle

DEFAULTS = dict(max_num_iterations=500, function_tolerance=1e-6, gradient_tolerance=1e-6, parameter_tolerance=1e-6,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_num_consecutive_invalid_steps=5)


def block_costs(p, sq):
    a = p.huber
    rho = np.where((a > 0) & (sq > a * a), 2 * a * np.sqrt(sq) - a * a, sq)
    return 0.5 * rho


def initial_parameters(p, rays=None, rho=None):
    """The parameter array [n_points, d]: the world points (d = 3), or the inverse depths (d = 1)."""
    return np.array(p.xyz, np.float64) if rays is None else np.array(rho, np.float64).reshape(-1, 1)


def world_points(x, rays=None):
    return x if rays is None else rays[:, :3] + rays[:, 3:] / x


def evaluate(p, x, rays=None, blocks=True, autodiff=True):
    """(cost, V [n, d, d], g [n, d]) at the parameters x with the cameras as they are."""
    lin = oracle.linearize(p, autodiff=autodiff, cams=p.cams, xyz=world_points(x, rays), blocks=blocks)
    cost = float(block_costs(p, lin["block_sqnorm"]).sum())
    V, g = lin.get("V"), lin["grad_pts"]
    if rays is not None:
        q = -rays[:, 3:] / (x * x)                                   # dX / drho
        g = np.einsum("ni,ni->n", q, g)[:, None]
        if V is not None:
            V = np.einsum("ni,nij,nj->n", q, V, q)[:, None, None]
    return cost, V, g


def _step(V, g, scale, radius, min_diag, max_diag):
    d = g.shape[1]
    Vs = V * scale[:, :, None] * scale[:, None, :]
    gs = g * scale
    D2 = np.clip(np.einsum("kii->ki", Vs), min_diag, max_diag) / radius
    S = Vs + np.einsum("ki,ij->kij", D2, np.eye(d))
    y = np.zeros_like(gs)
    try:
        L = np.linalg.cholesky(S)
        for k in range(len(S)):
            y[k] = np.linalg.solve(L[k].T, np.linalg.solve(L[k], gs[k]))
        ok = bool(np.all(np.isfinite(y)))
    except np.linalg.LinAlgError:
        ok = False
    if not ok:
        y[:] = 0.0               # a failed block fails the linear solver: the step is zero everywhere
    # -m^T (r + m / 2) with m = J step, step = -y:  y^T gs - y^T Vs y / 2
    mcc = float(np.sum(y * gs) - 0.5 * np.einsum("ki,kij,kj->", y, Vs, y))
    return dict(S=S, rhs=gs, delta=-y * scale, model_cost_change=mcc, linear_solver_ok=ok)


def first_step(p, radius=1e4, rays=None, rho=None, min_diag=1e-6, max_diag=1e32, autodiff=True):
    """The first LM step: dict(x, scale, S [n, d, d] (scaled + damped blocks), rhs [n, d], delta [n, d], model_cost_change,
    gradient [n, d], cost)."""
    x = initial_parameters(p, rays, rho)
    cost, V, g = evaluate(p, x, rays, autodiff=autodiff)
    scale = 1.0 / (1.0 + np.sqrt(np.einsum("kii->ki", V)))
    return dict(_step(V, g, scale, radius, min_diag, max_diag), x=x, scale=scale, gradient=g, cost=cost)


def solve(p, rays=None, rho=None, autodiff=True, **options):
    """Runs the loop.  Returns dict(iterations=[dict], states=[parameters after every logged iteration], x, xyz (world points),
    initial_cost, final_cost, fixed_cost, num_residual_blocks, message)."""
    o = dict(DEFAULTS)
    for k in options:
        if k not in o:
            raise KeyError(k)
    o.update(options)
    x = initial_parameters(p, rays, rho)

    def lin(v):
        return evaluate(p, v, rays, autodiff=autodiff)

    cost, V, g = lin(x)
    scale = 1.0 / (1.0 + np.sqrt(np.einsum("kii->ki", V)))
    radius, dec = o["initial_trust_region_radius"], 2.0
    its = [dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()),
                gradient_norm=float(np.linalg.norm(g)), step_norm=0.0, relative_decrease=0.0, trust_region_radius=radius,
                model_cost_change=0.0)]
    states = [x.copy()]
    minimum_cost, invalid, message = cost, 0, None
    min_candidate = float(x.min())       # smallest parameter of any evaluated point (inverse depths must stay positive)
    while message is None:
        last = its[-1]
        if last["iteration"] >= o["max_num_iterations"]:
            message = "Maximum number of iterations reached."
            break
        if last["step_is_successful"] and last["gradient_max_norm"] <= o["gradient_tolerance"]:
            message = "Gradient tolerance reached."
            break
        if radius <= o["min_trust_region_radius"]:
            message = "Minimum trust region radius reached."
            break
        it = dict(iteration=last["iteration"] + 1, step_is_valid=0, step_is_successful=0, cost=cost, cost_change=0.0,
                  gradient_max_norm=last["gradient_max_norm"], gradient_norm=last["gradient_norm"], step_norm=0.0, relative_decrease=0.0,
                  trust_region_radius=radius, model_cost_change=0.0)
        st = _step(V, g, scale, radius, o["min_lm_diagonal"], o["max_lm_diagonal"])
        it["model_cost_change"] = st["model_cost_change"]
        if not (st["linear_solver_ok"] and st["model_cost_change"] > 0.0):
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                message = "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps."
                its.append(it); states.append(x.copy())
                break
            radius /= dec
            dec *= 2.0
            it["trust_region_radius"] = radius
            its.append(it); states.append(x.copy())
            continue
        invalid = 0
        it["step_is_valid"] = 1
        cand = x + st["delta"]
        it["step_norm"] = float(np.linalg.norm(st["delta"]))
        x_norm = float(np.linalg.norm(x))
        if it["step_norm"] <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            message = "Parameter tolerance reached."
            break
        it["min_candidate"] = float(cand.min())
        min_candidate = min(min_candidate, float(cand.min()))
        cand_cost, _, _ = evaluate(p, cand, rays, blocks=False, autodiff=autodiff)
        it["cost_change"] = cost - cand_cost
        if abs(it["cost_change"]) <= o["function_tolerance"] * cost:
            message = "Function tolerance reached."
            break
        rd = it["cost_change"] / st["model_cost_change"]
        it["relative_decrease"] = rd
        if rd > o["min_relative_decrease"]:
            x = cand
            cost, V, g = lin(x)
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rd - 1.0) ** 3))
            dec = 2.0
            it.update(step_is_successful=1, cost=cost, gradient_max_norm=float(np.abs(g).max()), gradient_norm=float(np.linalg.norm(g)))
            minimum_cost = min(minimum_cost, cost)
        else:
            radius /= dec
            dec *= 2.0
            it["cost"] = cand_cost       # Ceres >= 1.12 logs the candidate's cost for a rejected step
        it["trust_region_radius"] = radius
        its.append(it); states.append(x.copy())
    return dict(iterations=its, states=states, x=x, xyz=world_points(x, rays), initial_cost=its[0]["cost"], final_cost=minimum_cost,
                fixed_cost=0.0, num_residual_blocks=int(p.n_obs), message=message, min_candidate=min_candidate, inverse_depth=rays is not None)


def compared_iterations(res, min_relative_decrease=1e-3, function_tolerance=1e-6):
    """Number of leading iterations whose decisions are clear: up to (not including) the first one whose relative decrease is within
    1e-2 of min_relative_decrease or whose |cost_change| / cost is within 10 x of function_tolerance (near the minimum the
    objective is piecewise bilinear and decisions hinge on the last bits)."""
    n = 1
    for it in res["iterations"][1:]:
        prev_cost = it["cost"] + it["cost_change"]       # (a rejected step logs the candidate's cost)
        denom = max(abs(prev_cost), 1e-300)
        if it["step_is_valid"]:
            if abs(it["relative_decrease"] - min_relative_decrease) <= 1e-2:
                break
            if abs(it["cost_change"]) / denom <= 10.0 * function_tolerance:
                break
        n += 1
    return n


# ---- the windows of the device tests: cameras at the ground truth, points as make_window leaves them (1 % depth noise) -----------------
_SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
_LONG = dict(size=(120, 200), K=(250.0, 250.0, 100.0, 60.0))
TRACE_CASES = {
    # name: (make_window arguments, extras)
    "3-frames-r1-huber": (dict(n_frames=3, n_points=200, radius=1, huber=0.05, seed_offset=1, **_SMALL), ()),
    "5-frames-r2": (dict(n_frames=5, n_points=200, radius=2, seed_offset=2, **_SMALL), ()),
    "8-frames-r1-huber-causal": (dict(n_frames=8, n_points=200, radius=1, huber=0.05, visibility="causal", seed_offset=3, **_LONG), ()),
    "20-frames-r1-causal": (dict(n_frames=20, n_points=150, radius=1, visibility="causal", seed_offset=2, **_SMALL), ("one-and-all",)),
    "4-frames-r2-gaussian-huber": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, gaussian=True, seed_offset=4, **_SMALL), ()),
    "4-frames-r1-3-channels": (dict(n_frames=4, n_points=150, radius=1, seed_offset=5, **_SMALL), ("channels3",)),
    # (seed 4: every candidate of the 12 iterations keeps its inverse depths positive, min 0.011.  With seeds 7..12 the first steps send
    # some of them below zero -- a point behind every camera, outside the parameterisation's domain, where the oracle returns some finite
    # cost and the device's sampler a failed evaluation -- and with seed 3 the ninth does; test_points_only_cpu.py asserts the domain)
    "4-frames-r2-inverse-depth": (dict(n_frames=4, n_points=200, radius=2, seed_offset=4, **_SMALL), ("inverse-depth",)),
    "single-observation-5-frames-r1": (None, ("single-observation",)),
}
REF_ITERATIONS = 12      # iteration limit of the yardstick in the trace tests (the device runs the compared ones)
BOUNDARY_WINDOW = dict(n_frames=4, n_points=700, radius=1, seed_offset=8, **_SMALL)      # the 700-point window of the system test
BOUNDARY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 700)       # one fewer than, exactly and one more than a wave / a 256-thread workgroup


def cameras_to_ground_truth(p):
    p.cams = np.array(p.meta["cams_gt"], dtype=np.float64)
    return p


def first_points(p, k):
    """The problem of the first k points of p (their observations are the first ones of the list)."""
    from photobundle_amd.problem import WindowProblem
    keep = np.asarray(p.obs_point) < k
    return WindowProblem(K=p.K, radius=p.radius, planes=p.planes, cams=p.cams, xyz=p.xyz[:k].copy(), desc=p.desc[:k],
                         obs_point=p.obs_point[keep].astype(np.int32), obs_slot=p.obs_slot[keep].astype(np.int32), weights=p.weights,
                         huber=p.huber, fixed_slot=p.fixed_slot, images=p.images, meta=p.meta, channels=p.channels,
                         channel_images=p.channel_images)


def trace_case(name):
    """(problem, extras, rays, rho) of a trace case; rays / rho are None but for "inverse-depth" (what the engine is given too).
    "one-and-all": the first point seen by fewer than all frames keeps its first observation only, and the window must hold a point
    seen by every frame; "single-observation": the tracking problem of pose_only_ref (one residual block per point: every V has rank 2
    and only the damping makes the block solvable)."""
    from photobundle_amd import synthetic
    kw, extras = TRACE_CASES[name]
    if "single-observation" in extras:
        import pose_only_ref
        p = pose_only_ref.tracking_problem(pose_only_ref.tracking_window(sorted(pose_only_ref.TRACKING_SHAPES)[0]), "velocity")
        cameras_to_ground_truth(p)
        assert p.n_obs == p.n_points
        return p, extras, None, None
    if "channels3" in extras:
        kw = dict(kw, channel_fn=synthetic.channel_fn("IntensityAndGradient"))
    p = cameras_to_ground_truth(synthetic.make_window(**kw))
    if "one-and-all" in extras:
        count = np.bincount(p.obs_point, minlength=p.n_points)
        assert count.max() == p.n_frames, "the window must hold a point seen by every frame"
        victim = int(np.nonzero(count < p.n_frames)[0][0])
        first = int(np.searchsorted(p.obs_point, victim))
        keep = (np.asarray(p.obs_point) != victim) | (np.arange(p.n_obs) == first)
        p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
        count = np.bincount(p.obs_point, minlength=p.n_points)
        assert count.min() == 1 and count.max() == p.n_frames
    rays = rho = None
    if "inverse-depth" in extras:
        rays, rho = synthetic.inverse_depth_rays(p)
    return p, extras, rays, rho
