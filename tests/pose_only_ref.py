"""Yardstick of the pose-only mode (pba_set_points_constant): a numpy Levenberg-Marquardt over the CAMERA columns only, written from
Ceres' documented rules for the reduced program (TrustRegionMinimizer + LevenbergMarquardtStrategy, as
test_oracle_solver.py::test_lm_trace_matches_an_independent_dense_loop restates them for the full problem):

  program        parameter blocks = the free cameras that have at least one residual block; the residual blocks of the constant camera
                 leave the program, their loss-corrected cost is `fixed_cost` (in initial_cost / final_cost, not in the iterations)
  scaling        1 / (1 + sqrt(diag J^T J)) per camera column, fixed at iteration 0
  damping        clip(diag of the scaled J^T J, min_lm_diagonal, max_lm_diagonal) / radius
  step           exact solve of the block-diagonal normal equations (one 6 x 6 block per camera), model cost change -m^T (r + m / 2)
  decision       relative decrease > min_relative_decrease; radius / max(1/3, 1 - (2 rho - 1)^3) on success, / 2, / 4, ... on failure
  termination    gradient tolerance after a successful step; parameter and function tolerance on the candidate (the solve ends without
                 logging that iteration); iteration limit; minimum radius

Evaluations come from the unchanged oracle (oracle.linearize's U, grad_cams, block_sqnorm).  Shares no code with the engine."""
import numpy as np

from oracle import oracle

DEFAULTS = dict(max_num_iterations=500, function_tolerance=1e-6, gradient_tolerance=1e-6, parameter_tolerance=1e-6,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_num_consecutive_invalid_steps=5)


def program_cameras(p):
    """Slots of the reduced program: free and with at least one residual block."""
    used = np.unique(np.asarray(p.obs_slot))
    return [int(c) for c in used if c != p.fixed_slot]


def block_costs(p, sq):
    a = p.huber
    rho = np.where((a > 0) & (sq > a * a), 2 * a * np.sqrt(sq) - a * a, sq)
    return 0.5 * rho


def evaluate(p, cams, xyz=None, blocks=True):
    """(program cost, fixed cost, U [n_frames, 6, 6], g [n_frames, 6]) at `cams` with the points as they are."""
    lin = oracle.linearize(p, cams=cams, xyz=p.xyz if xyz is None else xyz, blocks=blocks)
    c = block_costs(p, lin["block_sqnorm"])
    fixed = np.asarray(p.obs_slot) == p.fixed_slot
    return float(c[~fixed].sum()), float(c[fixed].sum()), lin.get("U"), lin["grad_cams"]


def first_step(p, radius=1e4, cams=None, xyz=None, min_diag=1e-6, max_diag=1e32):
    """The first LM step: dict(cols (program slots), scale, S [k, 6, 6] (scaled + damped blocks), rhs [k, 6], delta [k, 6],
    model_cost_change, gradient [k, 6], cost, fixed_cost)."""
    cams = p.cams if cams is None else cams
    cols = program_cameras(p)
    cost, fixed, U, g = evaluate(p, cams, xyz)
    U, g = U[cols], g[cols]
    diag = np.einsum("kii->ki", U)
    scale = 1.0 / (1.0 + np.sqrt(diag))
    return dict(_step(U, g, scale, radius, min_diag, max_diag), cols=cols, scale=scale, gradient=g, cost=cost, fixed_cost=fixed)


def _step(U, g, scale, radius, min_diag, max_diag):
    Us = U * scale[:, :, None] * scale[:, None, :]
    gs = g * scale
    D2 = np.clip(np.einsum("kii->ki", Us), min_diag, max_diag) / radius
    S = Us + np.einsum("ki,ij->kij", D2, np.eye(6))
    ok = True
    y = np.zeros_like(gs)
    for k in range(len(S)):
        try:
            L = np.linalg.cholesky(S[k])
            y[k] = np.linalg.solve(L.T, np.linalg.solve(L, gs[k]))
        except np.linalg.LinAlgError:
            ok = False
    ok = ok and bool(np.all(np.isfinite(y)))
    # -m^T (r + m / 2) with m = J step, step = -y:  y^T gs - y^T Us y / 2
    mcc = float(np.sum(y * gs) - 0.5 * np.einsum("ki,kij,kj->", y, Us, y))
    return dict(S=S, rhs=gs, delta=-y * scale, model_cost_change=mcc, linear_solver_ok=ok)


def solve(p, cams=None, xyz=None, **options):
    """Runs the loop.  Returns dict(iterations=[dict], states=[cameras after every logged iteration], cams, initial_cost, final_cost,
    fixed_cost, num_residual_blocks, message)."""
    o = dict(DEFAULTS)
    for k in options:
        if k not in o:
            raise KeyError(k)
    o.update(options)
    cams = np.array(p.cams if cams is None else cams, dtype=np.float64)
    cols = program_cameras(p)
    if not cols:
        raise ValueError("empty program: no free camera has a residual block")
    n_blocks = int(np.sum(np.asarray(p.obs_slot) != p.fixed_slot))

    def lin(c):
        cost, fixed, U, g = evaluate(p, c, xyz)
        return cost, fixed, U[cols], g[cols]

    cost, fixed_cost, U, g = lin(cams)
    scale = 1.0 / (1.0 + np.sqrt(np.einsum("kii->ki", U)))
    radius, dec = o["initial_trust_region_radius"], 2.0
    its = [dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()),
                gradient_norm=float(np.linalg.norm(g)), step_norm=0.0, relative_decrease=0.0, trust_region_radius=radius,
                model_cost_change=0.0)]
    states = [cams.copy()]
    minimum_cost, invalid, message = cost, 0, None
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
        st = _step(U, g, scale, radius, o["min_lm_diagonal"], o["max_lm_diagonal"])
        it["model_cost_change"] = st["model_cost_change"]
        if not (st["linear_solver_ok"] and st["model_cost_change"] > 0.0):
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                message = "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps."
                its.append(it); states.append(cams.copy())
                break
            radius /= dec
            dec *= 2.0
            it["trust_region_radius"] = radius
            its.append(it); states.append(cams.copy())
            continue
        invalid = 0
        it["step_is_valid"] = 1
        cand = cams.copy()
        cand[cols] += st["delta"]
        it["step_norm"] = float(np.linalg.norm(st["delta"]))
        x_norm = float(np.linalg.norm(cams[cols]))
        if it["step_norm"] <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            message = "Parameter tolerance reached."
            break
        cand_cost, _, _, _ = evaluate(p, cand, xyz, blocks=False)
        it["cost_change"] = cost - cand_cost
        if abs(it["cost_change"]) <= o["function_tolerance"] * cost:
            message = "Function tolerance reached."
            break
        rho = it["cost_change"] / st["model_cost_change"]
        it["relative_decrease"] = rho
        if rho > o["min_relative_decrease"]:
            cams = cand
            cost, _, U, g = lin(cams)
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            dec = 2.0
            it.update(step_is_successful=1, cost=cost, gradient_max_norm=float(np.abs(g).max()), gradient_norm=float(np.linalg.norm(g)))
            minimum_cost = min(minimum_cost, cost)
        else:
            radius /= dec
            dec *= 2.0
            it["cost"] = cand_cost       # Ceres >= 1.12 logs the candidate's cost for a rejected step
        it["trust_region_radius"] = radius
        its.append(it); states.append(cams.copy())
    return dict(iterations=its, states=states, cams=cams, initial_cost=its[0]["cost"] + fixed_cost, final_cost=minimum_cost + fixed_cost,
                fixed_cost=fixed_cost, num_residual_blocks=n_blocks, message=message)


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


def pose_error(cam, cam_gt):
    """(rotation angle [rad], translation distance |t - t_gt|) between two world->camera parameter vectors [w, t], the form
    meta['cams_gt'] holds."""
    from scipy.spatial.transform import Rotation
    Ra, Rb = Rotation.from_rotvec(cam[:3]), Rotation.from_rotvec(cam_gt[:3])
    return float(np.linalg.norm((Ra * Rb.inv()).as_rotvec())), float(np.linalg.norm(cam[3:] - cam_gt[3:]))


# ---- the tracking case: ONE camera against a map whose points stay put ------------------------------------------------------------
TRACKING_SHAPES = {      # the three shapes of the tracking bar: size, K, radius, depth noise
    "120x160-r1-exact": dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), radius=1, depth_noise=0.0),
    # (scene seed 1: with seed 0 the 1 % depth noise alone puts the minimum of this shape 21-23 mm from the ground truth -- measured on
    # the yardstick, independent of the start and of the tolerances --, i.e. beyond the bar before any solver runs)
    "120x160-r2-noise": dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0), radius=2, depth_noise=0.01, seed_offset=1),
    "188x620-r1-noise": dict(size=(188, 620), K=(359.428, 359.428, 303.5964, 92.60785), radius=1, depth_noise=0.01),
}
TRACK_BAR_M, TRACK_BAR_RAD = 0.02, 1.75e-3      # one sigma of make_window's `trans` / `rot_deg` defaults (0.02 m, 0.1 degree)


def tracking_window(shape, n_frames=5, n_points=400, huber=0.05):
    from photobundle_amd import synthetic
    return synthetic.make_window(n_frames=n_frames, n_points=n_points, huber=huber, **TRACKING_SHAPES[shape])


def tracking_problem(p, start, slot=None):
    """The window `p` reduced to the tracking problem of its frame `slot` (default: the last): only that frame's residual blocks, every
    other camera at its ground truth (none of them has a residual block, so none is in the program), the tracked camera at `start`:
    "velocity" = the constant-velocity prediction from the two frames before it, "zero" = zero motion (the previous frame's pose)."""
    from photobundle_amd import se3
    from photobundle_amd.problem import WindowProblem
    slot = p.n_frames - 1 if slot is None else slot
    T = p.meta["T_gt"]
    if start == "velocity":
        T0 = T[slot - 1] @ (np.linalg.inv(T[slot - 2]) @ T[slot - 1])
    elif start == "zero":
        T0 = T[slot - 1]
    else:
        raise KeyError(start)
    keep = np.asarray(p.obs_slot) == slot
    pts = np.unique(p.obs_point[keep])
    remap = -np.ones(p.n_points, np.int64)
    remap[pts] = np.arange(len(pts))
    cams = np.array(p.meta["cams_gt"], dtype=np.float64)
    cams[slot] = se3.pose_to_params(np.linalg.inv(T0))
    return WindowProblem(K=p.K, radius=p.radius, planes=p.planes, cams=cams, xyz=p.xyz[pts].copy(), desc=p.desc[pts],
                         obs_point=remap[p.obs_point[keep]].astype(np.int32), obs_slot=p.obs_slot[keep].astype(np.int32),
                         weights=p.weights, huber=p.huber, fixed_slot=0, images=p.images, meta=dict(p.meta, tracked_slot=slot),
                         channels=p.channels, channel_images=p.channel_images)


# ---- the windows of the device trace tests --------------------------------------------------------------------------------------------
_SMALL = dict(size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
_LONG = dict(size=(120, 200), K=(250.0, 250.0, 100.0, 60.0))
TRACE_CASES = {
    # name: (make_window arguments, fixed_slot, extras)
    "3-frames-r1-huber": (dict(n_frames=3, n_points=200, radius=1, huber=0.05, seed_offset=1, **_SMALL), 0, ()),
    "5-frames-r2-no-fixed": (dict(n_frames=5, n_points=200, radius=2, seed_offset=2, **_SMALL), -1, ()),
    "8-frames-r1-huber-middle-fixed-causal": (dict(n_frames=8, n_points=200, radius=1, huber=0.05, visibility="causal", seed_offset=3, **_LONG), 3, ()),
    "20-frames-r1-causal": (dict(n_frames=20, n_points=150, radius=1, visibility="causal", seed_offset=2, **_SMALL), 0, ()),
    "4-frames-r2-gaussian-huber": (dict(n_frames=4, n_points=200, radius=2, huber=0.05, gaussian=True, seed_offset=4, **_SMALL), 0, ()),
    "4-frames-r1-3-channels": (dict(n_frames=4, n_points=150, radius=1, seed_offset=5, **_SMALL), 0, ("channels3",)),
    "4-frames-r1-camera-without-blocks": (dict(n_frames=4, n_points=200, radius=1, huber=0.05, seed_offset=6, **_SMALL), 0, ("drop-slot-2",)),
    "4-frames-r2-inverse-depth": (dict(n_frames=4, n_points=200, radius=2, seed_offset=7, **_SMALL), 0, ("inverse-depth",)),
    "tracking-5-frames-r1": (None, 0, ("tracking",)),
}


def trace_case(name):
    """(problem, extras) of a trace case.  "drop-slot-2": slot 2 keeps no residual block (a free camera outside the program);
    "inverse-depth": the engine is given rays + inverse depths (the points the yardstick uses are then the engine's own world points);
    "tracking": the tracking problem of the first tracking shape from the constant-velocity prediction."""
    from photobundle_amd import synthetic
    kw, fixed, extras = TRACE_CASES[name]
    if "tracking" in extras:
        return tracking_problem(tracking_window(sorted(TRACKING_SHAPES)[0]), "velocity"), extras
    if "channels3" in extras:
        kw = dict(kw, channel_fn=synthetic.channel_fn("IntensityAndGradient"))
    p = synthetic.make_window(**kw)
    p.fixed_slot = fixed
    if "drop-slot-2" in extras:
        keep = np.asarray(p.obs_slot) != 2
        p.obs_point, p.obs_slot = p.obs_point[keep], p.obs_slot[keep]
        assert len(np.unique(p.obs_point)) == p.n_points
    return p, extras
